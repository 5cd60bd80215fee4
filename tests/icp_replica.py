"""A float64 numpy restatement of the ICP contract of include/spr.h ("ICP for all pairs"): test infrastructure, written
from that text.  Brute force: the n x m matrix of d2 and argmin, so that ties go to the lowest index; np.linalg.svd for
the Kabsch solve.  One pair per call.

perturb: every solved pose T_{k+1} is multiplied element-wise by 1 + perturb * (+-1) (a fixed sign pattern) before it
is evaluated -- the stability condition of tests/test_icp_host.py: a case whose integer outputs survive a relative
2^-40 there can only disagree with the kernel in its integers if the kernel is wrong."""
import numpy as np

_SIGNS = np.array([[1, -1, 1, -1], [-1, 1, 1, 1], [1, 1, -1, -1]], dtype=np.float64)


def transform(T, x):
    """s'[k] = ((R[k][0] x + R[k][1] y) + R[k][2] z) + t[k], one rounding per operation."""
    x = x.astype(np.float64)
    return np.stack([((T[k, 0] * x[:, 0] + T[k, 1] * x[:, 1]) + T[k, 2] * x[:, 2]) + T[k, 3] for k in range(3)], 1)


def evaluate(src, tgt, T, max_dist):
    """E(T): (corr int32 [n], count, fitness, inlier_rmse, the transformed source)."""
    a, b = transform(T, src), tgt.astype(np.float64)
    n, m = len(a), len(b)
    corr = np.full(n, -1, dtype=np.int32)
    best = np.zeros(n)
    if n and m:
        dx, dy, dz = (a[:, None, k] - b[None, :, k] for k in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        j = np.argmin(d2, axis=1)                      # the first minimum: the lowest index among equals
        best = d2[np.arange(n), j]
        hit = best < max_dist * max_dist               # strict
        corr[hit] = j[hit]
    count = int((corr >= 0).sum())
    fitness = count / n if n else 0.0
    rmse = float(np.sqrt(best[corr >= 0].sum() / count)) if count else 0.0
    return corr, count, fitness, rmse, a


def kabsch(a, b):
    """Umeyama without scale: R from the SVD of sum (a - mean a)(b - mean b)^T, sign fix at det <= 0, t = mean b - R mean a."""
    if len(a) == 0:
        return np.hstack([np.eye(3), np.zeros((3, 1))])
    ca, cb = a.mean(0), b.mean(0)
    cov = (a - ca).T @ (b - cb) / len(a)
    U, _, Vt = np.linalg.svd(cov)
    V = Vt.T
    R = V @ U.T
    if np.linalg.det(R) <= 0:
        V[:, 2] = -V[:, 2]
        R = V @ U.T
    return np.hstack([R, (cb - R @ ca)[:, None]])


def compose(U, T):
    return np.hstack([U[:, :3] @ T[:, :3], (U[:, :3] @ T[:, 3] + U[:, 3])[:, None]])


def icp(src, tgt, pose_init, max_dist, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, perturb=0.0):
    """One pair.  Returns the outputs of the contract, plus 'trace': corr of every pass."""
    T = np.array(pose_init, dtype=np.float64)[:3, :4]
    if not (np.isfinite(src).all() and np.isfinite(tgt).all() and np.isfinite(T).all()):
        return dict(status=-1, pose64=T, pose=T.astype(np.float32), fitness=0.0, inlier_rmse=0.0, iterations=0, count=0,
                    corr=np.full(len(src), -1, dtype=np.int32), trace=[])
    corr, count, fit, rmse, a = evaluate(src, tgt, T, max_dist)
    trace, k = [corr], 0
    while k < max_iter:
        U = kabsch(a[corr >= 0], tgt[corr[corr >= 0]].astype(np.float64))
        T = compose(U, T)
        if perturb:
            T = T * (1.0 + perturb * _SIGNS)
        prev = (fit, rmse)
        corr, count, fit, rmse, a = evaluate(src, tgt, T, max_dist)
        trace.append(corr)
        k += 1
        if abs(fit - prev[0]) < rel_fitness and abs(rmse - prev[1]) < rel_rmse:
            break
    return dict(status=0, pose64=T, pose=T.astype(np.float32), fitness=fit, inlier_rmse=rmse, iterations=k, count=count,
                corr=corr, trace=trace)
