"""A float64 numpy restatement of the point-to-plane ICP contract of include/spr.h ("Point-to-plane ICP for all pairs"):
test infrastructure, written from that text.  The evaluation E(T), transform and compose are tests/icp_replica.py's
(brute-force association, ties to the lowest index); the normal equations are summed by numpy (another order than the
kernel's), the LDL^T and the step are written out operation by operation.  One pair per call.

perturb: as in tests/icp_replica.py, every solved pose T_{k+1} is multiplied element-wise by 1 + perturb * (+-1) before
it is evaluated -- the stability condition of tests/test_icp_plane_host.py."""
import numpy as np

import icp_replica as R

KERNELS = ("l2", "huber", "tukey")
PIVOT = 1e-12


def weights(r, kernel, k):
    ar = np.abs(r)
    if kernel == "l2":
        return np.ones_like(r)
    with np.errstate(divide="ignore", invalid="ignore"):
        if kernel == "huber":
            return np.where(ar <= k, 1.0, k / ar)
        q = r / k
        u = 1.0 - q * q
        return np.where(ar <= k, u * u, 0.0)


def residuals(a, b, n):
    e = a - b
    return (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]


def normal_equations(a, b, n, c, kernel, k):
    """(A [6, 6] symmetric, g [6], r) of the matched rows a (transformed source), b (partners), n (their normals)."""
    r = residuals(a, b, n)
    p = a - c
    J = np.stack([p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2],
                  p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]], 1)
    wJ = weights(r, kernel, k)[:, None] * J
    A = np.zeros((6, 6))
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = (wJ[:, i] * J[:, j]).sum()
    return A, (wJ * r[:, None]).sum(0), r


def ldlt_solve(A, g):
    """x of A x = -g by unpivoted LDL^T in the contract's order, or None when a pivot is not > 1e-12 max_i A_ii."""
    m = max(A[i, i] for i in range(6))
    L, d = np.zeros((6, 6)), np.zeros(6)
    for k in range(6):
        dk = A[k, k]
        for p in range(k):
            dk = dk - (L[k, p] * d[p]) * L[k, p]
        if not dk > PIVOT * m:
            return None
        d[k] = dk
        for i in range(k + 1, 6):
            s = A[i, k]
            for p in range(k):
                s = s - (L[i, p] * d[p]) * L[k, p]
            L[i, k] = s / dk
    y, x = np.zeros(6), np.zeros(6)
    for i in range(6):
        s = -g[i]
        for p in range(i):
            s = s - L[i, p] * y[p]
        y[i] = s
    for i in range(5, -1, -1):
        s = y[i] / d[i]
        for p in range(i + 1, 6):
            s = s - L[p, i] * x[p]
        x[i] = s
    return x


def step(x, c):
    """U [3, 4] = [Rz(x2) Ry(x1) Rx(x0) | v - omega x c]."""
    sx, cx, sy, cy, sz, cz = np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]), np.sin(x[2]), np.cos(x[2])
    t = [x[3] - (x[1] * c[2] - x[2] * c[1]), x[4] - (x[2] * c[0] - x[0] * c[2]), x[5] - (x[0] * c[1] - x[1] * c[0])]
    return np.array([[cz * cy, (cz * sy) * sx - sz * cx, (cz * sy) * cx + sz * sx, t[0]],
                     [sz * cy, (sz * sy) * sx + cz * cx, (sz * sy) * cx - cz * sx, t[1]],
                     [-sy, cy * sx, cy * cx, t[2]]])


def icp(src, tgt, nrm, pose_init, max_dist, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, kernel="l2", kernel_k=None,
        perturb=0.0):
    """One pair.  The outputs of the contract, plus 'trace' (corr of every pass), 'resid' (the matched residuals r of
    every pass that was followed by a step) and 'refused' (per step: the solve was refused, U = I)."""
    T = np.array(pose_init, dtype=np.float64)[:3, :4]
    if not (np.isfinite(src).all() and np.isfinite(tgt).all() and np.isfinite(nrm).all() and np.isfinite(T).all()):
        return dict(status=-1, pose64=T, pose=T.astype(np.float32), fitness=0.0, inlier_rmse=0.0, iterations=0, count=0,
                    corr=np.full(len(src), -1, dtype=np.int32), trace=[], resid=[], refused=[])
    b64, n64 = tgt.astype(np.float64), nrm.astype(np.float64)
    c = b64.min(0) if len(b64) else np.zeros(3)
    corr, count, fit, rmse, a = R.evaluate(src, tgt, T, max_dist)
    trace, resid, refused, k = [corr], [], [], 0
    while k < max_iter:
        hit = corr >= 0
        U = np.hstack([np.eye(3), np.zeros((3, 1))])
        x = None
        if count:
            A, g, r = normal_equations(a[hit], b64[corr[hit]], n64[corr[hit]], c, kernel, kernel_k)
            resid.append(r)
            x = ldlt_solve(A, g)
        if x is not None:
            U = step(x, c)
        refused.append(x is None)
        T = R.compose(U, T)
        if perturb:
            T = T * (1.0 + perturb * R._SIGNS)
        prev = (fit, rmse)
        corr, count, fit, rmse, a = R.evaluate(src, tgt, T, max_dist)
        trace.append(corr)
        k += 1
        if abs(fit - prev[0]) < rel_fitness and abs(rmse - prev[1]) < rel_rmse:
            break
    return dict(status=0, pose64=T, pose=T.astype(np.float32), fitness=fit, inlier_rmse=rmse, iterations=k, count=count,
                corr=corr, trace=trace, resid=resid, refused=refused)
