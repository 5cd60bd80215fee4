"""The contract of spr_eval_pairs (include/spr.h, "Registration metrics for all pairs") in numpy float64, one pair at a
time: every product and sum written out in the contract's order (numpy's elementwise float64 multiply / add / subtract
round once and are never fused), nearest neighbours by brute force with the lowest index of a tie (np.argmin).  The
mean sums are taken with math.fsum -- the exactly rounded sum -- so that the replica is within (n - 1) 2^-53 relative of
ANY summation order of the n non-negative terms."""
import math

import numpy as np

COLUMNS = ('r_mse', 'r_mae', 't_mse', 't_mae', 'err_r_deg', 'err_t', 'trans_err', 'chamfer_src', 'chamfer_ref',
           'chamfer_dist', 'inlier_count', 'inlier_ratio')


def dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def apply(T, xyz):
    """T [3,4] float64 on xyz [n,3] float32 -> [n,3] float64: ((R0 x + R1 y) + R2 z) + t per row."""
    p = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([dot3(T[k, 0], x, T[k, 1], y, T[k, 2], z) + T[k, 3] for k in range(3)], axis=1)


def compose(A, B):
    """A o B (apply B first), [3,4] each."""
    O = np.zeros((3, 4))
    for r in range(3):
        for q in range(3):
            O[r, q] = dot3(A[r, 0], B[0, q], A[r, 1], B[1, q], A[r, 2], B[2, q])
        O[r, 3] = dot3(A[r, 0], B[0, 3], A[r, 1], B[1, 3], A[r, 2], B[2, 3]) + A[r, 3]
    return O


def inverse(G):
    Gi = np.zeros((3, 4))
    Gi[:, :3] = G[:, :3].T
    for r in range(3):
        Gi[r, 3] = -dot3(G[0, r], G[0, 3], G[1, r], G[1, 3], G[2, r], G[2, 3])
    return Gi


def deg(x):
    return x * 180.0 / math.pi


def clamp1(v):
    return min(max(v, -1.0), 1.0)


def euler_xyz_deg(T):
    return np.array([deg(math.atan2(T[2, 1], T[2, 2])), deg(-math.asin(clamp1(T[2, 0]))),
                     deg(math.atan2(T[1, 0], T[0, 0]))])


def norm3(v):
    return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def d2_matrix(a, b):
    """[n, m]: ((ax-bx)^2 + (ay-by)^2) + (az-bz)^2 of float64 rows."""
    dx, dy, dz = (a[:, None, k] - b[None, :, k] for k in range(3))
    return (dx * dx + dy * dy) + dz * dz


def nearest(q, t):
    """(d2 [n] f64, nn [n] i32) of queries q against targets t, both float64 rows; t not empty."""
    d = d2_matrix(q, t)
    nn = np.argmin(d, axis=1)                    # the first (lowest) index of the minimum
    return d[np.arange(len(q)), nn], nn.astype(np.int32)


def finite(*arrays):
    return all(bool((np.abs(np.asarray(a, dtype=np.float64)) < 1e300).all()) for a in arrays)


def eval_pair(src, ref, pose_gt, pose_pred, raw=None, corr=None, acceptance_radius=None):
    """One pair.  Returns dict: the columns, 'status', and with raw: d2_src / nn_src / d2_ref / nn_ref."""
    G, P = np.asarray(pose_gt, dtype=np.float64)[:3], np.asarray(pose_pred, dtype=np.float64)[:3]
    out = {k: 0.0 for k in COLUMNS}
    ns, nt = len(src), len(ref)
    if raw is not None:
        out.update(d2_src=np.zeros(ns), nn_src=np.full(ns, -1, np.int32), d2_ref=np.zeros(nt),
                   nn_ref=np.full(nt, -1, np.int32))
    everything = [src, ref, G, P] + ([raw] if raw is not None else []) + (list(corr) if corr is not None else [])
    if not finite(*everything):
        out['status'] = -1
        return out
    out['status'] = -2 if raw is not None and len(raw) == 0 and (ns > 0 or nt > 0) else 0
    Gi = inverse(G)
    C, D = compose(Gi, P), compose(P, Gi)
    u, v = euler_xyz_deg(G) - euler_xyz_deg(P), G[:, 3] - P[:, 3]
    out['r_mse'] = ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) / 3.0
    out['r_mae'] = ((abs(u[0]) + abs(u[1])) + abs(u[2])) / 3.0
    out['t_mse'] = ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) / 3.0
    out['t_mae'] = ((abs(v[0]) + abs(v[1])) + abs(v[2])) / 3.0
    out['err_r_deg'] = deg(math.acos(clamp1(0.5 * (((C[0, 0] + C[1, 1]) + C[2, 2]) - 1.0))))
    out['err_t'] = norm3(C[:, 3])
    out['trans_err'] = norm3(D[:, 3])
    if raw is not None and out['status'] == 0:
        raw64 = np.asarray(raw, dtype=np.float64).reshape(-1, 3)
        if ns:
            out['d2_src'], out['nn_src'] = nearest(apply(P, src), raw64)
        if nt:
            out['d2_ref'], out['nn_ref'] = nearest(np.asarray(ref, dtype=np.float64), apply(D, raw))
        out['chamfer_src'] = math.fsum(out['d2_src']) / ns if ns else 0.0
        out['chamfer_ref'] = math.fsum(out['d2_ref']) / nt if nt else 0.0
        out['chamfer_dist'] = out['chamfer_src'] + out['chamfer_ref']
    if corr is not None:
        a, b = apply(G, corr[0]), np.asarray(corr[1], dtype=np.float64).reshape(-1, 3)
        dx, dy, dz = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1], a[:, 2] - b[:, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        out['inlier_count'] = float(int((d2 < acceptance_radius * acceptance_radius).sum()))
        out['inlier_ratio'] = out['inlier_count'] / len(a) if len(a) else 0.0
    return out
