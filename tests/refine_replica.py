"""TEST INFRASTRUCTURE ONLY -- numpy restatement of spr_refine_pairs for ONE pair, written from the contract in
include/spr.h (steps 1-7), not from any implementation.

The selections (ratio test, median threshold, overlap product, top-k) are defined on float32 values, so they are
computed in float32 here -- one rounding per operation, as the contract says -- and every discrete choice is exact.
The pose solves and the LGR residuals run in float64: they are what the float32 kernels are measured against.
`trace` collects the quantities a test needs to prove its inputs keep a gap at every discrete choice.
"""
import numpy as np


def kabsch(a, b, w):
    """compute_rigid_transform (weights normalised by max(sum w, 1e-6)), float64, [3,4]."""
    a, b, w = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(w, np.float64)
    if a.shape[0] == 0:
        return np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    wn = w / max(w.sum(), 1e-6)
    ca, cb = (wn[:, None] * a).sum(0), (wn[:, None] * b).sum(0)
    H = (a - ca).T @ ((b - cb) * wn[:, None])
    U, S, Vt = np.linalg.svd(H)
    V = Vt.T
    R = V @ U.T
    if np.linalg.det(R) <= 0:
        V = V.copy()
        V[:, 2] = -V[:, 2]
        R = V @ U.T
    return np.concatenate([R, (cb - R @ ca)[:, None]], 1)


def refine_pair(val, val2, ind, ov_src, ov_tgt, src_xyz, tgt_xyz, *, ratio=False, median=False, overlap=False,
                overlap_w=False, k=None, lgr_steps=0, lowe_thres=0.0, radius=0.0, pose_in=None, sinkhorn=False,
                trace=None):
    """val / val2 / ind: the own side's entries (the tgt tokens when N > M, else the src tokens).  Returns
    (pose [3,4] f64, val f32, ind i64, src_pts, tgt_pts)."""
    N, M = src_xyz.shape[0], tgt_xyz.shape[0]
    on_tgt = N > M
    n = min(N, M)
    f32 = np.float32
    v = np.asarray(val, f32).copy()
    ind = np.asarray(ind, np.int64)
    assert v.shape == (n,) and ind.shape == (n,)
    tr = trace if trace is not None else {}
    if ratio:
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.asarray(val2, f32) / v
        tr["ratios"] = r.copy()
        v = np.where(r < f32(lowe_thres), v, f32(0))
    if median:
        med = np.sort(v, kind="stable")[(n - 1) // 2]
        tr["median"] = (med, np.sort(v, kind="stable"))
        v = np.where(v > med, v, f32(0))
    pos = np.arange(n)
    ov = None
    if overlap:
        os_, ot_ = np.asarray(ov_src, f32).reshape(-1), np.asarray(ov_tgt, f32).reshape(-1)
        ov = (os_[ind] * ot_[pos]) if on_tgt else (os_[pos] * ot_[ind])
        if not overlap_w:
            v = (v * ov).astype(f32)
    order = pos
    if k is not None:
        order = np.lexsort((pos, -v.astype(np.float64)))[:k]      # descending value, ties to the lower position
        tr["topk"] = (v.copy(), order.copy())
    v_o = v[order]
    if sinkhorn:
        a, b = src_xyz[order], tgt_xyz[order]
    elif on_tgt:
        a, b = src_xyz[ind[order]], tgt_xyz[order]
    else:
        a, b = src_xyz[order], tgt_xyz[ind[order]]
    ind_o = order.astype(np.int64) if k is not None else ind[order]
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    if pose_in is not None:
        T = np.asarray(pose_in, np.float64)
    else:
        T = kabsch(a64, b64, (ov[order] if overlap_w else v_o))
    w = v_o.astype(np.float64)
    tr["residuals"] = []
    for _ in range(lgr_steps):
        res = np.linalg.norm(b64 - (a64 @ T[:, :3].T + T[:, 3]), axis=1)
        tr["residuals"].append(res)
        w = w * (res < radius)
        T = kabsch(a64, b64, w)
    return T, v_o, ind_o, a, b
