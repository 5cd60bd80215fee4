"""numpy statement of the ModelNet pair contract of include/spr.h ("8f-7"), written from the header: the draw
mappings of tags 16-20 and the float64 apply rules (centre, crop, overlap, transform, resample, jitter, shuffle).
Shared by test_modelnet_pairs_host.py, test_gpu_modelnet_pairs.py and scripts/gen_modelnet_pairs_golden.py (not a test
module)."""
import math

import numpy as np

from augment_replica import block, normal2, uniform

TAG_PAIR, TAG_RESAMPLE, TAG_EXTRA, TAG_NOISE, TAG_SHUFFLE = 16, 17, 18, 19, 20


def percentile_q(p):
    """The reference's (1.0 - p_keep) * 100 with p_keep a numpy float32 scalar, as a Python float."""
    return float((1.0 - np.float32(p)) * 100)


# ---- draws -----------------------------------------------------------------------------------------------------------
def decide(seed, pair_key, rot_mag, trans_mag):
    """(dirs [2,3] f64, transform [3,4] f32) of one pair: tag 16, float64, libm."""
    dirs = np.zeros((2, 3))
    for side in range(2):
        w = block(seed, pair_key, side, [0], TAG_PAIR)[0]
        phi, z = 2.0 * math.pi * float(uniform(w[0])), 2.0 * float(uniform(w[1])) - 1.0
        th = math.acos(z)
        dirs[side] = (math.sin(th) * math.cos(phi), math.sin(th) * math.sin(phi), math.cos(th))
    b = block(seed, pair_key, 0, [1, 2], TAG_PAIR)
    ax, ay, az = (float(uniform(b[0, j])) * math.pi * rot_mag / 180.0 for j in range(3))
    Rx = [[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]]
    Ry = [[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]]
    Rz = [[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]]

    def mul(A, B):
        return [[(A[i][0] * B[0][j] + A[i][1] * B[1][j]) + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]
    R = np.array(mul(mul(Rx, Ry), Rz), dtype=np.float64)
    t = np.array([-trans_mag + 2.0 * trans_mag * float(uniform(b[1, j])) for j in range(3)])
    return dirs, np.concatenate([R, t[:, None]], axis=1).astype(np.float32)


def resample_keys(seed, pair_key, side, n):
    return block(seed, pair_key, side, np.arange(n), TAG_RESAMPLE)[:, 0]


def extra_words(seed, pair_key, side, k):
    return block(seed, pair_key, side, np.arange(k), TAG_EXTRA)[:, 0]


def shuffle_keys(seed, pair_key, side, k):
    return block(seed, pair_key, side, np.arange(k), TAG_SHUFFLE)[:, 0]


def noise64(seed, pair_key, side, k):
    """float64 Box-Muller of the tag-19 words: (noise [k,3], r [k,3] = the radius behind each component)."""
    b = block(seed, pair_key, side, np.arange(k), TAG_NOISE)
    c0, s0 = normal2(b[:, 0], b[:, 1])
    c1, _ = normal2(b[:, 2], b[:, 3])
    r0, r1 = np.sqrt(-2.0 * np.log(uniform(b[:, 0]))), np.sqrt(-2.0 * np.log(uniform(b[:, 2])))
    return np.stack([c0, s0, c1], axis=1), np.stack([r0, r0, r1], axis=1)


# ---- apply contract ----------------------------------------------------------------------------------------------------
def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def cloud_sum(x):
    """The float64 sum of a cloud [n,3] in the contract's fixed order."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    n = x.shape[0]
    rows = max(1, -(-n // 1024))
    pad = np.zeros((rows * 1024, 3))          # + 0.0 changes no partial (none is -0.0: every partial starts from +0.0)
    pad[:n] = x
    pad = pad.reshape(rows, 1024, 3)
    p = np.zeros((1024, 3))
    for r in range(rows):
        p = p + pad[r]
    idx = np.arange(1024)
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[idx ^ o]
    s = np.zeros(3)
    for w in range(16):
        s = s + p[64 * w]
    return s


def crop_threshold(d, q):
    """numpy's 'linear' percentile of d at q, as the contract writes it out."""
    n = d.shape[0]
    h = (n - 1) * (q / 100.0)
    lo = min(max(int(math.floor(h)), 0), n - 1)
    hi = min(lo + 1, n - 1)
    s = np.sort(d)
    t, a, b = h - lo, s[lo], s[hi]
    return a + (b - a) * t if t < 0.5 else b - (b - a) * (1.0 - t)


def crop(x, c, direction, p, q):
    """(mask [n] bool, d [n] f64, thr) of one side."""
    v = _f32(x - c)
    d = _dot3(v[:, 0], direction[0], v[:, 1], direction[1], v[:, 2], direction[2])
    p = np.float32(p)
    if p == np.float32(1.0):
        return np.ones(x.shape[0], bool), d, -np.inf
    thr = 0.0 if p == np.float32(0.5) else crop_threshold(d, q)
    return d > thr, d, thr


def make_pair(xyz, p, q, k, scale, clip, transform, dirs, rkeys, extra, noise, skeys):
    """One pair through the contract.  xyz [n,3] float32; p, q: per-side (source, reference) p_keep and percentile;
    transform [3,4] f32; dirs [2,3] f64; per side: rkeys [n] u32, extra [k] u32 (words), noise [k,3] f32, skeys [k] u32.
    Returns float32 src_xyz / tgt_xyz / pose, uint8 overlaps, int indices, corr [2,K], status and intermediates."""
    x = np.asarray(xyz, np.float32).astype(np.float64).reshape(-1, 3)
    n = x.shape[0]
    T = np.asarray(transform, np.float32).astype(np.float64)
    pose = np.zeros((3, 4))
    for i in range(3):
        pose[i, :3] = T[:3, i]
        pose[i, 3] = -_dot3(T[0, i], T[0, 3], T[1, i], T[1, 3], T[2, i], T[2, 3])
    out = {"pose": pose.astype(np.float32), "status": 0, "corr": np.zeros((2, 0), np.int64)}
    for s in ("src", "tgt"):
        out[s + "_xyz"] = np.zeros((k, 3), np.float32)
        out[s + "_overlap"] = np.zeros(k, np.uint8)
        out[s + "_index"] = np.zeros(k, np.int64)
    if not (np.isfinite(x).all() and np.isfinite(T).all() and np.isfinite(np.asarray(dirs)).all()):
        out["status"] = 1
        return out
    c = _f32(cloud_sum(x) / n) if n else np.zeros(3)
    masks, ds, thrs = zip(*(crop(x, c, np.asarray(dirs, np.float64)[s], p[s], q[s]) for s in range(2))) if n else \
        ((np.zeros(0, bool),) * 2, (np.zeros(0),) * 2, (0.0, 0.0))
    out.update(crop_masks=masks, d=ds, thr=thrs, centroid=c)
    if not (masks[0].any() and masks[1].any()):
        out["status"] = 2
        return out
    moved = _f32(np.stack([_dot3(T[i, 0], x[:, 0], T[i, 1], x[:, 1], T[i, 2], x[:, 2]) + T[i, 3] for i in range(3)], axis=1))
    sc, cl = np.float32(scale), np.float32(clip)
    final = []                                                  # per side: raw index -> output slot, or -1
    for s, name in enumerate(("src", "tgt")):
        kept = np.nonzero(masks[s])[0]
        nk = kept.shape[0]
        order = kept[np.argsort(np.asarray(rkeys[s], np.uint32)[kept], kind="stable")]
        sel = order[:k]
        if nk < k:
            u = uniform(np.asarray(extra[s], np.uint32)[:k - nk])
            sel = np.concatenate([order, kept[np.floor(u * nk).astype(np.int64)]])   # extras count in raw order
        pts = (moved if s == 0 else x)[sel].astype(np.float32)
        e = np.clip((np.asarray(noise[s], np.float32).reshape(k, 3) * sc).astype(np.float32), -cl, cl)
        pts = (pts + e).astype(np.float32)
        perm = np.argsort(np.asarray(skeys[s], np.uint32)[:k], kind="stable")
        out[name + "_xyz"] = pts[perm]
        out[name + "_index"] = sel[perm]
        out[name + "_overlap"] = masks[1 - s][sel[perm]].astype(np.uint8)
        pos = np.full(n, -1, np.int64)
        pos[sel] = np.arange(k)                                  # repeated indices: the last (largest) position wins
        inv = np.empty(k, np.int64)
        inv[perm] = np.arange(k)
        final.append(np.where(pos >= 0, inv[np.maximum(pos, 0)], -1))
        out[name + "_resampled"] = sel
    both = np.nonzero((final[0] >= 0) & (final[1] >= 0))[0]
    out["corr"] = np.stack([final[0][both], final[1][both]])
    return out
