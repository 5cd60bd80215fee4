"""numpy statement of the augmentation contract of include/spr.h ("8f-6"), written from the header: Philox4x32-10,
the draw mappings, the pair decisions and the float64 apply rules.  Shared by test_augment_host.py and
test_gpu_augment.py (not a test module)."""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
TAG_PAIR, TAG_NOISE, TAG_KEY = 0, 1, 2
MODES = {'none': 0, 'small': 1, 'large': 2}


def philox(ctr, key):
    """ctr [n,4], key [2] (uint32 values) -> [n,4] uint32."""
    c = np.asarray(ctr, dtype=np.uint64).reshape(-1, 4).copy()
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[:, 0], np.uint64(M1) * c[:, 2]
        n0 = (p1 >> np.uint64(32)) ^ c[:, 1] ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c[:, 3] ^ k1
        c = np.stack([n0, p1 & MASK, n2, p0 & MASK], axis=1)
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c.astype(np.uint32)


def block(seed, pair_key, side, elements, tag):
    q = (2 * int(pair_key) + int(side)) & (2 ** 64 - 1)
    e = np.asarray(elements, dtype=np.uint64).reshape(-1)
    ctr = np.stack([e, np.full_like(e, q & 0xFFFFFFFF), np.full_like(e, tag), np.full_like(e, q >> 32)], axis=1)
    return philox(ctr, (int(seed) & 0xFFFFFFFF, int(seed) >> 32))


def uniform(w):
    return ((np.asarray(w, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normal2(a, b):
    r, t = np.sqrt(-2.0 * np.log(uniform(a))), 2.0 * np.pi * uniform(b)
    return r * np.cos(t), r * np.sin(t)


def decide(seed, pair_key, mode):
    """(perturb_src, swap, P [3,4] f32, extras) of one pair."""
    b = block(seed, pair_key, 0, [0, 1, 2], TAG_PAIR)
    perturb_src, swap = bool(uniform(b[0, 0]) > 0.5), bool(uniform(b[0, 1]) > 0.5)
    R, t, extra = np.eye(3), np.zeros(3), {}
    if mode == 'small':
        std = 0.1
        z = 2.0 * uniform(b[1, 0]) - 1.0
        s, phi = math.sqrt(1.0 - z * z), 2.0 * math.pi * uniform(b[1, 1])
        k = np.array([s * math.cos(phi), s * math.sin(phi), z])
        th = float(normal2(b[1, 2], b[1, 3])[0]) * std * math.pi / math.sqrt(3.0)
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = math.cos(th) * np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * np.outer(k, k)
        t0, t1 = normal2(b[2, 0], b[2, 1])
        t2, _ = normal2(b[2, 2], b[2, 3])
        t = np.array([t0, t1, t2]) * std / math.sqrt(3.0)
        extra = {'axis': k, 'angle': th}
    elif mode == 'large':
        az, ay, ax = (2.0 * math.pi * uniform(b[1, j]) for j in range(3))
        Rz = np.array([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]])
        Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
        Rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
        R = Rx @ (Ry @ Rz)
        t = -4.0 + 8.0 * uniform(b[2, :3])
        extra = {'euler_zyx': (az, ay, ax)}
    return perturb_src, swap, np.concatenate([R, t[:, None]], axis=1).astype(np.float32), extra


def keys(seed, pair_key, side, n):
    return block(seed, pair_key, side, np.arange(n), TAG_KEY)[:, 0]


def noise64(seed, pair_key, side, n):
    """float64 Box-Muller of a cloud's tag-1 words: (noise [n,3], r [n,3] = the radius behind each component)."""
    b = block(seed, pair_key, side, np.arange(n), TAG_NOISE)
    c0, s0 = normal2(b[:, 0], b[:, 1])
    c1, _ = normal2(b[:, 2], b[:, 3])
    r0, r1 = np.sqrt(-2.0 * np.log(uniform(b[:, 0]))), np.sqrt(-2.0 * np.log(uniform(b[:, 2])))
    return np.stack([c0, s0, c1], axis=1), np.stack([r0, r0, r1], axis=1)


# ---- apply contract: float64 on the exactly converted float32 inputs, one rounding per operation -------------------
def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _dot3(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def cat(A, B):
    o = np.zeros((3, 4))
    for i in range(3):
        for j in range(3):
            o[i, j] = _dot3(A[i, 0], B[0, j], A[i, 1], B[1, j], A[i, 2], B[2, j])
        o[i, 3] = _dot3(A[i, 0], B[0, 3], A[i, 1], B[1, 3], A[i, 2], B[2, 3]) + A[i, 3]
    return o


def inv(A):
    o = np.zeros((3, 4))
    for i in range(3):
        for j in range(3):
            o[i, j] = A[j, i]
        o[i, 3] = -_dot3(A[0, i], A[0, 3], A[1, i], A[1, 3], A[2, i], A[2, 3])
    return o


def apply_pair(src, tgt, pose, P, perturb_src, swap, mode, scale, max_pts, noise_src, noise_tgt, keys_src, keys_tgt,
               src_mask=None, tgt_mask=None, corr=None):
    """One pair through the contract.  float32 inputs; noise_* [n,3] float32; keys_* [n] uint32.  Returns a dict with
    float32 src_xyz / tgt_xyz / pose, int perms, masks, corr [2,K] and the centroid used."""
    clouds = [np.asarray(src, np.float32).astype(np.float64), np.asarray(tgt, np.float32).astype(np.float64)]
    G = np.asarray(pose, np.float32).astype(np.float64)
    out_pose, centroid = G, np.zeros(3)
    if mode != 'none':
        Pd = np.asarray(P, np.float32).astype(np.float64)
        side = 0 if perturb_src else 1
        pts = clouds[side]
        if mode == 'small':
            n = pts.shape[0]
            centroid = _f32(pts.sum(axis=0) / n) if n else np.zeros(3)
            c = centroid
            for k in range(3):
                Pd[k, 3] = _dot3(Pd[k, 0], -c[0], Pd[k, 1], -c[1], Pd[k, 2], -c[2]) + (Pd[k, 3] + c[k])
            Pd = _f32(Pd)
        out_pose = _f32(cat(G, inv(Pd)) if perturb_src else cat(Pd, G))
        moved = np.stack([_dot3(Pd[k, 0], pts[:, 0], Pd[k, 1], pts[:, 1], Pd[k, 2], pts[:, 2]) + Pd[k, 3]
                          for k in range(3)], axis=1) if pts.shape[0] else pts
        clouds[side] = _f32(moved)
    sc = np.float32(scale)
    res = []
    for side, (pts, nz, ky) in enumerate(zip(clouds, (noise_src, noise_tgt), (keys_src, keys_tgt))):
        x = pts.astype(np.float32) + (np.asarray(nz, np.float32).reshape(-1, 3) * sc).astype(np.float32)
        perm = np.argsort(np.asarray(ky, dtype=np.uint32), kind='stable')[:max_pts]
        res.append((x.astype(np.float32)[perm], perm))
    masks = [None if m is None else np.asarray(m, bool)[res[s][1]] for s, m in enumerate((src_mask, tgt_mask))]
    new_corr = None
    if corr is not None:
        corr = np.asarray(corr, dtype=np.int64).reshape(2, -1)
        rev = []
        for s in range(2):
            r = np.full(clouds[s].shape[0], -1, dtype=np.int64)
            r[res[s][1]] = np.arange(res[s][1].shape[0])
            rev.append(r)
        new_corr = np.stack([rev[0][corr[0]], rev[1][corr[1]]])
        new_corr = new_corr[:, np.all(new_corr >= 0, axis=0)]
    if swap:
        res, masks = res[::-1], masks[::-1]
        new_corr = None if new_corr is None else new_corr[::-1].copy()
        out_pose = _f32(inv(out_pose))
    return {'src_xyz': res[0][0], 'tgt_xyz': res[1][0], 'src_perm': res[0][1], 'tgt_perm': res[1][1],
            'pose': out_pose.astype(np.float32), 'src_mask': masks[0], 'tgt_mask': masks[1], 'corr': new_corr,
            'centroid': centroid}
