"""The cases of the ICP tests (tests/test_icp_host.py, tests/test_gpu_icp.py, tests/test_gpu_icp_guarded.py): the
smallest shapes at which the kernels of csrc/icp.hip can still go wrong, and their replica results, computed once.

A case is one CALL: src / tgt (lists of float32 [n, 3]), pose (float64 [nb, 3, 4], the initial poses), max_dist,
max_iter.  snap: two passes from a small perturbation; slide: six passes from a large one, with wrong partners among
the first correspondences; ragged: five pairs of sizes (729, 510), (1, 1), (257, 300), (5, 0), (0, 7) -- more than one
association block, a partial block, one-point and empty clouds; boundary (max_iter = 0): the strict threshold, ties,
duplicates, lattice coordinates that are exact multiples of the cell edge, negative coordinates; far: two clusters of
10 points 10^4 apart (table capacity: the cells grow coarser); nonfinite: one NaN in pair 1 of 3."""
import functools

import numpy as np

import icp_replica as R

F32, F64 = np.float32, np.float64
ITERATED = ("snap", "slide", "ragged", "far")


def axis_angle(axis, deg):
    """Rodrigues' rotation in float64."""
    k = np.asarray(axis, dtype=F64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def rigid(axis, deg, t):
    return np.hstack([axis_angle(axis, deg), np.asarray(t, dtype=F64)[:, None]])


def apply(T, x):
    return x.astype(F64) @ T[:, :3].T + T[:, 3]


GT = rigid((1, 2, 3), 25.0, (0.7, -0.3, 0.2))


@functools.lru_cache(maxsize=None)
def lattice_pair():
    """Source: a 9 x 9 x 9 lattice of spacing 1, centred, jittered by +-0.1 (729 points); target: GT applied in float64,
    rounded to float32, a random 70 % kept (510 points)."""
    rng = np.random.default_rng(3)
    g = np.arange(9, dtype=F64) - 4.0
    src = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    src = (src + rng.uniform(-0.1, 0.1, src.shape)).astype(F32)
    keep = np.sort(rng.permutation(len(src))[:510])
    return src, apply(GT, src).astype(F32)[keep]


def _cloud_pair(n, m, seed, pose):
    """n random source points in [-2, 2]^3; target: their images under `pose` (float32) with 0.01 of noise, shuffled,
    cut or filled with random points to m."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-2, 2, (n, 3)).astype(F32)
    tgt = (apply(pose, src) + rng.normal(0, 0.01, (n, 3)))[rng.permutation(n)]
    if m > n:
        tgt = np.concatenate([tgt, rng.uniform(-3, 3, (m - n, 3))])
    return src, tgt[:m].astype(F32)


def _empty():
    return np.zeros((0, 3), dtype=F32)


def _boundary():
    """max_iter = 0, max_dist 0.5: cell edge 0.5 (1 + 2^-8) = 0.501953125, exact in float32."""
    h = F32(0.501953125)
    I = rigid((0, 0, 1), 0.0, (0, 0, 0))
    o = np.zeros((1, 3), dtype=F32)
    at = np.array([[0.5, 0, 0], [-0.5, 0, 0]], dtype=F32)             # exactly at the threshold: strict, no match
    g = (np.arange(7) - 3).astype(F32) * h                            # lattice ON the cell faces, negative half included
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F32)
    rng = np.random.default_rng(11)
    probes = np.concatenate([lat[::3], lat[1::5] + F32(0.25) * h, lat[2::7] - rng.uniform(0, 0.3, lat[2::7].shape).astype(F32),
                             lat[:9] + np.array([0.5, 0, 0], dtype=F32),
                             lat[-9:] + np.array([0.5, 0, 0], dtype=F32),      # exactly 0.5 outside the lattice: no match
                             lat[-3:] + np.array([40.0, 0, 0], dtype=F32)]).astype(F32)
    ties = np.array([[0.3, 0, 0], [-0.3, 0, 0], [0, 0.3, 0], [1, 1, 1], [1, 1, 1], [1, 1, 1]], dtype=F32)   # equidistant; duplicates
    src = [o, o, np.array([[0, 0, 0], [1.05, 1, 1], [0, -0.05, 0]], dtype=F32), probes, (-probes[::2]).astype(F32)]
    tgt = [at, np.concatenate([at, np.array([[0.25, 0, 0]], dtype=F32)]), ties, lat, lat[::-1].copy()]
    pose = np.stack([I, I, I, I, rigid((0, 0, 1), 90.0, (0, 0, 0))])
    return dict(src=src, tgt=tgt, pose=pose, max_dist=0.5, max_iter=0)


@functools.lru_cache(maxsize=None)
def case(name):
    src, tgt = lattice_pair()
    if name == "snap":
        init = R.compose(rigid((3, -1, 2), 1.0, (0.05, -0.04, 0.03)), GT)
        return dict(src=[src], tgt=[tgt], pose=init[None], max_dist=0.4, max_iter=30)
    if name == "slide":
        init = R.compose(rigid((3, -1, 2), 3.0, (0.45, 0.2, -0.1)), GT)
        return dict(src=[src], tgt=[tgt], pose=init[None], max_dist=0.75, max_iter=30)
    if name == "ragged":
        p2 = rigid((1, -1, 0.5), 10.0, (0.2, 0.1, -0.3))
        s2, t2 = _cloud_pair(257, 300, 21, p2)
        one = np.array([[0.25, -0.5, 1.0]], dtype=F32)
        return dict(src=[src, one, s2, np.arange(15, dtype=F32).reshape(5, 3), _empty()],
                    tgt=[tgt, apply(GT, one).astype(F32) + F32(0.05), t2, _empty(), np.arange(21, dtype=F32).reshape(7, 3)],
                    pose=np.stack([R.compose(rigid((3, -1, 2), 1.0, (0.05, -0.04, 0.03)), GT), GT,
                                   R.compose(rigid((0, 1, 0), 0.5, (0.02, -0.01, 0.01)), p2), GT, GT]),
                    max_dist=0.4, max_iter=30)
    if name == "boundary":
        return _boundary()
    if name == "far":
        rng = np.random.default_rng(5)
        s = np.concatenate([rng.uniform(-1, 1, (10, 3)), rng.uniform(-1, 1, (10, 3)) + np.array([1.0e4, 0, 0])]).astype(F32)
        p = rigid((0, 0, 1), 0.001, (0.05, -0.02, 0.03))
        return dict(src=[s], tgt=[apply(p, s).astype(F32)], pose=rigid((0, 0, 1), 0.0, (0, 0, 0))[None], max_dist=0.5,
                    max_iter=10)
    if name == "nonfinite":
        parts = [_cloud_pair(50, 60, 31 + b, GT) for b in range(3)]
        bad = parts[1][0].copy()
        bad[17, 1] = np.nan
        return dict(src=[parts[0][0], bad, parts[2][0]], tgt=[p[1] for p in parts],
                    pose=np.stack([R.compose(rigid((1, 0, 0), 0.5, (0.01, 0.01, 0.01)), GT)] * 3), max_dist=0.4, max_iter=30)
    raise KeyError(name)


CASES = ("snap", "slide", "ragged", "boundary", "far", "nonfinite")


@functools.lru_cache(maxsize=None)
def replica(name, perturb=0.0, max_iter=None):
    """The replica's result for every pair of the case's call (max_iter: the case's own unless given)."""
    c = case(name)
    it = c["max_iter"] if max_iter is None else max_iter
    return [R.icp(s, t, p, c["max_dist"], it, perturb=perturb) for s, t, p in zip(c["src"], c["tgt"], c["pose"])]


def pose_error(T, gt=GT):
    return float(np.abs(np.asarray(T, dtype=F64) - gt).max())
