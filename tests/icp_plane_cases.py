"""The cases of the point-to-plane ICP tests (tests/test_icp_plane_host.py, tests/test_gpu_icp_plane.py,
tests/test_gpu_icp_plane_guarded.py): small surfaces with analytic normals, a few hundred points per cloud, and their
replica results (tests/icp_plane_replica.py), computed once.

A case is one CALL: src / tgt / nrm (lists of float32 [n, 3]; nrm row-aligned with tgt), pose (float64 [nb, 3, 4], the
initial poses), max_dist, max_iter, kernel, kernel_k.
The corner: three mutually orthogonal 2 x 2 faces meeting at the origin.  The source is 257 uniform points on them
(86 + 86 + 85: two association blocks, the second one with a single point); the target is an INDEPENDENT sample of 100
points per face, mapped by icp_cases.GT and rounded to float32, its normals the faces' rotated by GT and rounded.
  corner_snap / corner_slide   the starts of icp_cases' snap / slide
  ragged        five pairs: the corner, a one-point pair, a second corner (another sample, pose and start), an empty
                target, an empty source
  plane         one flat patch whose normals are all exactly (0, 0, 1): three columns of J are exactly zero, the third
                pivot is an exact zero, U = I, one step, the pose stays pose_init bit for bit
  zero_normals  the corner with every fifth target normal zero
  robust_*      the corner with 30 of the 300 target points pushed 0.15 .. 0.3 off their face along the normal, run
                with each kernel; kernel_k = 0.1 lies between the inliers' and the outliers' residuals
  far           the corner shifted by 1e4 on x (float32 spacing there: 1e-3), a nearly pure translation to recover
  nonfinite     three small corners, a NaN in one normal of pair 1"""
import functools

import numpy as np

import icp_cases as C0
import icp_plane_replica as P
import icp_replica as R

F32, F64 = np.float32, np.float64
GT = C0.GT
FACE_NORMALS = np.eye(3)[::-1].copy()          # face 0: z = 0, face 1: y = 0, face 2: x = 0


def faces(counts, seed, lo=0.0):
    """Uniform points on the three faces (counts per face; [lo, 2] x [lo, 2] of each), and their normals; float64, the
    corner's own frame."""
    rng = np.random.default_rng(seed)
    pts, nrm = [], []
    for f, n in enumerate(counts):
        uv = rng.uniform(lo, 2.0, (n, 2))
        p = np.insert(uv, 2 - f, 0.0, axis=1)          # the zero goes to z, y, x
        pts.append(p)
        nrm.append(np.repeat(FACE_NORMALS[f][None], n, 0))
    return np.concatenate(pts), np.concatenate(nrm)


SRC_MARGIN = 0.35      # the source keeps off the shared edges: at the ground truth its partners lie on its own face


def corner(src_counts=(86, 86, 85), tgt_counts=(100, 100, 100), seed=7, pose=GT, shift=(0.0, 0.0, 0.0)):
    """(src, tgt, nrm) float32: two independent samples; the target and its normals under `pose`."""
    s, _ = faces(src_counts, seed, lo=SRC_MARGIN)
    t, n = faces(tgt_counts, seed + 1000)
    shift = np.asarray(shift, dtype=F64)
    src = (s + shift).astype(F32)
    tgt = C0.apply(pose, (t + shift).astype(F32)).astype(F32)
    return src, tgt, (n @ pose[:, :3].T).astype(F32)


def _empty():
    return np.zeros((0, 3), dtype=F32)


def _call(src, tgt, nrm, pose, max_dist, max_iter=30, kernel="l2", kernel_k=None, gt=GT):
    return dict(src=src, tgt=tgt, nrm=nrm, pose=np.asarray(pose, dtype=F64), max_dist=max_dist, max_iter=max_iter,
                kernel=kernel, kernel_k=kernel_k, gt=gt)


SNAP = R.compose(C0.rigid((3, -1, 2), 1.0, (0.05, -0.04, 0.03)), GT)
SLIDE = R.compose(C0.rigid((3, -1, 2), 3.0, (0.45, 0.2, -0.1)), GT)
ROBUST_K = 0.1


@functools.lru_cache(maxsize=None)
def case(name):
    src, tgt, nrm = corner()
    if name == "corner_snap":
        return _call([src], [tgt], [nrm], SNAP[None], 0.4)
    if name == "corner_slide":
        return _call([src], [tgt], [nrm], SLIDE[None], 0.75)
    if name == "ragged":
        p2 = C0.rigid((1, -1, 0.5), 10.0, (0.2, 0.1, -0.3))
        s2, t2, n2 = corner((90, 80, 87), (70, 110, 95), seed=21, pose=p2)
        one = np.array([[0.25, 0.5, 0.0]], dtype=F32)
        one_t = C0.apply(GT, one).astype(F32) + F32(0.05)
        one_n = (FACE_NORMALS[:1] @ GT[:, :3].T).astype(F32)
        return _call([src, one, s2, np.arange(15, dtype=F32).reshape(5, 3), _empty()],
                     [tgt, one_t, t2, _empty(), np.arange(21, dtype=F32).reshape(7, 3)],
                     [nrm, one_n, n2, _empty(), np.tile(np.array([[0, 0, 1]], dtype=F32), (7, 1))],
                     np.stack([SNAP, GT, R.compose(C0.rigid((0, 1, 0), 0.5, (0.02, -0.01, 0.01)), p2), GT, GT]), 0.4)
    if name == "plane":
        rng = np.random.default_rng(13)
        s = np.concatenate([rng.uniform(0, 2, (257, 2)), np.full((257, 1), 0.5)], 1).astype(F32)
        t = np.concatenate([rng.uniform(0, 2, (300, 2)), np.full((300, 1), 0.5)], 1).astype(F32)
        n = np.tile(np.array([[0, 0, 1]], dtype=F32), (300, 1))
        return _call([s], [t], [n], C0.rigid((0, 0, 1), 0.0, (0.01, 0.02, 0.05))[None], 0.4)
    if name == "zero_normals":
        z = nrm.copy()
        z[::5] = 0.0
        return _call([src], [tgt], [z], SNAP[None], 0.4)
    if name.startswith("robust_"):
        rng = np.random.default_rng(17)
        t, n = faces((100, 100, 100), 1007)            # the corner's own target sample, before the pose
        out = np.sort(rng.permutation(300)[:30])
        t = t.copy()
        t[out] += n[out] * rng.uniform(0.15, 0.3, (30, 1)) * rng.choice([-1.0, 1.0], (30, 1))
        kernel = name[len("robust_"):]
        return _call([src], [C0.apply(GT, t.astype(F32)).astype(F32)], [nrm], SNAP[None], 0.4, kernel=kernel,
                     kernel_k=None if kernel == "l2" else ROBUST_K)
    if name == "far":
        p = C0.rigid((0, 0, 1), 0.001, (0.05, -0.02, 0.03))
        s, t, n = corner(pose=p, shift=(1.0e4, 0.0, 0.0))
        return _call([s], [t], [n], C0.rigid((0, 0, 1), 0.0, (0, 0, 0))[None], 0.5, max_iter=10, gt=p)
    if name == "nonfinite":
        parts = [corner((20, 20, 20), (24, 23, 23), seed=31 + b) for b in range(3)]
        bad = parts[1][2].copy()
        bad[17, 1] = np.nan
        return _call([p[0] for p in parts], [p[1] for p in parts], [parts[0][2], bad, parts[2][2]],
                     np.stack([R.compose(C0.rigid((1, 0, 0), 0.5, (0.01, 0.01, 0.01)), GT)] * 3), 0.4)
    raise KeyError(name)


ROBUST = ("robust_l2", "robust_huber", "robust_tukey")
CASES = ("corner_snap", "corner_slide", "ragged", "plane", "zero_normals") + ROBUST + ("far", "nonfinite")
ITERATED = CASES                                   # every case's integers are pinned exactly on the GPU


@functools.lru_cache(maxsize=None)
def replica(name, perturb=0.0, max_iter=None):
    """The replica's result for every pair of the case's call (max_iter: the case's own unless given)."""
    c = case(name)
    it = c["max_iter"] if max_iter is None else max_iter
    return [P.icp(s, t, n, p, c["max_dist"], it, kernel=c["kernel"], kernel_k=c["kernel_k"], perturb=perturb)
            for s, t, n, p in zip(c["src"], c["tgt"], c["nrm"], c["pose"])]


@functools.lru_cache(maxsize=None)
def sensitivity(name):
    """(pose64, inlier_rmse): how far the replica's own outputs move, over the case's pairs, when every solved pose is
    perturbed by a relative 2^-40 -- the reference's spread that the GPU tolerances are derived from."""
    plain, moved = replica(name), replica(name, 2.0 ** -40)
    ok = [(p, m) for p, m in zip(plain, moved) if p["status"] == 0]
    return (max(float(np.abs(p["pose64"] - m["pose64"]).max()) for p, m in ok),
            max(abs(p["inlier_rmse"] - m["inlier_rmse"]) for p, m in ok))


def bounds(name):
    """The GPU tolerances of a case: 16 x the replica's sensitivity, every case but `far` capped at 1e-9."""
    pose, rmse = (16.0 * v for v in sensitivity(name))
    return (pose, rmse) if name == "far" else (min(pose, 1e-9), min(rmse, 1e-9))


def pose_error(T, gt=GT):
    return float(np.abs(np.asarray(T, dtype=F64) - gt).max())
