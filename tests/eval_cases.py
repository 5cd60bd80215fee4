"""The case table of the evaluation tests (tests/test_eval_host.py, tests/test_gpu_eval.py,
tests/test_gpu_eval_guarded.py): small batches of pairs around the two tile constants of csrc/evaluate.hip,
T = targets per LDS tile and Q = queries per workgroup, and the edge rules of the contract.  Every case is a dict
  src, ref: lists of [n,3] float32;  raw: such a list or None;  corr: (list, list) of [k,3] float32 or None;
  gt, pred: [B,3,4] float64;  radius: the acceptance radius (None without corr)
replica(name) is the contract's value per pair (tests/eval_replica.py), computed once and shared."""
import functools

import numpy as np

import eval_replica as R
from superpoints_registration_amd.evaluation import QUERIES as Q, TILE as T


def rigid(axis, angle_deg, t):
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = np.deg2rad(angle_deg)
    rot = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    return np.hstack([rot, np.asarray(t, dtype=np.float64)[:, None]])


def cloud(n, rng):
    return rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)


def poses(nb, rng):
    """gt: up to 45 degrees and 0.5; pred: 1 to 5 degrees and up to 0.05 away from it."""
    gt, pred = [], []
    for _ in range(nb):
        g = rigid(rng.normal(size=3), rng.uniform(5, 45), rng.uniform(-0.5, 0.5, 3))
        d = rigid(rng.normal(size=3), rng.uniform(1, 5), rng.uniform(-0.05, 0.05, 3) / np.sqrt(3))
        gt.append(g)
        pred.append(R.compose(d, g))
    return np.stack(gt), np.stack(pred)


def _sized(sizes, seed, corr_sizes=None, radius=None):
    """sizes: (n_src, n_ref, n_raw) per pair.  The source is the raw shape's points moved back by gt plus noise, the
    reference raw points plus noise: distances are small but not zero.  corr: source points against their images under
    gt plus noise of about the radius, so that some are inliers and some are not."""
    rng = np.random.default_rng(seed)
    gt, pred = poses(len(sizes), rng)
    src, ref, raw, cs, ct = [], [], [], [], []
    for b, (ns, nt, nr) in enumerate(sizes):
        shape = cloud(nr, rng)
        raw.append(shape)
        pick = (lambda n: shape[rng.integers(0, nr, n)].astype(np.float64)) if nr else (lambda n: rng.uniform(-1, 1, (n, 3)))
        ref.append((pick(nt) + rng.normal(0, 0.02, (nt, 3))).astype(np.float32))
        src.append((R.apply(R.inverse(gt[b]), pick(ns).astype(np.float32)) + rng.normal(0, 0.02, (ns, 3))).astype(np.float32))
        if corr_sizes is not None:
            k = corr_sizes[b]
            a = cloud(k, rng)
            cs.append(a)
            ct.append((R.apply(gt[b], a) + rng.normal(0, radius / 1.5, (k, 3))).astype(np.float32))
    return {"src": src, "ref": ref, "raw": raw, "corr": (cs, ct) if corr_sizes is not None else None, "gt": gt,
            "pred": pred, "radius": radius}


def _tiles():
    # target counts T-1, T, T+1, 2T+3; query counts Q-1, Q, Q+1 in both directions
    return _sized([(Q - 1, Q, T - 1), (Q, Q + 1, T), (Q + 1, Q - 1, T + 1), (Q, Q - 1, 2 * T + 3)], 11)


def _ones():
    return _sized([(1, 1, 1)], 12, corr_sizes=[1], radius=0.1)


def _ragged():
    # an empty source, an empty reference, one-point clouds, more than one block and tile
    return _sized([(0, 30, 40), (70, 1, 3), (Q + 44, 129, T + 88), (5, 0, 9), (64, 64, 64)], 13,
                  corr_sizes=[17, 0, 300, 1, 64], radius=0.1)


def _ties():
    """Every raw point twice: each minimum is attained at j and j + n, the lower one is the answer."""
    c = _sized([(40, 50, 30), (Q + 1, 20, T)], 14)
    c["raw"] = [np.concatenate([r, r]) for r in c["raw"]]
    return c


def _boundary():
    """gt = identity: correspondences at exactly the radius (no inlier: strict), inside it and outside it."""
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])[None]
    cs = np.zeros((4, 3), np.float32)
    ct = np.array([[0.5, 0, 0], [0, 0.25, 0], [0, 0, 0.75], [0.3, 0.4, 0]], np.float32)   # 0.3^2 + 0.4^2 != 0.25 in f32
    x = cloud(3, np.random.default_rng(15))
    return {"src": [x], "ref": [x], "raw": None, "corr": ([cs], [ct]), "gt": eye, "pred": eye.copy(), "radius": 0.5}


def _emptyraw():
    c = _sized([(20, 30, 40), (20, 30, 0), (0, 0, 0)], 16)
    return c


def _nonfinite():
    c = _sized([(20, 30, 40), (20, 30, 40), (33, 12, 70)], 17, corr_sizes=[5, 5, 5], radius=0.1)
    c["ref"][1][7, 2] = np.nan
    return c


def _same():
    """pair 0: identity poses and one cloud on all three sides: every column is 0; pair 1: pred == gt."""
    c = _sized([(50, 50, 50), (40, 30, 60)], 18)
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    c["src"][0] = c["ref"][0] = c["raw"][0]
    c["gt"][0] = c["pred"][0] = eye
    c["pred"][1] = c["gt"][1]
    return c


def _posesonly():
    c = _sized([(9, 7, 0), (3, 4, 0)], 19)
    c["raw"] = None
    return c


_BUILD = {"tiles": _tiles, "ones": _ones, "ragged": _ragged, "ties": _ties, "boundary": _boundary,
          "emptyraw": _emptyraw, "nonfinite": _nonfinite, "same": _same, "posesonly": _posesonly}
CASES = sorted(_BUILD)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILD[name]()


@functools.lru_cache(maxsize=None)
def replica(name):
    c = case(name)
    out = []
    for b in range(len(c["src"])):
        out.append(R.eval_pair(c["src"][b], c["ref"][b], c["gt"][b], c["pred"][b],
                               None if c["raw"] is None else c["raw"][b],
                               None if c["corr"] is None else (c["corr"][0][b], c["corr"][1][b]), c["radius"]))
    return out
