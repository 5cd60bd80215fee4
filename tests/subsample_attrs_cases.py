"""Seeded inputs of grid subsampling with features and labels, shared by test_subsample_attrs_host.py,
test_gpu_subsample_attrs.py, test_gpu_subsample_attrs_guarded.py and scripts/gen_subsample_attrs_golden.py.  Plain
numpy; only what the reference made of these inputs is stored (tests/golden/subsample_attrs.npz, cases of
REFERENCE_DEFINED in the reference's own row order).  Everything is built once per process and handed out read-only.

Every point sits well inside a cell of the dl grid (at least 0.2 dl from each face) and the grid offset is a multiple of
dl, so which voxel a point falls into is decided by construction, not by rounding; what the cases vary is how many
points share a voxel, in which order they arrive, and what they carry:

  sizes.*     clouds of 1, 2, 63, 64, 65 and 257 points, alone and three to a batch
  dims.*      fdim 0, 1, 3, 4, 7, 33 x ldim 0, 1, 3 on one 65-point cloud; dims.nb3.* the same widths in a batch of three
  own         every point in a voxel of its own
  one300      300 points in one voxel: features of mixed magnitude (1e8, 1, -1e8: the float32 sum depends on the
              order), labels from a palette of seven
  one300.distinct   300 points in one voxel with 300 distinct labels, all tied: the vote goes through every bucket
              count up to 541
  extremes    labels INT_MIN, INT_MAX, -1, negative and positive neighbours of the bucket counts, tied on purpose
  ties.k2 .. ties.k5   48 voxels each, k labels of equal count per voxel, label values of both signs
  distinct14, distinct30   a voxel with exactly 14 / 30 distinct labels, all tied (the second and third bucket counts),
              beside ordinary voxels
  max_p       a batch of three cut to 5 voxels per cloud (one cloud has fewer)
"""
import functools
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name pts lens dl max_p feat lab")    # feat: None or [N, fdim] f32; lab: None or [N, ldim] i32

DL, OFFSET = 0.05, -1.3
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
SIZES = (1, 2, 63, 64, 65, 257)
FDIMS = (0, 1, 3, 4, 7, 33)
LDIMS = (0, 1, 3)
PALETTE = np.array([3, -1, 0, 12, -14, 26, 13], np.int32)        # 26 = 0 mod 13, -14 and 12 share a bucket under 13


def _ro(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _cells(rng, m):
    """m distinct cells of a cube."""
    side = int(np.ceil((2.0 * m) ** (1.0 / 3.0))) + 1
    c = rng.permutation(side ** 3)[:m]
    return np.stack([c % side, (c // side) % side, c // (side * side)], 1)


def _place(rng, cells):
    return ((cells + 0.5 + rng.uniform(-0.3, 0.3, cells.shape)) * DL + OFFSET).astype(np.float32)


def _features(rng, n, fdim, wild=False):
    if fdim == 0:
        return None
    f = rng.normal(0.0, 1.0, (n, fdim)) * 10.0 ** rng.uniform(-3.0, 3.0, (n, fdim))
    if wild:
        f = np.where(rng.uniform(size=f.shape) < 0.4, rng.choice([1e8, -1e8, 3e7], f.shape), f)
    return f.astype(np.float32)


def _case(name, pts, lens, feat, lab, max_p=0):
    n = int(np.sum(lens))
    assert pts.shape == (n, 3) and (feat is None or feat.shape[0] == n) and (lab is None or lab.shape[0] == n)
    return Case(name, _ro(pts), tuple(int(v) for v in lens), DL, int(max_p), _ro(feat),
                _ro(None if lab is None else lab.astype(np.int32)))


def _random(name, seed, lens, fdim, ldim, per_voxel=3, max_p=0):
    """Every cloud: n points thrown at max(1, n // per_voxel) cells; labels from PALETTE (small voxels tie often)."""
    rng = np.random.default_rng(seed)
    pts = []
    for n in lens:
        cells = _cells(rng, max(1, n // per_voxel))
        pts.append(_place(rng, cells[rng.integers(0, len(cells), n)]))
    n = int(np.sum(lens))
    lab = PALETTE[rng.integers(0, len(PALETTE), (n, ldim))] if ldim else None
    return _case(name, np.concatenate(pts), lens, _features(rng, n, fdim), lab, max_p)


def _voxels(name, seed, votes, fdim=3, wild=False):
    """One cloud built from `votes`: per voxel an int array [k, ldim] of the label rows of its k points.  The points of
    all voxels are shuffled together, so arrival order inside a voxel is random too."""
    rng = np.random.default_rng(seed)
    cells = _cells(rng, len(votes))
    cell_of = np.concatenate([np.full(len(v), i) for i, v in enumerate(votes)])
    lab = np.concatenate([np.asarray(v, np.int64).reshape(len(v), -1) for v in votes])
    perm = rng.permutation(len(cell_of))
    pts = _place(rng, cells[cell_of[perm]])
    return _case(name, pts, [len(perm)], _features(rng, len(perm), fdim, wild), lab[perm])


def _tie_votes(rng, voxels, k, values):
    """Per voxel k distinct labels from `values`, each 1 to 3 times (the same count for all k)."""
    out = []
    for _ in range(voxels):
        labels = rng.choice(values, k, replace=False)
        out.append(np.repeat(labels, int(rng.integers(1, 4))))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case, in a fixed order."""
    out = [_random(f"sizes.nb1.n{n}", 100 + n, [n], 3, 1) for n in SIZES]
    out += [_random("sizes.nb3.a", 181, [65, 1, 257], 4, 1), _random("sizes.nb3.b", 182, [2, 63, 64], 4, 1)]
    out += [_random(f"dims.f{f}.l{l}", 200 + 10 * i + j, [65], f, l) for i, f in enumerate(FDIMS) for j, l in enumerate(LDIMS)]
    out += [_random(f"dims.nb3.f{f}.l{l}", 300 + i, [63, 2, 65], f, l) for i, (f, l) in enumerate(((33, 3), (7, 3), (4, 1)))]
    rng = np.random.default_rng(400)
    out.append(_voxels("own", 401, [PALETTE[rng.integers(0, 7, (1, 1))] for _ in range(100)]))
    out.append(_voxels("one300", 402, [PALETTE[rng.integers(0, 7, (300, 1))]], fdim=4, wild=True))
    out.append(_voxels("one300.distinct", 403, [rng.permutation(np.arange(-150, 150))[:, None] * 7], fdim=1))
    edge = np.array([INT_MIN, INT_MAX, -1, 0, 13, -13, 29, -29, INT_MIN + 1, INT_MAX - 1, 12, 28], np.int64)
    out.append(_voxels("extremes", 404, _tie_votes(rng, 60, 2, edge) + _tie_votes(rng, 60, 3, edge) + _tie_votes(rng, 40, 5, edge)))
    wide = np.concatenate([np.arange(-40, 41), [1000003, -1000003, 541, -541]]).astype(np.int64)
    out += [_voxels(f"ties.k{k}", 410 + k, _tie_votes(rng, 48, k, wide)) for k in (2, 3, 4, 5)]
    for m in (14, 30):
        # `m` distinct labels, all twice, beside 20 ordinary voxels; a second such voxel holds them once
        votes = [np.repeat(rng.choice(wide, m, replace=False), 2), rng.choice(wide, m, replace=False)]
        votes += [PALETTE[rng.integers(0, 7, int(rng.integers(1, 6)))] for _ in range(20)]
        out.append(_voxels(f"distinct{m}", 420 + m, votes))
    out.append(_random("max_p", 430, [65, 9, 257], 3, 1, per_voxel=4, max_p=5))
    return {c.name: c for c in out}


def fdim(c):
    return 0 if c.feat is None else c.feat.shape[1]


def ldim(c):
    return 0 if c.lab is None else c.lab.shape[1]


def reference_defined(c):
    """Where the reference's output is defined (grid_subsampling.cpp:157-158 slices the class vector wrongly for
    ldim > 1 in a batch of more than one cloud)."""
    return ldim(c) <= 1 or len(c.lens) == 1


NAMES = tuple(cases())
REFERENCE_DEFINED = tuple(n for n in NAMES if reference_defined(cases()[n]))
