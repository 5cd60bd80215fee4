"""Inputs of the tie-order tests (tie_order='reference'), shared by test_tie_order_host.py, test_gpu_tie_order.py,
scripts/gen_tie_order_golden.py and scripts/tie_order_bench.py.  Plain numpy, seeded, built once per process and handed
out read-only.  Only what the reference made of them is stored (tests/golden/tie_order.npz).

Where exact ties are wanted the coordinates are multiples of 2^-5, so that every d2 is exact in float32 and equal
distances are equal bit for bit.  The smallest shapes at which each piece of the replay can go wrong:

  leaf boundary   n1 n2 n10 n11 n21   a root leaf, the first split (11 > leaf size 10), two levels
  degenerate      same40              40 identical points: every cut equals every point, split index = count / 2
                  line64              64 points that differ along x only
                  geom24              2^0 .. 2^23 on one axis, each value twice (so that rows tie and are replayed): the
                                      clamped cut peels points off, a deep, lopsided tree
  lattice         lat.r*              8 x 8 x 4 of step 2^-4, shuffled, and a copy translated by 64 (two clouds); the radii
                                      give rows of 7, 19, 27, 52 and 100 entries at most (the slab is 4 sites thin) in runs of 6 - 24 equal
                                      distances: rows below and above the sort's 16-element threshold
                  latdup.*            the same with every fourth point twice (d2 == 0 ties)
  cross           centres.*           queries = cell centres (every distance class has 8 members)
                  pool.*              a subset of the lattice as queries against the whole (a pool search)
                  up.*                the whole lattice as queries against the subset (an up-sampling search)
  batch           batch3              three clouds of 150, 1 and 77 points
  no ties         float600            600 random float points: nothing to fix
Every case is run at LIMITS = (5, 17, 40, 128): on the lattice rows the cut falls inside a run for at least one."""
import functools
import hashlib
import os
from collections import namedtuple

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tie_order.npz")
LIMITS = (5, 17, 40, 128)
STEP = 0.0625
Q = 0.03125                       # 2^-5

Case = namedtuple("Case", "name sup s_lens qry q_lens radius")


def _ro(a, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype=dtype)
    a.setflags(write=False)
    return a


def _self(name, sup, s_lens, radius):
    sup = _ro(sup)
    return Case(name, sup, tuple(s_lens), sup, tuple(s_lens), float(radius))


def _cross(name, sup, s_lens, qry, q_lens, radius):
    return Case(name, _ro(sup), tuple(s_lens), _ro(qry), tuple(q_lens), float(radius))


def _lattice(seed):
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    a = g[rng.permutation(len(g))] * STEP
    b = g[rng.permutation(len(g))] * STEP + 64.0
    return a.astype(np.float32), b.astype(np.float32)


# radius -> entries of an interior row: d2 / step^2 in {0, 1, 2, 3, 4, 5, 6, 8, 9} has 1, 6, 12, 8, 6, 24, 24, 12, 30 sites
LATTICE_RADII = {"r7": 0.07, "r19": 0.09, "r27": 0.11, "r57": 0.145, "r123": 0.19}


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    rng = np.random.default_rng(7001)
    for n in (1, 2, 10, 11, 21):
        out.append(_self(f"n{n}", rng.integers(0, 4, (n, 3)) * Q, [n], 0.25))
    out.append(_self("same40", np.tile(np.array([[0.5, -0.25, 2.0]]), (40, 1)), [40], 0.1))
    line = np.zeros((64, 3))
    line[:, 0] = rng.permutation(64) * Q
    line[:, 1:] = (0.75, -1.5)
    out.append(_self("line64", line, [64], 0.3))
    geom = np.zeros((48, 3))
    geom[:, 2] = 2.0 ** (rng.permutation(48) % 24)
    out.append(_self("geom24", geom, [48], 2000.0))     # (the table search takes at most 8191 cells per axis)
    a, b = _lattice(7002)
    lat = np.concatenate([a, b])
    for tag, r in LATTICE_RADII.items():
        out.append(_self(f"lat.{tag}", lat, [256, 256], r))
    dup = [np.concatenate([c, c[::4]])[rng.permutation(320)] for c in (a, b)]
    for tag in ("r7", "r27", "r57"):
        out.append(_self(f"latdup.{tag}", np.concatenate(dup), [320, 320], LATTICE_RADII[tag]))
    centres = [c[rng.permutation(256)[:90]] + np.float32(STEP / 2) for c in (a, b)]
    for tag, r in (("r19", 0.09), ("r57", 0.145)):
        out.append(_cross(f"centres.{tag}", lat, [256, 256], np.concatenate(centres), [90, 90], r))
    keep = [np.sort(rng.permutation(256)[:70]) for _ in range(2)]
    sub = [c[k] for c, k in zip((a, b), keep)]
    out.append(_cross("pool.r27", lat, [256, 256], np.concatenate(sub), [70, 70], 0.11))
    out.append(_cross("pool.r57", lat, [256, 256], np.concatenate(sub), [70, 70], 0.145))
    out.append(_cross("up.r57", np.concatenate(sub), [70, 70], lat, [256, 256], 0.145))
    out.append(_cross("up.r123", np.concatenate(sub), [70, 70], lat, [256, 256], 0.19))
    c0, c2 = a[:150], b[:77] - 64.0
    one = np.array([[0.25, 0.25, 0.125]], np.float32)
    out.append(_self("batch3", np.concatenate([c0, one, c2]), [150, 1, 77], 0.145))
    out.append(_self("float600", np.random.default_rng(7003).uniform(0.0, 1.0, (600, 3)), [600], 0.15))
    return {c.name: c for c in out}


NAMES = ["n1", "n2", "n10", "n11", "n21", "same40", "line64", "geom24"] + [f"lat.{t}" for t in LATTICE_RADII] + \
        ["latdup.r7", "latdup.r27", "latdup.r57", "centres.r19", "centres.r57", "pool.r27", "pool.r57", "up.r57",
         "up.r123", "batch3", "float600"]
TIED = [n for n in NAMES if n != "float600"]


# ---- randomised: 300 seeded clouds of 12 - 200 points, coordinates quantised to 2^-3 -----------------------------------------
N_RANDOM = 300
RANDOM_RADIUS = 0.3               # d2 / 2^-6 < 5.76: up to 57 entries, runs of up to 24


@functools.lru_cache(maxsize=None)
def random_case(k):
    rng = np.random.default_rng(9000 + k)
    n = int(rng.integers(12, 201))
    side = int(rng.integers(3, 9))
    sup = rng.integers(0, side, (n, 3)) * 0.125
    return _self(f"rand{k}", sup, [n], RANDOM_RADIUS), LIMITS[k % len(LIMITS)]


def digest(rows):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(rows, np.int32).tobytes()).digest(), np.uint8)


# ---- what the library's search returns for a case, computed on the host -------------------------------------------------
@functools.lru_cache(maxsize=None)
def index_rows(name, limit):
    """(rows [Nq, min(mc, limit)] in (d2, index) order, max count) of the float32 brute force the suite pins the
    table search to (oracle.native.radius_neighbors): the input of the fix-up."""
    from oracle import native
    c = cases()[name] if not name.startswith("rand") else random_case(int(name[4:]))[0]
    rows, mc = native.radius_neighbors(c.qry, c.sup, c.q_lens, c.s_lens, c.radius, limit=limit)
    return _ro(rows, np.int32), mc


def load_golden():
    """The stored rows of the reference; a missing file is an error (the tests that need it fail, they do not skip)."""
    if not os.path.exists(GOLDEN):
        raise FileNotFoundError(f"{GOLDEN} is missing: regenerate it with scripts/gen_tie_order_golden.py "
                                "(needs the compiled reference, oracle/_ref)")
    return dict(np.load(GOLDEN))


def reference_rows(gold, name, limit):
    """The reference's matrix of a case cut to `limit` columns (kpconv.py:259-260), from the golden (stored up to 128
    columns, the library's widest row)."""
    return gold[f"{name}.rows"][:, :limit]
