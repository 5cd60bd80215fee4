"""Edge inputs of the two index operators (grid subsampling, radius search), shared by test_preprocess_edges_host.py,
test_gpu_preprocess_edges.py and oracle/gen_golden.py (sub-command `preprocess_edges`).  Plain numpy, seeded; only
what the reference made of these inputs is stored (tests/golden/preprocess_edges.npz).  Everything is built once per
process and handed out read-only.

Subsampling cases (name -> SubCase):
  S1 below_origin  the grid origin floor(min * (1/dl)) * dl rounds to one ulp ABOVE the cloud's minimum: the minimum
                   point has cell index -1, which the reference casts to 2^64 - 1 (key arithmetic modulo 2^64)
  S2 rehash        exactly m occupied voxels, m on both sides of every bucket-count growth of the hash map
  S3 faces         coordinates on voxel faces and one float32 step to either side
  S4 heavy         5 000 points in one voxel: the barycentre depends on the sequential float32 summation order
  S5 degenerate    coincident points, flat and linear clouds, a one-point cloud between large ones, a cloud twice
  S6 max_p         the S2 batch, cut to the first max_p voxels of every cloud
  S7 capacity      a voxel key above 2^40 (the library's documented error)
Radius cases: see radius_case()."""
import functools
import hashlib
import os
from collections import namedtuple

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SubCase = namedtuple("SubCase", "name pts lens dl max_p")

FULL_ROWS = 2358          # clouds of up to this many voxels are stored whole, larger ones as slices + digest
EDGE_ROWS = 64            # rows kept from either end of a larger output


def _ro(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def _case(name, pts, lens, dl, max_p=0):
    pts = np.asarray(pts, np.float32)
    assert pts.shape == (int(np.sum(lens)), 3)
    return SubCase(name, _ro(pts), tuple(int(v) for v in lens), float(dl), int(max_p))


# ------------------------------------------------------------------------------------------------------------------
# S1: a point below the grid origin
# ------------------------------------------------------------------------------------------------------------------
def origin_of(mn, dl):
    """The reference's grid origin of a cloud minimum, in its float32 arithmetic (grid_subsampling.cpp:27)."""
    dl = np.float32(dl)
    inv = np.float32(1.0) / dl
    return np.floor(np.float32(mn) * inv) * dl


# (dl, a minimum whose origin lies above it)
S1_MINIMA = ((0.025, 0.225), (0.05, 0.45), (0.05, 65.45), (0.3, 3.3))
S1_AXES = ("x", "y", "z", "xyz")
S1_KINDS = ("row", "own")     # the stray point joins another row's last voxel / has a wrapped key of its own
S1_CONTROL_MIN = 0.40         # dl 0.05: origin == minimum, nothing lies below it
S1_WIDE = {"s1.wide.z.row": ("z", "row", (20, 20, 2), 4000), "s1.wide.z.own": ("z", "own", (20, 20, 2), 4000),
           "s1.wide.y.row": ("y", "row", (300, 4, 2), 6000), "s1.wide.y.own": ("y", "own", (300, 4, 2), 6000)}


def _s1_cloud(dl, m, axes, kind, seed, cells=(4, 4, 2), n=600):
    """n points in a box of 4 x 4 x 2 cells (every cell occupied) whose minimum along `axes` is exactly m; along
    the other axes the box starts 0.02 cells above a lattice plane (origin safely below the minimum).  The wide
    boxes (S1_WIDE) have nx > 256 or nx ny > 256: there an index of 2^32 - 1 instead of -1 on y or z -- what a GPU
    float -> unsigned conversion makes of -1.0f -- lifts the key above 2^40."""
    rng = np.random.default_rng(seed)
    dl32, m32 = np.float32(dl), np.float32(m)
    assert origin_of(m32, dl32) > m32
    safe = np.float32(np.float32(7.02) * dl32)
    assert origin_of(safe, dl32) < safe
    cells = np.array(cells)
    base = np.array([m32 if a in axes else safe for a in "xyz"], np.float32)
    c = np.stack([rng.permutation(np.arange(n) % cells[d]) for d in range(3)], 1)
    # strictly inside the cells: never on the minimum itself (only the stray points sit there), never on a face
    pts = (base.astype(np.float64) + (c + rng.uniform(0.05, 0.95, (n, 3))) * float(dl32)).astype(np.float32)
    assert tuple(cells) != (4, 4, 2) or len(np.unique(c @ np.array([1, 4, 16]))) == 32

    def at(ix, iy, iz):      # a point in cell (ix, iy, iz); -1 = exactly on the offending minimum
        idx = np.array([ix, iy, iz])
        p = (base.astype(np.float64) + (idx + rng.uniform(0.3, 0.7, 3)) * float(dl32)).astype(np.float32)
        return np.where(idx < 0, m32, p).astype(np.float32)

    if axes == "xyz":
        stray = [at(-1, -1, -1)] if kind == "own" else [at(-1, 2, 1), at(2, -1, 1), at(2, 2, -1), at(-1, -1, 1)]
    else:
        other = (2, 2, 1) if kind == "row" else (0, 0, 0)
        idx = [(-1 if a == axes else other[d]) for d, a in enumerate("xyz")]
        stray = [at(*idx)]
    pts = np.concatenate([pts, np.stack(stray)])
    return pts[rng.permutation(len(pts))]


def _s1_cases():
    out = []
    for k, (dl, m) in enumerate(S1_MINIMA):
        for a, axes in enumerate(S1_AXES):
            for j, kind in enumerate(S1_KINDS):
                name = f"s1.dl{dl}.min{m}.{axes}.{kind}"
                p = _s1_cloud(dl, m, axes, kind, 1000 + 100 * k + 10 * a + j)
                out.append(_case(name, p, [len(p)], dl))
    for j, (name, (axes, kind, cells, n)) in enumerate(S1_WIDE.items()):
        p = _s1_cloud(0.05, 0.45, axes, kind, 1900 + j, cells, n)
        out.append(_case(name, p, [len(p)], 0.05))
    rng = np.random.default_rng(1999)
    assert origin_of(S1_CONTROL_MIN, 0.05) == np.float32(S1_CONTROL_MIN)
    p = (np.float32(S1_CONTROL_MIN) + rng.uniform(0.0, 1.0, (600, 3)) * np.array([0.2, 0.2, 0.1])).astype(np.float32)
    p[0] = np.float32(S1_CONTROL_MIN)
    out.append(_case("s1.control", p, [600], 0.05))
    return out


# ------------------------------------------------------------------------------------------------------------------
# S2 / S6: voxel counts on both sides of every rehash
# ------------------------------------------------------------------------------------------------------------------
S2_PRIMES = (13, 29, 59, 127, 257, 541, 1109, 2357, 5087, 10273, 20753)     # libstdc++ bucket counts
S2_COUNTS = (1, 2) + tuple(v for p in S2_PRIMES for v in (p, p + 1))
S2_DL, S2_OFFSET = 0.05, -1.3
S6_MAX_P = (1, 12, 13, 14, 5000)


@functools.lru_cache(maxsize=None)
def s2_cloud(m):
    """A cloud with exactly m occupied voxels: m distinct cells of a cube, one point well inside each, plus m // 3
    further points in cells already taken; shuffled; translated by -1.3 (a multiple of dl)."""
    rng = np.random.default_rng(2000 + m)
    side = int(np.ceil((2.0 * m) ** (1.0 / 3.0))) + 1
    cells = rng.permutation(side ** 3)[:m]
    cells = np.concatenate([cells, cells[rng.integers(0, m, m // 3)]])
    c = np.stack([cells % side, (cells // side) % side, cells // (side * side)], 1)
    p = (c + 0.5 + rng.uniform(-0.3, 0.3, c.shape)) * S2_DL + S2_OFFSET
    return _ro(p[rng.permutation(len(p))].astype(np.float32))


def s2_batch(reverse=False, max_p=0):
    counts = S2_COUNTS[::-1] if reverse else S2_COUNTS
    clouds = [s2_cloud(m) for m in counts]
    name = "s2.batch" + (".reversed" if reverse else "") + (f".max_p{max_p}" if max_p else "")
    return _case(name, np.concatenate(clouds), [len(c) for c in clouds], S2_DL, max_p), counts


# ------------------------------------------------------------------------------------------------------------------
# S3: voxel faces
# ------------------------------------------------------------------------------------------------------------------
S3_OFFSETS = (0.0, -80.0, 100.0, 1000.0)
S3_DLS = (0.025, 0.05, 0.3)


def _s3_cases():
    out = []
    for i, off in enumerate(S3_OFFSETS):
        for j, dl in enumerate(S3_DLS):
            rng = np.random.default_rng(3000 + 10 * i + j)
            face = (off + np.arange(40) * dl).astype(np.float32)                       # float32(off + k dl)
            vals = np.concatenate([face, np.nextafter(face, np.float32(-np.inf)), np.nextafter(face, np.float32(np.inf))])
            p = np.stack([vals[rng.permutation(120)] for _ in range(3)], 1)
            out.append(_case(f"s3.off{off:g}.dl{dl}", p, [120], dl))
    return out


# ------------------------------------------------------------------------------------------------------------------
# S4, S5, S7
# ------------------------------------------------------------------------------------------------------------------
def _s4_cases():
    out = []
    for name, shift in (("s4.heavy", 0.0), ("s4.heavy_far", 100.0)):
        rng = np.random.default_rng(4000 + int(shift))
        heavy = (0.5 + 0.05 * 7 + rng.uniform(0.002, 0.048, (5000, 3)) + shift).astype(np.float32)
        spread = rng.uniform(0.0, 2.0, (300, 3)).astype(np.float32)
        p = np.concatenate([heavy, spread])
        out.append(_case(name, p[rng.permutation(len(p))], [len(p)], 0.05))
    return out


def _s5_cases():
    rng = np.random.default_rng(5000)
    out = [_case("s5.coincident", np.tile(np.array([[0.3, -1.7, 2.9]], np.float32), (50, 1)), [50], 0.05)]
    flat = rng.uniform(-0.5, 0.5, (300, 3)).astype(np.float32)
    flat[:, 2] = np.float32(0.123)
    out.append(_case("s5.flat", flat, [300], 0.05))
    line = flat.copy()
    line[:, 0] = np.float32(-0.77)
    out.append(_case("s5.line", line, [300], 0.05))
    a = rng.uniform(0.0, 1.0, (2000, 3)).astype(np.float32)
    b = rng.uniform(-3.0, -2.0, (2000, 3)).astype(np.float32)
    out.append(_case("s5.one_between", np.concatenate([a, np.array([[7.0, 7.0, 7.0]], np.float32), b]),
                     [2000, 1, 2000], 0.05))
    out.append(_case("s5.single", a, [2000], 0.05))
    out.append(_case("s5.twice", np.concatenate([a, a]), [2000, 2000], 0.05))
    return out


def s7_cases():
    """Two points 1e5 apart at dl 0.025: 4e6 cells per axis.  Apart in x and y the key is ix + nx iy ~ 8e12 > 2^40;
    apart along the space diagonal nx ny iz ~ 1.2e19 also passes 2^63."""
    d2, d3 = 1e5 / np.sqrt(2.0), 1e5 / np.sqrt(3.0)
    return [_case("s7.xy", np.array([[0.01, 0.01, 0.01], [d2, d2, 0.01]], np.float32), [2], 0.025),
            _case("s7.xyz", np.array([[0.01, 0.01, 0.01], [d3, d3, d3]], np.float32), [2], 0.025)]


@functools.lru_cache(maxsize=None)
def sub_cases():
    """name -> SubCase of every subsampling case that has a golden (S1 - S6), in a fixed order."""
    cases = _s1_cases()
    cases += [_case(f"s2.m{m}", s2_cloud(m), [len(s2_cloud(m))], S2_DL) for m in S2_COUNTS]
    cases += [s2_batch()[0], s2_batch(reverse=True)[0]]
    cases += _s3_cases() + _s4_cases() + _s5_cases()
    cases += [s2_batch(max_p=k)[0] for k in S6_MAX_P]
    return {c.name: c for c in cases}


def sub_names(prefix):
    return [n for n in sub_cases() if n.startswith(prefix)]


S1_NAMES = [f"s1.dl{dl}.min{m}.{axes}.{kind}" for dl, m in S1_MINIMA for axes in S1_AXES for kind in S1_KINDS]
S2_NAMES = [f"s2.m{m}" for m in S2_COUNTS] + ["s2.batch", "s2.batch.reversed"]
S3_NAMES = [f"s3.off{off:g}.dl{dl}" for off in S3_OFFSETS for dl in S3_DLS]
S4_NAMES = ["s4.heavy", "s4.heavy_far"]
S5_NAMES = ["s5.coincident", "s5.flat", "s5.line", "s5.one_between", "s5.single", "s5.twice"]
S6_NAMES = [f"s2.batch.max_p{k}" for k in S6_MAX_P]
SUB_NAMES = S1_NAMES + list(S1_WIDE) + ["s1.control"] + S2_NAMES + S3_NAMES + S4_NAMES + S5_NAMES + S6_NAMES


# ------------------------------------------------------------------------------------------------------------------
# golden records of a subsampling output: per cloud its length, a digest, and the rows (whole or both ends)
# ------------------------------------------------------------------------------------------------------------------
def digest(rows):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(rows, np.float32).tobytes()).digest(), np.uint8)


def pack_sub(name, sub, sub_lens):
    """The golden arrays of one case from the reference's output."""
    sub, sub_lens = np.asarray(sub, np.float32), np.asarray(sub_lens, np.int32)
    offs = np.concatenate([[0], np.cumsum(sub_lens)])
    rows, digs = [], []
    for c in range(len(sub_lens)):
        seg = sub[offs[c]:offs[c + 1]]
        digs.append(digest(seg))
        rows.append(seg if len(seg) <= FULL_ROWS else np.concatenate([seg[:EDGE_ROWS], seg[-EDGE_ROWS:]]))
    return {f"{name}.sub_lens": sub_lens, f"{name}.digest": np.stack(digs),
            f"{name}.rows": np.concatenate(rows).astype(np.float32)}


def assert_sub_matches_golden(gold, name, sub, sub_lens):
    """Equality of uint32 views with the stored rows, cloud by cloud, and of the SHA-256 of every cloud's bytes."""
    sub, sub_lens = np.asarray(sub, np.float32), np.asarray(sub_lens)
    want_lens = gold[f"{name}.sub_lens"]
    assert np.array_equal(sub_lens, want_lens), (name, sub_lens.tolist(), want_lens.tolist())
    assert sub.shape == (int(want_lens.sum()), 3)
    offs = np.concatenate([[0], np.cumsum(want_lens)])
    rows, r = gold[f"{name}.rows"], 0
    for c, m in enumerate(want_lens):
        seg = sub[offs[c]:offs[c + 1]]
        if m <= FULL_ROWS:
            want = rows[r:r + m]
            r += m
            assert np.array_equal(seg.view(np.uint32), want.view(np.uint32)), (name, c)
        else:
            want = rows[r:r + 2 * EDGE_ROWS]
            r += 2 * EDGE_ROWS
            assert np.array_equal(seg[:EDGE_ROWS].view(np.uint32), want[:EDGE_ROWS].view(np.uint32)), (name, c, "head")
            assert np.array_equal(seg[-EDGE_ROWS:].view(np.uint32), want[EDGE_ROWS:].view(np.uint32)), (name, c, "tail")
        assert np.array_equal(digest(seg), gold[f"{name}.digest"][c]), (name, c, "digest")
    assert r == len(rows)


# ------------------------------------------------------------------------------------------------------------------
# radius search
# ------------------------------------------------------------------------------------------------------------------
RadCase = namedtuple("RadCase", "name sup s_lens radius qry q_lens limits")
CELL_MARGIN = 1.0 + 1.0 / 256.0      # the search's cell edge is r * (1 + 2^-8)
R1_STEP = 0.0625
R1_RADII = {"r1.out": 0.125, "r1.in": float(np.nextafter(np.float32(0.125), np.float32(1.0)))}
R3_SHIFTS = (100.0, -100.0, 1000.0, -1000.0)


def _r1(name):
    """Exactly representable lattice 8 x 8 x 4 of step 2^-4, shuffled, and a copy translated by 64.  Neighbours at
    distance exactly 0.125 (two steps along an axis) have d2 == r2 bit for bit: out under the strict d2 < r2, in once
    the radius is one float32 step larger.  Queries: lattice sites and cell centres (multiples of 2^-5)."""
    rng = np.random.default_rng(6001)
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    a = (g[rng.permutation(len(g))] * R1_STEP).astype(np.float32)
    b = (g[rng.permutation(len(g))] * R1_STEP + 64.0).astype(np.float32)
    sup = np.concatenate([a, b])
    q = [np.concatenate([c[rng.permutation(256)[:60]],
                         c[rng.permutation(256)[:40]] + np.float32(R1_STEP / 2)]).astype(np.float32) for c in (a, b)]
    return RadCase(name, _ro(sup), (256, 256), R1_RADII[name], _ro(np.concatenate(q)), (100, 100), (8, 64))


def _r2():
    """Supports in [0, 1]^3 (both corners are supports), r = 0.1.  Queries beyond each of the six faces by 0.5 r,
    0.99 r, r, 1.5 r and 3, 4, 5, 6 cells (the cell coordinate clamps at -4 below the minimum; the table at dim - 1
    above the maximum), queries above the box on one axis and below it on another, and 120 inside."""
    rng = np.random.default_rng(6002)
    r = 0.1
    cell = r * CELL_MARGIN
    sup = rng.uniform(0.0, 1.0, (1500, 3))
    sup[0], sup[1] = 0.0, 1.0
    q = [rng.uniform(0.0, 1.0, (120, 3))]
    dists = [0.5 * r, 0.99 * r, r, 1.5 * r] + [k * cell for k in (3, 4, 5, 6)]
    for axis in range(3):
        for side in (0, 1):
            for d in dists:
                p = rng.uniform(0.0, 1.0, (4, 3))
                p[:, axis] = -d if side == 0 else 1.0 + d
                q.append(p)
    for up in range(3):
        for down in range(3):
            if up == down:
                continue
            for d in (0.5 * r, r, 4 * cell):
                p = rng.uniform(0.0, 1.0, (2, 3))
                p[:, up], p[:, down] = 1.0 + d, -d
                q.append(p)
    q = np.concatenate(q).astype(np.float32)
    return RadCase("r2", _ro(sup.astype(np.float32)), (1500,), r, _ro(q), (len(q),), (8, 64))


def _r3(name):
    """The `dense` cloud of preprocess.npz translated on all axes; the expectation is the brute force AT the
    translated coordinates (float32 spacing there is up to 6e-5: distances differ from the untranslated ones)."""
    g = np.load(os.path.join(GOLDEN, "preprocess.npz"))
    shift = np.float32(float(name.split("shift")[1]))
    pts = (g["dense.pts"] + shift).astype(np.float32)
    lens = tuple(int(v) for v in g["dense.lens"])
    rng = np.random.default_rng(6003)
    q = np.concatenate([pts[:500][rng.permutation(500)[:80]], pts[500:][rng.permutation(400)[:60]]])
    q = (q + rng.normal(0, 0.004, q.shape)).astype(np.float32)
    return RadCase(name, _ro(pts), lens, float(g["dense.radius"]), _ro(q), (80, 60), (40,))


def _r4(name):
    """Three clouds; `r4.empty_q`: the middle cloud has no queries; `r4.empty_s`: it has queries and no supports
    (their rows are all shadow)."""
    rng = np.random.default_rng(6004)
    s_lens = (300, 120, 200) if name == "r4.empty_q" else (300, 0, 200)
    q_lens = (200, 0, 150) if name == "r4.empty_q" else (200, 50, 150)
    sup = np.concatenate([rng.uniform(0, 1, (n, 3)) + 3.0 * i for i, n in enumerate(s_lens)]).astype(np.float32)
    qry = np.concatenate([rng.uniform(0, 1, (n, 3)) + 3.0 * i for i, n in enumerate(q_lens)]).astype(np.float32)
    return RadCase(name, _ro(sup), s_lens, 0.15, _ro(qry), q_lens, (16,))


RAD_NAMES = ["r1.out", "r1.in", "r2"] + [f"r3.shift{s:g}" for s in R3_SHIFTS] + ["r4.empty_q", "r4.empty_s"]
RAD_SELF = [n for n in RAD_NAMES if not n.startswith("r4")]      # cases whose self search is run too
RAD_GOLDEN = ["r1.out", "r1.in", "r2"]                           # cases with rows of the reference in the golden


@functools.lru_cache(maxsize=None)
def radius_case(name):
    if name.startswith("r1"):
        return _r1(name)
    if name == "r2":
        return _r2()
    if name.startswith("r3"):
        return _r3(name)
    if name.startswith("r4"):
        return _r4(name)
    raise KeyError(name)


def golden_searches(name):
    """The searches of a RAD_GOLDEN case whose reference rows are stored: (key, queries, q_lens, supports, s_lens).
    R1: the self search of the first cloud alone; R2: the outside queries against the supports."""
    c = radius_case(name)
    if name.startswith("r1"):
        a = c.sup[:256]
        return [(f"{name}.self", a, (256,), a, (256,))]
    return [(f"{name}.cross", c.qry, c.q_lens, c.sup, c.s_lens)]


@functools.lru_cache(maxsize=None)
def expected_rows(name, cross, limit):
    """(nearest rows [Nq, min(mc, limit)], index rows [Nq, limit], max count) of the float32 brute force the suite
    pins to the reference (oracle.native.radius_neighbors: (dx dx + dy dy) + dz dz, query - support, strict <,
    order (d2, index)); the index rule's rows are cut from its untruncated rows as in ball_query_cases."""
    from ball_query_cases import cut_by_index
    from oracle import native
    c = radius_case(name)
    q, ql = (c.qry, c.q_lens) if cross else (c.sup, c.s_lens)
    near, mc = native.radius_neighbors(q, c.sup, ql, c.s_lens, c.radius, limit=limit)
    full, mc2 = native.radius_neighbors(q, c.sup, ql, c.s_lens, c.radius, limit=0)
    assert mc == mc2
    return _ro(near), _ro(cut_by_index(full, c.sup.shape[0], limit)), mc
