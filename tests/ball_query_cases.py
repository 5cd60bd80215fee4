"""Inputs and expectations of the index selection rule of the neighbour search (SPR_SELECT_INDEX: the rows of the
reference's batch_neighbors_kpconv_gpu, kpconv.py:265-292 -> pytorch3d.ops.ball_query), shared by
test_ball_query_host.py and test_gpu_ball_query.py.

The expectation is derived from the CPU oracle the suite already pins against the reference: the FULL in-range row of
every query (native.radius_neighbors(limit=0): same float32 d2, same strict d2 < r2), sorted by index and cut or padded
to K columns.  Everything is computed once per process and handed out read-only."""
import functools

import numpy as np

from oracle import native

CELL_MARGIN = 1.0 + 1.0 / 256.0      # the search's cell edge is r * (1 + 2^-8)


def ball_rows(q, s, q_lens, s_lens, radius, k):
    """(int32 [Nq, k] rows, untruncated max count): per query the k lowest support indices in range, ascending,
    padded with the shadow index Ns."""
    full, mc = native.radius_neighbors(q, s, q_lens, s_lens, radius, limit=0)
    return cut_by_index(full, s.shape[0], k), mc


def cut_by_index(full, ns, k):
    """Rows of any width, shadow = ns -> sorted ascending (shadows sort last), cut or padded to k columns."""
    rows = np.sort(np.asarray(full, np.int64), axis=1)[:, :k]
    if rows.shape[1] < k:
        rows = np.concatenate([rows, np.full((rows.shape[0], k - rows.shape[1]), ns, np.int64)], 1)
    return np.ascontiguousarray(rows.astype(np.int32))


def row_counts(full, ns):
    return (np.asarray(full) != ns).sum(1)


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def _split_queries(rng, pts, lens, n_extra):
    """n_extra random queries inside the bounding box of every cloud, split over the clouds (every cloud gets one)."""
    nb = len(lens)
    ql = np.full(nb, 1, np.int64)
    ql += rng.multinomial(n_extra - nb, np.asarray(lens, np.float64) / np.sum(lens))
    offs = np.concatenate([[0], np.cumsum(lens)])
    out = []
    for c in range(nb):
        seg = pts[offs[c]:offs[c + 1]]
        lo, hi = seg.min(0), seg.max(0)
        out.append(rng.uniform(lo, np.maximum(hi, lo + 1e-3), (ql[c], 3)))
    return np.concatenate(out).astype(np.float32), [int(v) for v in ql]


def _cell_sorted(pts, lens, radius, reverse):
    """Every cloud ordered by the search's own cell key (z, y, x of floor((p - min) / cell)) -- the order in which
    the kernels meet the records -- or by its reverse."""
    offs = np.concatenate([[0], np.cumsum(lens)])
    out = []
    for c in range(len(lens)):
        seg = pts[offs[c]:offs[c + 1]]
        cell = np.floor((seg - seg.min(0)) / np.float32(radius * CELL_MARGIN)).astype(np.int64)
        order = np.lexsort((cell[:, 0], cell[:, 1], cell[:, 2]))
        out.append(seg[order[::-1] if reverse else order])
    return np.concatenate(out).astype(np.float32)


RAGGED_LENS = [700, 1, 333]
RAGGED_RADIUS = 0.215   # mean count ~ 20 over the three clouds


def _ragged():
    rng = np.random.default_rng(11)
    return rng.uniform(0.0, 1.0, (sum(RAGGED_LENS), 3)).astype(np.float32), rng


DENSE_RADIUS = 0.1
DENSE_SIDE = 0.32       # interior balls hold 2000 * (4/3) pi r^3 / side^3 ~ 256 supports, corner ones an eighth of that


@functools.lru_cache(maxsize=None)
def case(name):
    """(supports [N,3] f32, lengths, radius, extra queries [200,3] f32, their lengths) of input `name`."""
    if name in ("ragged", "cell_order", "cell_order_reversed"):
        pts, rng = _ragged()
        lens, r = RAGGED_LENS, RAGGED_RADIUS
        if name != "ragged":
            pts = _cell_sorted(pts, lens, r, reverse=name.endswith("reversed"))
    elif name == "dense":
        rng = np.random.default_rng(12)
        pts, lens, r = rng.uniform(0.0, DENSE_SIDE, (2000, 3)).astype(np.float32), [2000], DENSE_RADIUS
    elif name == "lattice":
        rng = np.random.default_rng(13)
        g = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
        g = g[rng.permutation(len(g))] * np.float32(0.25)
        pts, lens, r = np.concatenate([g, g]), [2 * len(g)], 0.5       # duplicate i of point i sits at i + 216
    elif name == "overflow":
        # two far-apart clusters in one cloud: the bounding box needs far more cells than the table holds
        rng = np.random.default_rng(0)
        a = rng.uniform(0, 0.05, (300, 3)).astype(np.float32)
        pts, lens, r = np.concatenate([a, a + np.float32(60.0)]), [600], 0.01
    else:
        raise KeyError(name)
    if name == "lattice":      # queries ON lattice sites and between them: d2 == r2 pairs exist for the former
        q = np.concatenate([pts[rng.integers(0, len(pts), 100)],
                            rng.uniform(0.0, 1.25, (100, 3)).astype(np.float32)]).astype(np.float32)
        ql = [200]
    elif name == "overflow":   # around both clusters (a box-uniform draw would hit neither)
        q = (pts[rng.integers(0, len(pts), 200)] + rng.normal(0, 0.004, (200, 3))).astype(np.float32)
        ql = [200]
    else:
        q, ql = _split_queries(rng, pts, lens, 200)
    return _frozen(pts, lens, r, q, ql)


CASE_LIMITS = {"ragged": (16, 40), "dense": (40, 74, 128), "lattice": (16, 40), "cell_order": (16, 40),
               "cell_order_reversed": (16, 40), "overflow": (8, 32)}


@functools.lru_cache(maxsize=None)
def full_rows(name, cross):
    """The oracle's untruncated rows (ascending (d2, index), shadow = Ns) and max count of a case's self or
    cross search."""
    pts, lens, r, q, ql = case(name)
    full, mc = native.radius_neighbors(q, pts, ql, lens, r, limit=0) if cross else \
        native.radius_neighbors(pts, pts, lens, lens, r, limit=0)
    return _frozen(full)[0], mc


@functools.lru_cache(maxsize=None)
def expected(name, cross, k):
    """(index-rule rows [Nq, k], nearest-rule rows [Nq, min(mc, k)], max count)."""
    pts, lens, r, q, ql = case(name)
    full, mc = full_rows(name, cross)
    near, mc_near = native.radius_neighbors(q, pts, ql, lens, r, limit=k) if cross else \
        native.radius_neighbors(pts, pts, lens, lens, r, limit=k)
    assert mc_near == mc
    return _frozen(cut_by_index(full, pts.shape[0], k), near) + (mc,)


# --------------------------------------------------------------------------------------------------------------
# the pyramid under the index rule, in numpy
# --------------------------------------------------------------------------------------------------------------
def plan_levels(cfg):
    from oracle import torch_oracle
    return torch_oracle.plan_levels(cfg)


def ball_pyramid(cfg, clouds):
    """torch_oracle.preprocess with every neighbour matrix replaced by its index-rule rows: same points and lengths
    (native.grid_subsample), conv / pool / up-sampling rows = ball_rows at the level's limit.  Also returns, per
    level, the share of conv rows with more than `limit` supports in range and the largest count."""
    pts = np.concatenate([np.asarray(c, np.float32) for c in clouds], 0)
    lens = np.asarray([len(c) for c in clouds], np.int32)
    r = cfg.first_subsampling_dl * cfg.conv_radius
    out = {k: [] for k in ('points', 'neighbors', 'pools', 'upsamples', 'stack_lengths', 'over_limit', 'max_count')}
    empty = np.zeros((0, 1), np.int64)
    for l, names in enumerate(plan_levels(cfg)):
        k = int(cfg.neighborhood_limits[l])
        down = 'pool' in names[-1] or 'strided' in names[-1]
        full, mc = native.radius_neighbors(pts, pts, lens, lens, r, limit=0)
        out['over_limit'].append(float((row_counts(full, pts.shape[0]) > k).mean()))
        out['max_count'].append(mc)
        has_conv = any(not ('pool' in n or 'strided' in n) for n in names)
        conv = cut_by_index(full, pts.shape[0], k).astype(np.int64) if has_conv else empty
        pool, up = empty, empty
        if down:
            dl = 2 * r / cfg.conv_radius
            sub, sub_lens = native.grid_subsample(pts, lens, dl)
            pool = ball_rows(sub, pts, sub_lens, lens, r, k)[0].astype(np.int64)
            up = ball_rows(pts, sub, lens, sub_lens, 2 * r, k)[0].astype(np.int64)
        out['points'].append(pts)
        out['neighbors'].append(conv)
        out['pools'].append(pool)
        out['upsamples'].append(up)
        out['stack_lengths'].append(lens)
        if down:
            pts, lens = sub, sub_lens
        r *= 2
    return out
