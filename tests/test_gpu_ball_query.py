"""GPU: the index selection rule of the neighbour search (select=ops.SELECT_INDEX, neighbor_select='index') -- the
neighbour rows of the reference's PreprocessorGPU (batch_neighbors_kpconv_gpu, kpconv.py:265-292 ->
pytorch3d.ops.ball_query): per query the K lowest support indices with d2 < r2, ascending, K columns, padded with the
shadow index.  Every route of the library (both algos of spr_radius_neighbors; the table's thread-per-query,
wave-per-query and default selections; self and cross searches) must give, entry for entry, the CPU oracle's full
in-range rows sorted by index and cut at K (ball_query_cases.py), and leave the default rule untouched."""
import functools

import numpy as np
import pytest
import torch

import ball_query_cases as bq
from oracle import torch_oracle
from superpoints_registration_amd import get_config, ops, synthetic
from superpoints_registration_amd.kpconv import Preprocessor
from superpoints_registration_amd.regtr import RegTR

pytestmark = pytest.mark.gpu

CASES = [(name, k) for name in ("ragged", "dense", "lattice", "cell_order", "cell_order_reversed", "overflow")
         for k in bq.CASE_LIMITS[name]]


def _cu(lens, device):
    return ops.lengths_to_cu([int(v) for v in lens], device)


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name,k", CASES, ids=[f"{n}-K{k}" for n, k in CASES])
@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
def test_every_route_gives_the_index_rows(device, name, k, cross):
    pts, lens, r, qs, ql = bq.case(name)
    want, near, mc = bq.expected(name, cross, k)
    s, s_cu = torch.tensor(pts, device=device), _cu(lens, device)
    q, q_cu = (torch.tensor(qs, device=device), _cu(ql, device)) if cross else (s, s_cu)
    nq = q.shape[0]

    def check(tag, got, m):
        assert tuple(got.shape) == (nq, k) and got.dtype == torch.int32, tag
        assert m == mc, f"{tag}: max_count {m} != {mc}"
        got = _np(got)
        bad = np.flatnonzero((got != want).any(1))
        assert bad.size == 0, f"{tag}: {bad.size} of {nq} rows differ, first {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"

    for algo in (0, 1):
        check(f"radius_neighbors algo {algo}", *ops.radius_neighbors(q, s, q_cu, s_cu, r, k, algo=algo,
                                                                     select=ops.SELECT_INDEX))
    table = ops.RadiusTable(s, s_cu, r)
    for dense in (False, True, None):
        check(f"table dense={dense}", *table.query(q, q_cu, k, dense=dense, select=ops.SELECT_INDEX))
    # one table answers both rules; the default rule is what it was
    for tag, (got, m) in (("radius_neighbors", ops.radius_neighbors(q, s, q_cu, s_cu, r, k)),
                          ("table", table.query(q, q_cu, k)),
                          ("table dense", table.query(q, q_cu, k, dense=True))):
        assert m == mc and np.array_equal(_np(got), near), f"default rule changed: {tag}"


def test_dense_input_really_is_dense():
    """Guards the generator: at K = 40 at least 5 % of the rows hold more than 2 K supports (scratch rows past
    their capacity, the histogram pass), and rows pass 128 (both wave-kernel instantiations are cut)."""
    cnt = bq.row_counts(bq.full_rows("dense", False)[0], 2000)
    assert (cnt > 80).mean() >= 0.05 and (cnt > 128).mean() >= 0.05


def test_no_neighbour_at_all_is_not_an_error_under_the_index_rule(device):
    """kpconv.py:284-292 has no emptiness check: K columns of shadows.  The default rule still raises."""
    pts, lens, r, _, _ = bq.case("ragged")
    s, s_cu = torch.tensor(pts, device=device), _cu(lens, device)
    far = torch.full((3, 3), 50.0, device=device)
    f_cu = _cu([1, 1, 1], device)
    for got, m in (ops.radius_neighbors(far, s, f_cu, s_cu, r, 8, select=ops.SELECT_INDEX),
                   ops.RadiusTable(s, s_cu, r).query(far, f_cu, 8, select=ops.SELECT_INDEX)):
        assert m == 0 and tuple(got.shape) == (3, 8) and bool((got == pts.shape[0]).all())
    with pytest.raises(RuntimeError):
        ops.radius_neighbors(far, s, f_cu, s_cu, r, 8)


# ---------------------------------------------------------------------------------------------------------------
# pyramid and encoder
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lidar():
    src, tgt, _ = synthetic.make_lidar_pair(n=10000, seed=0)
    return src, tgt


@functools.lru_cache(maxsize=None)
def _numpy_pyramid():
    return bq.ball_pyramid(get_config('kitti'), list(_lidar()))


def test_pyramid_under_the_index_rule(device):
    """Preprocessor(neighbor_select='index') on a LiDAR-shaped pair, KITTI config: every level's conv, pool and
    up-sampling matrix equals the numpy pyramid (native.grid_subsample + sorted-and-cut oracle rows); points and
    lengths are those of the default preprocessor.  Run twice: the second forward picks its routes from the first
    one's row counts (wave per query where rows were dense)."""
    cfg = get_config('kitti')
    ref = _numpy_pyramid()
    # the levels that feed the transformer are cut in most rows: the test is about rows the rules disagree on
    assert ref['over_limit'][2] > 0.5 and ref['over_limit'][3] > 0.5, ref['over_limit']
    clouds = [torch.tensor(c, device=device) for c in _lidar()]
    base = Preprocessor(cfg)(clouds)
    pre = Preprocessor(cfg, neighbor_select='index')
    n_levels = len(ref['points'])
    for rep in range(2):
        meta = pre(clouds)
        assert len(meta['points']) == n_levels
        for l in range(n_levels):
            assert torch.equal(meta['points'][l], base['points'][l])
            assert torch.equal(meta['stack_lengths'][l], base['stack_lengths'][l])
            assert np.array_equal(_np(meta['points'][l]).view(np.uint32), ref['points'][l].view(np.uint32))
            for key in ('neighbors', 'pools', 'upsamples'):
                got, want = _np(meta[key][l]), ref[key][l]
                assert got.dtype == np.int64
                assert got.shape == want.shape, f"rep {rep} level {l} {key}: {got.shape} != {want.shape}"
                assert np.array_equal(got, want), f"rep {rep} level {l} {key}"
        assert [pre._row_counts[(l, 'conv')] for l in range(n_levels)] == ref['max_count']
    differs = [not torch.equal(meta['neighbors'][l], base['neighbors'][l]) for l in range(n_levels)]
    assert differs[2] and differs[3]


def test_encoder_end_to_end_under_the_index_rule(device):
    """RegTR(neighbor_select='index'): the KPConv encoder's output against the float64 oracle encoder over the numpy
    pyramid, at the bar tests/test_gpu_backward.py holds encoder features to (2e-5 of the largest feature).  The
    default model's features differ from these by more than that bar: the switch reaches the kernels.

    The encoder's kernels do not depend on the order inside a row (sums, maxima), so the bound is the one of the
    default rule."""
    cfg = get_config('kitti', neighbor_select='index')
    clouds = [torch.tensor(c, device=device) for c in _lidar()]
    feats = {}
    for tag, c in (('index', cfg), ('nearest', get_config('kitti'))):
        model = RegTR(c)
        synthetic.fill_parameters(model, seed=0)
        model = model.to(device).eval()
        with torch.no_grad():
            meta = model.preprocessor(clouds)
            x0 = torch.ones((meta['points'][0].shape[0], 1), device=device)
            feats[tag] = model.kpf_encoder(x0, meta)[0].double().cpu()
        if tag == 'index':
            sd = {k: v.detach().double().cpu() for k, v in model.state_dict().items() if k.startswith('kpf_encoder.')}
    ref = _numpy_pyramid()
    meta64 = {'points': [torch.from_numpy(p).double() for p in ref['points']],
              'stack_lengths': [torch.from_numpy(np.asarray(l)) for l in ref['stack_lengths']],
              'neighbors': [torch.from_numpy(n) for n in ref['neighbors']],
              'pools': [torch.from_numpy(n) for n in ref['pools']]}
    with torch.no_grad():
        f64, _ = torch_oracle.encoder(cfg, sd, meta64)
    bar = 2e-5 * float(f64.abs().max())
    err = float((feats['index'] - f64).abs().max())
    moved = float((feats['index'] - feats['nearest']).abs().max())
    print(f"encoder under the index rule: max |err| {err:.3e}, bar {bar:.3e}, max |index - nearest| {moved:.3e}")
    assert feats['index'].shape == f64.shape
    assert err <= bar, f"{err:.3e} > {bar:.3e}"
    assert moved > bar, f"the two rules give the same features ({moved:.3e} <= {bar:.3e})"
