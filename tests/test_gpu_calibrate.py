"""GPU: the count-only walk of the cell table (spr_radius_table_count, ops.RadiusTable.count) and
calibrate_neighbors on top of it.  Everything is integer equality: counts and histograms against the full rows of
the CPU oracle, against the row-producing kernels on the same table, and against the committed golden
(tests/golden/calibrate.npz: the reference's procedure on six small pairs)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import calibrate_cases as cc
import preprocess_edge_cases as pe
from superpoints_registration_amd import _lib, get_config, kpconv, ops
from superpoints_registration_amd.calibration import calibrate_neighbors, coverage

pytestmark = pytest.mark.gpu


def _on_device(device, case):
    """(table, queries, q_cu): the table's own tensors as queries for a self search."""
    s, scu = torch.tensor(case.sup).to(device), ops.lengths_to_cu(list(case.s_lens), device)
    table = ops.RadiusTable(s, scu, case.radius)
    if case.qry is None:
        return table, table.supports, table.s_cu
    return table, torch.tensor(case.qry).to(device), ops.lengths_to_cu(list(case.q_lens), device)


@functools.lru_cache(maxsize=None)
def _expected(name):
    case = cc.count_cases()[name]
    counts = cc.expected_counts(case)
    counts.setflags(write=False)
    return counts


def _check(device, case, want, hist_n):
    table, q, qcu = _on_device(device, case)
    counts, hist = table.count(q, qcu, hist_n)
    assert counts.dtype == torch.int32 and hist.dtype == torch.int32
    assert np.array_equal(counts.cpu().numpy(), want)
    assert np.array_equal(hist.cpu().numpy(), cc.expected_hist(case, want, hist_n))
    assert table._slot == 0                                   # counting takes no result slot of the table


@pytest.mark.parametrize("name", sorted(cc.count_cases()))
def test_counts_and_histogram_are_the_oracles(device, name):
    case, want = cc.count_cases()[name], _expected(name)
    for hist_n in (905, 16):                                  # the shipped width, and one that many counts exceed
        _check(device, case, want, hist_n)


@functools.lru_cache(maxsize=None)
def _edge_case(name, cross):
    c = pe.radius_case(name)
    case = cc.CountCase(name, c.sup, c.s_lens, c.radius, c.qry if cross else None, c.q_lens if cross else None)
    return case, cc.expected_counts(case)


@pytest.mark.parametrize("name,cross", [(n, True) for n in pe.RAD_NAMES] + [(n, False) for n in pe.RAD_SELF])
def test_boundary_cases_of_the_radius_search(device, name, cross):
    """Supports at exactly d2 == r2 (out; in one float32 step later), queries outside the supports' box and below
    its minimum, far-off coordinates, clouds without queries or without supports."""
    case, want = _edge_case(name, cross)
    assert want.max() == pe.expected_rows(name, cross, pe.radius_case(name).limits[0])[2]
    _check(device, case, want, 64)


@pytest.mark.parametrize("name", ["s1.dl0.05.min0.45.xyz.own", "s1.dl0.05.min0.45.xyz.row", "s1.wide.z.own"])
def test_a_cloud_with_points_below_the_grid_origin(device, name):
    """The subsampling edge clouds as supports: the search's cells start at the cloud's true minimum."""
    c = pe.sub_cases()[name]
    case = cc.CountCase(name, c.pts, c.lens, 2.5 * c.dl, None, None)
    _check(device, case, cc.expected_counts(case), 905)


def test_histogram_rules(device):
    case = cc.clumps_case()
    want = cc.expected_counts(case)
    assert sorted(set(want.tolist())) == [2, 3, 7, 8, 12]
    table, q, qcu = _on_device(device, case)
    # hist_n 8: 7 is binned, 8 and 12 are not
    counts, hist = table.count(q, qcu, 8)
    assert np.array_equal(counts.cpu().numpy(), want)
    h = hist.cpu().numpy()
    assert h[0].tolist() == [0, 0, 0, 3, 0, 0, 0, 7] and h[1].tolist() == [0] * 8 and h[2].tolist() == [0, 0, 2] + [0] * 5
    assert np.array_equal(h, cc.expected_hist(case, want, 8))
    # added to what is there; the row of the empty cloud is not touched
    init = torch.arange(3 * 8, dtype=torch.int32, device=device).view(3, 8) + 5
    keep = init.clone()
    none, same = table.count(q, qcu, counts=False, hist=init)
    assert none is None and same is init
    assert np.array_equal(init.cpu().numpy(), keep.cpu().numpy() + h)
    assert np.array_equal(init[1].cpu().numpy(), keep[1].cpu().numpy())
    # counts alone
    counts, nohist = table.count(q, qcu)
    assert nohist is None and np.array_equal(counts.cpu().numpy(), want)
    # the widest histogram the library takes
    _, wide = table.count(q, qcu, 4096, counts=False)
    assert np.array_equal(wide.cpu().numpy(), cc.expected_hist(case, want, 4096))


@pytest.mark.parametrize("name", ["n513.self", "n513.sub", "ragged.self", "ragged.tail.sub", "twins.self", "copies.sub"])
@pytest.mark.parametrize("dense", [False, True])
def test_counts_agree_with_the_row_producing_kernels(device, name, dense):
    case = cc.count_cases()[name]
    table, q, qcu = _on_device(device, case)
    rows, mc = table.query(q, qcu, 128, dense=dense)
    counts, _ = table.count(q, qcu)
    assert mc <= 128, "case chosen so that no row is cut"
    assert np.array_equal((rows < case.sup.shape[0]).sum(1).cpu().numpy(), counts.cpu().numpy())
    assert int(counts.max()) == mc


def _raw_count(table, q, qcu, self_search, counts, hist, hist_n):
    st = torch.full((1,), 77, dtype=torch.int32, device=q.device)
    rc = _lib.lib().spr_radius_table_count(
        ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(qcu.data_ptr()), q.shape[0], self_search, table.ns, table.nb,
        table.radius, ctypes.c_void_p(table.blob.data_ptr()), ctypes.c_void_p(counts.data_ptr()),
        ctypes.c_void_p(hist.data_ptr()), hist_n, ctypes.c_void_p(st.data_ptr()),
        ctypes.c_void_p(torch.cuda.current_stream(q.device).cuda_stream))
    return rc, st


@pytest.mark.parametrize("far,code,words", [(1.0e4, -1, "8191 cells"), (200.0, -2, "voxelise or split")])
def test_a_table_in_error_raises_and_leaves_the_outputs(device, far, code, words):
    """Two points 10^4 apart at radius 1: more than 8191 cells per axis (-1).  200 apart on every axis: 8 M cells
    against a table of 64 * 2 + 2^20 (-2; there is no other route to a count)."""
    p = [[0.0, 0.0, 0.0], [far, 0.0, 0.0]] if code == -1 else [[0.0, 0.0, 0.0], [far, far, far]]
    s, scu = torch.tensor(p, dtype=torch.float32, device=device), ops.lengths_to_cu([2], device)
    table = ops.RadiusTable(s, scu, 1.0)
    counts = torch.full((2,), -7, dtype=torch.int32, device=device)
    hist = torch.full((1, 8), -9, dtype=torch.int32, device=device)
    rc, st = _raw_count(table, table.supports, table.s_cu, 1, counts, hist, 8)
    assert rc == 0 and int(st) == code
    assert (counts == -7).all() and (hist == -9).all()
    with pytest.raises(RuntimeError, match=words):
        table.count(table.supports, table.s_cu, 8)
    # the next ordinary call is untouched by it
    case = cc.count_cases()["n257.self"]
    t2, q, qcu = _on_device(device, case)
    assert np.array_equal(t2.count(q, qcu)[0].cpu().numpy(), _expected("n257.self"))


@pytest.mark.parametrize("hist_n", [0, 4097])
def test_histogram_widths_outside_the_range_are_refused_on_the_host(device, hist_n):
    case = cc.count_cases()["n255.self"]
    table, q, qcu = _on_device(device, case)
    counts = torch.full((255,), -7, dtype=torch.int32, device=device)
    hist = torch.full((1, 8), -9, dtype=torch.int32, device=device)
    rc, st = _raw_count(table, q, qcu, 1, counts, hist, hist_n)
    assert rc != 0 and b"hist_n must be in [1,4096]" in _lib.lib().spr_last_error()
    assert int(st) == 77 and (counts == -7).all() and (hist == -9).all()
    with pytest.raises(RuntimeError, match="hist_n"):
        table.count(q, qcu, hist_n)


# ------------------------------------------------------------------------------------------------------------------
# calibrate_neighbors
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    g = dict(np.load(cc.GOLDEN))
    g["items"] = [{"src_xyz": g[f"pair{k}.src_xyz"], "tgt_xyz": g[f"pair{k}.tgt_xyz"]} for k in range(cc.GOLDEN_PAIRS)]
    return g


@pytest.fixture(scope="module")
def calibrated(gold, device):
    """calibrate_neighbors on the golden's inputs with the default chunk, computed once."""
    return calibrate_neighbors(gold["items"], cc.golden_config(), keep_ratio=float(gold["keep_ratio"]),
                               samples_threshold=int(gold["samples_threshold"]), return_hists=True)


def test_calibration_reproduces_the_golden(gold, calibrated):
    limits, hists, used = calibrated
    assert hists.dtype == np.int64 and hists.shape == gold["hists"].shape
    assert np.array_equal(hists, gold["hists"])
    assert np.array_equal(limits, gold["limits"]) and np.issubdtype(limits.dtype, np.integer)
    assert used == int(gold["samples_used"]) == cc.GOLDEN_STOP
    cov = coverage(hists, limits)
    assert np.array_equal(cov, cc.coverage(gold["hists"], gold["limits"])) and (cov >= float(gold["keep_ratio"])).all()


@pytest.mark.parametrize("chunk", [1, 4])
def test_the_result_does_not_depend_on_the_chunk(gold, calibrated, device, chunk):
    """chunk 8 (the default, `calibrated`) computes all six pairs and uses four; chunk 4 stops at its chunk's end;
    chunk 1 never computes the fifth."""
    limits, hists, used = calibrate_neighbors(gold["items"], cc.golden_config(), keep_ratio=float(gold["keep_ratio"]),
                                              samples_threshold=int(gold["samples_threshold"]), chunk=chunk,
                                              return_hists=True)
    assert used == calibrated[2]
    assert np.array_equal(hists, calibrated[1]) and np.array_equal(limits, calibrated[0])


def test_a_short_dataset_uses_every_sample(gold, device):
    items = gold["items"][:3]
    limits, hists, used = calibrate_neighbors(items, cc.golden_config(), keep_ratio=float(gold["keep_ratio"]),
                                              samples_threshold=int(gold["samples_threshold"]), chunk=2,
                                              return_hists=True)
    assert used == 3
    assert np.array_equal(hists, gold["per_sample"][:3].sum(0))
    assert np.array_equal(limits, cc.percentiles(hists, float(gold["keep_ratio"])))
    # without return_hists: the limits alone
    alone = calibrate_neighbors(items, cc.golden_config(), keep_ratio=float(gold["keep_ratio"]),
                                samples_threshold=int(gold["samples_threshold"]))
    assert isinstance(alone, np.ndarray) and np.array_equal(alone, limits)


def test_device_tensors_and_a_config_without_limits_give_the_same(gold, calibrated, device):
    items = [{k: torch.from_numpy(v).to(device) for k, v in it.items()} for it in gold["items"]]
    cfg = get_config("3dmatch", neighborhood_limits=None)
    limits, hists, used = kpconv.calibrate_neighbors(items, cfg, keep_ratio=float(gold["keep_ratio"]),
                                                     samples_threshold=int(gold["samples_threshold"]),
                                                     return_hists=True)
    assert used == calibrated[2]
    assert np.array_equal(hists, calibrated[1]) and np.array_equal(limits, calibrated[0])


def test_calibrated_limits_through_the_preprocessor(gold, calibrated, device):
    """A level whose calibrated limit is below its largest neighbourhood gets rows of exactly that many columns; one
    whose limit is not gets rows as wide as its largest neighbourhood."""
    limits = calibrated[0]
    cfg = get_config("3dmatch", neighborhood_limits=list(limits))
    it = gold["items"][1]
    meta = kpconv.Preprocessor(cfg)([torch.from_numpy(it["src_xyz"]).to(device), torch.from_numpy(it["tgt_xyz"]).to(device)])
    _, levels, _ = kpconv.plan_pyramid(cfg)
    below = 0
    for l, lv in enumerate(levels):
        pts, cu = meta["points"][l], meta["_cu"][l]
        table = ops.RadiusTable(pts, cu, lv.radius)
        mc = int(table.count(table.supports, table.s_cu)[0].max())
        want = int(limits[l]) if limits[l] < mc else mc
        assert meta["neighbors"][l].shape == (pts.shape[0], want), l
        below += int(limits[l] < mc)
    assert below >= 1          # a limit at the 80th percentile cuts the widest rows of at least one level
