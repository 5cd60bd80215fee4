"""CPU: the host side of calibrate_neighbors -- the reference's percentile lines, its stop rule and the coverage
report against the numpy replica (calibrate_cases.py) on hand-made histograms; plan_pyramid without limits; the
argument checks of spr_radius_table_count, which run before any launch; and the committed golden
(tests/golden/calibrate.npz, scripts/gen_calibrate_golden.py): the replica over the CPU oracle reproduces the
recorded histograms and limits exactly."""
import ctypes

import numpy as np
import pytest

import calibrate_cases as cc
from superpoints_registration_amd import _lib, calibration, get_config, kpconv


def _hists(rows, hist_n=16):
    out = np.zeros((len(rows), hist_n), np.int64)
    for l, row in enumerate(rows):
        for k, v in row.items():
            out[l, k] = v
    return out


HAND_MADE = {
    "two_levels": _hists([{2: 5, 3: 10, 9: 4, 15: 1}, {0: 3, 1: 3, 2: 3, 8: 1}]),
    "all_zero_level": _hists([{4: 7, 5: 9}, {}, {1: 2}]),
    "one_bin": _hists([{7: 100}]),
    "last_bin": _hists([{15: 3, 0: 1}]),
}


@pytest.mark.parametrize("name", sorted(HAND_MADE))
@pytest.mark.parametrize("keep_ratio", [0.0, 0.5, 0.8, 1.0])
def test_percentile_lines_are_the_replicas(name, keep_ratio):
    h = HAND_MADE[name]
    got = calibration.limits_from_hists(h, keep_ratio)
    assert np.array_equal(got, cc.percentiles(h, keep_ratio))
    assert got.shape == (h.shape[0],)


def test_percentile_edge_values():
    h = HAND_MADE["all_zero_level"]
    # keep_ratio 0: nothing lies strictly below 0; keep_ratio 1: every count below the largest one in use
    assert calibration.limits_from_hists(h, 0.0).tolist() == [0, 0, 0]
    assert calibration.limits_from_hists(h, 1.0).tolist() == [5, 0, 1]
    # 0.8 of 16 = 12.8: cumsum is 7 at count 4, 16 at count 5 -> five counts (0..4) stay below
    assert calibration.limits_from_hists(h, 0.8).tolist() == [5, 0, 1]
    assert calibration.limits_from_hists(HAND_MADE["two_levels"], 0.8).tolist() == [9, 2]


def _sample(totals, hist_n=8):
    h = np.zeros((len(totals), hist_n), np.int64)
    h[:, 1] = totals
    return h


@pytest.mark.parametrize("per_sample,threshold,want", [
    ([_sample([5, 5]), _sample([5, 0]), _sample([5, 0])], 9, 3),          # level 1 never gets there: all samples
    ([_sample([5, 5]), _sample([5, 5]), _sample([5, 5])], 10, 3),         # reached exactly at the second: > is strict
    ([_sample([5, 5]), _sample([5, 5]), _sample([5, 5])], 9, 2),
    ([_sample([5, 0]), _sample([5, 0])], 0, 2),                           # an all-zero level never exceeds 0
    ([_sample([1, 1]), _sample([5, 5])], 0, 1),
], ids=["never", "exactly", "exceeded", "zero_level", "first"])
def test_stop_index_is_the_replicas(per_sample, threshold, want):
    assert cc.stop_index(per_sample, threshold) == want
    assert calibration.stop_index(per_sample, threshold) == want


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_coverage_is_the_replicas(name):
    h = HAND_MADE[name]
    for limits in ([0] * len(h), [4] * len(h), [15] * len(h), [200] * len(h), list(cc.percentiles(h, 0.8))):
        assert np.array_equal(calibration.coverage(h, limits), cc.coverage(h, limits), equal_nan=True), limits


def test_coverage_values():
    h = HAND_MADE["all_zero_level"]
    cov = calibration.coverage(h, [4, 3, 0])
    assert cov[0] == 7 / 16 and np.isnan(cov[1]) and cov[2] == 0.0
    # the calibrated limit keeps at least keep_ratio of the binned neighbourhoods whole
    for name, hh in HAND_MADE.items():
        cov = calibration.coverage(hh, calibration.limits_from_hists(hh, 0.8))
        assert np.all((cov >= 0.8) | np.isnan(cov)), name


@pytest.mark.parametrize("name", ["3dmatch", "kitti", "modelnet"])
def test_plan_pyramid_without_limits(name):
    cfg = get_config(name)
    blocks, levels, dim = kpconv.plan_pyramid(cfg)
    assert [lv.limit for lv in levels] == [int(v) for v in cfg.neighborhood_limits[:len(levels)]]
    missing = get_config(name)
    del missing["neighborhood_limits"]
    for other in (get_config(name, neighborhood_limits=None), missing):
        b2, l2, d2 = kpconv.plan_pyramid(other)
        assert b2 == blocks and d2 == dim
        assert [(lv.radius, lv.has_conv, lv.down) for lv in l2] == [(lv.radius, lv.has_conv, lv.down) for lv in levels]
        assert all(lv.limit is None for lv in l2)
    # the replica's own reading of the architecture agrees with the plan
    assert cc.level_plan(cfg) == [(lv.radius, lv.has_conv, lv.down) for lv in levels]


def test_public_names():
    assert kpconv.calibrate_neighbors is calibration.calibrate_neighbors
    assert calibration.hist_width(get_config("3dmatch")) == 905 == cc.hist_n_of(get_config("3dmatch"))
    with pytest.raises(NotImplementedError):
        calibration.calibrate_neighbors([], get_config("3dmatch"), collate_fn=lambda *a, **k: None)


def test_count_arguments_are_checked_on_the_host():
    """Bad arguments come back as an error code with spr_last_error set before anything is launched (no GPU here)."""
    L = _lib.lib()
    buf = (ctypes.c_int * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(nq=4, self_=0, ns=4, hist=p, hist_n=8, status=p, radius=1.0):
        return L.spr_radius_table_count(p, p, nq, self_, ns, 1, radius, p, p, hist, hist_n, status, None)

    for hist_n in (0, 4097, -1):
        assert call(hist_n=hist_n) != 0
        assert b"hist_n must be in [1,4096]" in L.spr_last_error()
    assert call(self_=1, nq=3) != 0 and b"self search" in L.spr_last_error()
    assert call(status=None) != 0 and b"radius_table_count" in L.spr_last_error()
    assert call(nq=0) != 0 and call(ns=0) != 0 and call(radius=0.0) != 0


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(cc.GOLDEN))


def test_golden_inputs_are_the_case_builders(gold):
    data = cc.golden_dataset()
    assert len(data) == cc.GOLDEN_PAIRS
    for k, it in enumerate(data):
        for key in ("src_xyz", "tgt_xyz"):
            assert np.array_equal(gold[f"pair{k}.{key}"].view(np.uint32), it[key].view(np.uint32)), (k, key)
    assert int(gold["hist_n"]) == cc.hist_n_of(cc.golden_config()) == gold["hists"].shape[1]


def test_replica_over_the_oracle_reproduces_the_golden(gold):
    per_sample = list(cc.golden_per_sample())
    assert np.array_equal(np.stack(per_sample), gold["per_sample"])
    limits, hists, used = cc.replica(None, cc.golden_config(), float(gold["keep_ratio"]),
                                     int(gold["samples_threshold"]), per_sample=per_sample)
    assert used == int(gold["samples_used"]) == cc.GOLDEN_STOP < cc.GOLDEN_PAIRS
    assert np.array_equal(hists, gold["hists"])
    assert np.array_equal(limits, gold["limits"])
    # the package's host parts on the recorded histograms
    assert calibration.stop_index(per_sample, int(gold["samples_threshold"])) == cc.GOLDEN_STOP
    assert np.array_equal(calibration.limits_from_hists(gold["hists"], float(gold["keep_ratio"])), gold["limits"])
