"""Host side of the index selection rule of the neighbour search (SPR_SELECT_INDEX / neighbor_select='index': the
rows of the reference's PreprocessorGPU): argument validation of both C entry points without a GPU, the config
switch, and the expectation helper of the GPU tests checked against itself."""
import ctypes

import numpy as np
import pytest

import ball_query_cases as bq
from oracle import native
from superpoints_registration_amd import _lib, get_config, ops
from superpoints_registration_amd.config import CONFIGS
from superpoints_registration_amd.kpconv import Preprocessor, PreprocessorGPU
from superpoints_registration_amd.regtr import RegTR


def _neighbors(select):
    L = _lib.lib()
    return L.spr_radius_neighbors(None, None, 0, None, None, 0, 0, 0.0, 0, 0, select, None, None, None, 0, None)


def _table_query(select):
    L = _lib.lib()
    return L.spr_radius_table_query(None, None, 0, 0, 0, 0, 0.0, 0, 0, None, None, None, 0, select, None, 0, None)


@pytest.mark.parametrize("call", [_neighbors, _table_query], ids=["radius_neighbors", "radius_table_query"])
@pytest.mark.parametrize("select", [-1, 2, 7])
def test_select_outside_the_two_rules_is_rejected_before_any_device_work(call, select):
    """Null pointers, no GPU: the check comes first, and the error text names the argument."""
    assert call(select) != 0
    msg = _lib.lib().spr_last_error().decode()
    assert "select" in msg and str(select) in msg


@pytest.mark.parametrize("call", [_neighbors, _table_query], ids=["radius_neighbors", "radius_table_query"])
@pytest.mark.parametrize("select", [ops.SELECT_NEAREST, ops.SELECT_INDEX])
def test_both_rules_pass_the_select_check(call, select):
    """The same null call with a valid rule fails on its OTHER arguments."""
    assert call(select) != 0
    assert "select" not in _lib.lib().spr_last_error().decode()


def test_python_constants_match_the_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spr.h")).read()
    for name, val in (("SPR_SELECT_NEAREST", ops.SELECT_NEAREST), ("SPR_SELECT_INDEX", ops.SELECT_INDEX)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", hdr).group(1)) == val
    assert int(re.search(r"#define\s+SPR_VERSION\s+(\d+)", hdr).group(1)) == 6


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_config_switch(name):
    assert get_config(name).neighbor_select == 'nearest'
    cfg = get_config(name, neighbor_select='index')
    assert cfg.neighbor_select == 'index'
    assert RegTR(cfg).preprocessor.neighbor_select == 'index'
    assert RegTR(get_config(name)).preprocessor.neighbor_select == 'nearest'
    with pytest.raises(NotImplementedError, match="neighbor_select"):
        RegTR(get_config(name, neighbor_select='first'))


def test_preprocessor_argument():
    cfg = get_config('kitti')
    assert Preprocessor(cfg).neighbor_select == 'nearest'
    assert PreprocessorGPU(cfg).neighbor_select == 'nearest'          # the name keeps the CPU semantics by default
    assert PreprocessorGPU(cfg, neighbor_select='index').neighbor_select == 'index'
    assert Preprocessor(get_config('kitti', neighbor_select='index')).neighbor_select == 'index'
    assert Preprocessor(get_config('kitti', neighbor_select='index'), neighbor_select='nearest').neighbor_select == 'nearest'
    with pytest.raises(ValueError, match="neighbor_select"):
        Preprocessor(cfg, neighbor_select='first')


@pytest.mark.parametrize("name", sorted(bq.CASE_LIMITS))
@pytest.mark.parametrize("cross", [False, True], ids=["self", "cross"])
def test_expectation_helper_against_itself(name, cross):
    """Rows with at most K supports in range hold the nearest rule's set; rows with more hold the K smallest
    indices of the full row; every row ascends and its shadows trail."""
    pts = bq.case(name)[0]
    ns = pts.shape[0]
    full, mc = bq.full_rows(name, cross)
    cnt = bq.row_counts(full, ns)
    assert mc == cnt.max()
    for k in bq.CASE_LIMITS[name]:
        rows, near, mc_k = bq.expected(name, cross, k)
        assert rows.shape == (full.shape[0], k) and rows.dtype == np.int32 and mc_k == mc
        assert np.all(rows[:, 1:] >= rows[:, :-1]) and rows.max() <= ns
        assert np.array_equal((rows != ns).sum(1), np.minimum(cnt, k))
        near_k = bq.cut_by_index(near, ns, k)                # the nearest rule's rows as sorted sets
        small = cnt <= k
        assert np.array_equal(rows[small], near_k[small])
        for i in np.flatnonzero(~small):
            assert np.array_equal(rows[i], np.sort(full[i][full[i] != ns])[:k])
        if (cnt > k).any():                                  # the two rules do keep different points
            assert (rows[~small] != near_k[~small]).any()


def test_inputs_have_the_properties_they_are_there_for():
    ns = bq.case("ragged")[0].shape[0]
    cnt = bq.row_counts(bq.full_rows("ragged", False)[0], ns)
    assert 18 <= cnt.mean() <= 22                            # K = 16 cuts most rows, K = 40 few
    assert (cnt > 16).mean() > 0.5 and 0 < (cnt > 40).mean() < 0.1
    cnt = bq.row_counts(bq.full_rows("dense", False)[0], 2000)
    assert (cnt > 80).mean() >= 0.05 and cnt.max() > 256     # rows past 2 K at every K, past the 128-entry scratch
    # lattice: pairs at d2 == r2 are out (strict), both copies of a site are in, in index order
    pts, lens, r, _, _ = bq.case("lattice")
    rows, _, _ = bq.expected("lattice", False, 40)
    n = len(pts) // 2
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
    assert (d2 == np.float32(r * r)).any()
    for i in (0, 5, n + 3):
        kept = rows[i][rows[i] != len(pts)]
        assert np.all(d2[i, kept] < np.float32(r * r))
        full_i = np.flatnonzero(d2[i] < np.float32(r * r))
        assert np.array_equal(kept, full_i[:40])
        assert all(((j + n) % (2 * n) in full_i) for j in full_i)
    # order traps: the same points as "ragged", met by the kernels in ascending and in descending index order
    a, b = bq.case("cell_order")[0], bq.case("cell_order_reversed")[0]
    assert np.array_equal(np.sort(a[:700], 0), np.sort(bq.case("ragged")[0][:700], 0))
    assert np.array_equal(a[:700], b[:700][::-1]) and np.array_equal(a[701:], b[701:][::-1])


def test_numpy_pyramid_matches_the_oracle_pyramid_where_the_rules_agree():
    """On a cloud sparse enough that no ball holds more than the limit, the index-rule pyramid is the oracle's
    nearest-rule pyramid with every row sorted by index."""
    from oracle import torch_oracle
    from superpoints_registration_amd import synthetic
    cfg = get_config('modelnet')
    src, tgt, _ = synthetic.make_sphere_pair(300, seed=1)
    ball = bq.ball_pyramid(cfg, [src, tgt])
    ref = torch_oracle.preprocess(cfg, [src, tgt])
    assert max(ball['over_limit']) == 0.0
    for l in range(len(ref['points'])):
        assert np.array_equal(ball['points'][l], ref['points'][l])
        assert np.array_equal(ball['stack_lengths'][l], ref['stack_lengths'][l])
        for key in ('neighbors', 'pools', 'upsamples'):
            a, b = ball[key][l], ref[key][l]
            if b.shape[0] == 0:
                assert a.shape[0] == 0
                continue
            ns = (ref['points'][l] if key != 'upsamples' else ref['points'][l + 1]).shape[0]
            k = int(cfg.neighborhood_limits[l])
            assert a.shape == (b.shape[0], k)
            assert np.array_equal(a, bq.cut_by_index(b, ns, k))
