"""GPU: grid subsampling and radius search on the edge inputs of preprocess_edge_cases.py -- a point below the grid
origin, voxel counts at the hash map's rehash boundaries, points on voxel faces, a heavy voxel, degenerate clouds,
max_p, the key capacity; neighbours at exactly the radius, queries outside the supports' box, far-off coordinates,
empty clouds inside a batch.  Everything is equality: uint32 views of the barycentres against the reference's recorded
output (tests/golden/preprocess_edges.npz) and the CPU oracle, neighbour rows against the float32 brute force."""
import functools

import numpy as np
import pytest
import torch

import preprocess_edge_cases as pe
from conftest import assert_rows_equal_up_to_ties, load_golden
from oracle import native
from superpoints_registration_amd import hip_shim, ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return load_golden("preprocess_edges.npz")


def _subsample(device, c, order, max_p=None):
    sub, lens = ops.grid_subsample(torch.tensor(c.pts).to(device), ops.lengths_to_cu(list(c.lens), device), c.dl,
                                   max_p=c.max_p if max_p is None else max_p, order=order)
    return sub.cpu().numpy(), lens.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _oracle(name, order):
    c = pe.sub_cases()[name]
    return native.grid_subsample(c.pts, c.lens, c.dl, max_p=c.max_p, order=order)


def _assert_same(got, want):
    assert np.array_equal(got[1], want[1]), (got[1].tolist(), want[1].tolist())
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


@pytest.mark.parametrize("name", pe.SUB_NAMES)
def test_reference_order_is_the_recorded_reference_output(gold, device, name):
    sub, lens = _subsample(device, pe.sub_cases()[name], ops.ORDER_REFERENCE)
    pe.assert_sub_matches_golden(gold, name, sub, lens)


@pytest.mark.parametrize("name", pe.SUB_NAMES)
def test_reference_order_is_the_oracle(device, name):
    _assert_same(_subsample(device, pe.sub_cases()[name], ops.ORDER_REFERENCE), _oracle(name, "reference"))


@pytest.mark.parametrize("name", pe.SUB_NAMES)
def test_canonical_order_is_the_oracle(device, name):
    _assert_same(_subsample(device, pe.sub_cases()[name], ops.ORDER_CANONICAL), _oracle(name, "canonical"))


@pytest.mark.parametrize("name", ["s2.batch"] + pe.S6_NAMES)
def test_shim_subsample_batch_with_max_p(gold, device, name):
    c = pe.sub_cases()[name]
    sub, lens = hip_shim.cpp_subsampling.subsample_batch(np.array(c.pts), np.asarray(c.lens, np.int32), sampleDl=c.dl,
                                                         max_p=c.max_p)
    pe.assert_sub_matches_golden(gold, name, sub, lens)


@pytest.mark.parametrize("order", [ops.ORDER_REFERENCE, ops.ORDER_CANONICAL])
def test_a_cloud_twice_in_a_batch_gives_the_single_result_twice(device, order):
    cases = pe.sub_cases()
    one, n1 = _subsample(device, cases["s5.single"], order)
    two, n2 = _subsample(device, cases["s5.twice"], order)
    m = int(n1[0])
    assert n2.tolist() == [m, m]
    assert np.array_equal(two[:m].view(np.uint32), one.view(np.uint32))
    assert np.array_equal(two[m:].view(np.uint32), one.view(np.uint32))
    # ... and the one-point cloud between two large ones is its own point
    mid, n3 = _subsample(device, cases["s5.one_between"], order)
    assert n3[1] == 1 and np.array_equal(mid[n3[0]], np.array([7.0, 7.0, 7.0], np.float32))


@pytest.mark.parametrize("case", pe.s7_cases(), ids=lambda c: c.name)
@pytest.mark.parametrize("order", [ops.ORDER_REFERENCE, ops.ORDER_CANONICAL])
def test_key_capacity_raises_and_the_next_call_is_right(gold, device, case, order):
    """A voxel key above 2^40: the documented RuntimeError (the reference returns two voxels here), through ops and
    through the shim; the next ordinary call on the same stream is untouched by it."""
    with pytest.raises(RuntimeError):
        _subsample(device, case, order)
    with pytest.raises(RuntimeError):
        hip_shim.cpp_subsampling.subsample_batch(np.array(case.pts), np.asarray(case.lens, np.int32), sampleDl=case.dl)
    for name in ("s1.control", "s1.dl0.05.min0.45.xyz.own"):
        sub, lens = _subsample(device, pe.sub_cases()[name], ops.ORDER_REFERENCE)
        pe.assert_sub_matches_golden(gold, name, sub, lens)


# ------------------------------------------------------------------------------------------------------------------
# radius search: every route against the float32 brute force
# ------------------------------------------------------------------------------------------------------------------
def _routes(q, qcu, s, scu, radius, limit):
    """(route, select, rows, max count) of every way to the same search."""
    for select in (ops.SELECT_NEAREST, ops.SELECT_INDEX):
        for algo in (0, 1):
            rows, mc = ops.radius_neighbors(q, s, qcu, scu, radius, limit, algo=algo, select=select)
            yield f"algo{algo}", select, rows, mc
        table = ops.RadiusTable(s, scu, radius)
        for dense in (False, True):
            rows, mc = table.query(q, qcu, limit, dense=dense, select=select)
            yield f"table.dense{int(dense)}", select, rows, mc


def _search(device, name, cross):
    c = pe.radius_case(name)
    s, scu = torch.tensor(c.sup).to(device), ops.lengths_to_cu(list(c.s_lens), device)
    if not cross:
        return c, s, scu, s, scu                       # the same tensors: the library's self search
    return c, torch.tensor(c.qry).to(device), ops.lengths_to_cu(list(c.q_lens), device), s, scu


@pytest.mark.parametrize("name,cross", [(n, True) for n in pe.RAD_NAMES] + [(n, False) for n in pe.RAD_SELF])
def test_every_route_gives_the_brute_force_rows(device, name, cross):
    c, q, qcu, s, scu = _search(device, name, cross)
    for limit in c.limits:
        near, index, mc = pe.expected_rows(name, cross, limit)
        for route, select, rows, got_mc in _routes(q, qcu, s, scu, c.radius, limit):
            want = index if select == ops.SELECT_INDEX else near
            assert got_mc == mc, (route, select, limit)
            assert np.array_equal(rows.cpu().numpy(), want), (route, select, limit)


def test_rows_of_a_cloud_without_supports_are_all_shadow(device):
    c, q, qcu, s, scu = _search(device, "r4.empty_s", True)
    ns = c.sup.shape[0]
    mid = slice(c.q_lens[0], c.q_lens[0] + c.q_lens[1])
    for route, select, rows, _ in _routes(q, qcu, s, scu, c.radius, 16):
        rows = rows.cpu().numpy()
        assert (rows[mid] == ns).all(), (route, select)
        assert (rows[:c.q_lens[0], 0] != ns).any() and (rows[mid.stop:, 0] != ns).any(), (route, select)


@pytest.mark.parametrize("name", pe.RAD_GOLDEN)
def test_rows_are_the_reference_rows_up_to_ties(gold, device, name):
    c = pe.radius_case(name)
    for key, q, ql, s, sl in pe.golden_searches(name):
        ref = gold[f"{key}.nb"].astype(np.int64)
        s_ext = np.concatenate([s, np.full((1, 3), 1e6, np.float32)])
        ds, scu = torch.tensor(s).to(device), ops.lengths_to_cu(list(sl), device)
        dq, qcu = (ds, scu) if key.endswith("self") else (torch.tensor(q).to(device), ops.lengths_to_cu(list(ql), device))
        for limit in c.limits:
            for route, select, rows, mc in _routes(dq, qcu, ds, scu, c.radius, limit):
                if select != ops.SELECT_NEAREST:
                    continue
                assert mc == ref.shape[1], route
                w = min(mc, limit)
                assert rows.shape == (len(q), w)
                assert_rows_equal_up_to_ties(ref[:, :w], rows.cpu().numpy(), q, s_ext, truncated=w < ref.shape[1])
