"""Host: the CPU oracle (oracle/spr_oracle.c) on the edge inputs of preprocess_edge_cases.py against what the
reference's own C++ made of them (tests/golden/preprocess_edges.npz) -- in bits and in order, every case -- and
against oracle/_ref live where it is built.  The GPU tests (test_gpu_preprocess_edges.py) lean on both."""
import numpy as np
import pytest

import preprocess_edge_cases as pe
from conftest import assert_rows_equal_up_to_ties, load_golden
from oracle import native


@pytest.fixture(scope="module")
def gold():
    return load_golden("preprocess_edges.npz")


def test_case_list_is_the_golden_case_list(gold):
    assert list(pe.sub_cases()) == pe.SUB_NAMES
    assert {k.rsplit(".", 1)[0] for k in gold if k.endswith(".sub_lens")} == set(pe.SUB_NAMES)


@pytest.mark.parametrize("name", pe.SUB_NAMES)
def test_oracle_subsampling_is_the_golden(gold, name):
    c = pe.sub_cases()[name]
    sub, sub_lens = native.grid_subsample(c.pts, c.lens, c.dl, max_p=c.max_p)
    pe.assert_sub_matches_golden(gold, name, sub, sub_lens)


@pytest.mark.parametrize("name", pe.SUB_NAMES)
def test_oracle_subsampling_is_the_compiled_reference(name):
    if not native.ref_available():
        pytest.skip("oracle/_ref is not built here")
    c = pe.sub_cases()[name]
    sub, sub_lens = native.grid_subsample(c.pts, c.lens, c.dl, max_p=c.max_p)
    ref, ref_lens = native.ref_grid_subsample(c.pts, c.lens, c.dl, c.max_p)
    assert np.array_equal(sub_lens, ref_lens)
    assert np.array_equal(sub.view(np.uint32), ref.view(np.uint32))


def test_s1_constructions_put_a_point_below_the_origin(gold):
    """Every S1 cloud has a point whose cell index is -1 on the named axes (and the control cloud none); the `own`
    kind and every z case yield a key of the reference that wrapped modulo 2^64, the x / y `row` kinds none: their
    stray point joined a voxel of the neighbouring row, so the box's 32 cells stay 32 voxels."""
    for name in pe.S1_NAMES + list(pe.S1_WIDE) + ["s1.control"]:
        c = pe.sub_cases()[name]
        below = (c.pts.min(0) < pe.origin_of(c.pts.min(0), c.dl))
        _, lens, keys, _ = native.grid_subsample(c.pts, c.lens, c.dl, return_keys=True)
        wrapped = int((keys >= np.uint64(1) << np.uint64(63)).sum())
        if name == "s1.control":
            assert not below.any() and wrapped == 0 and lens.tolist() == [32]
            continue
        axes, kind = name.split(".")[-2:]
        assert below.tolist() == [a in axes for a in "xyz"], name
        joins = kind == "row" and axes in ("x", "y")
        assert (wrapped == 0) == joins, (name, wrapped)
        if name in pe.S1_NAMES:
            assert lens.tolist() == [32 + (0 if joins else 1)], (name, lens)


def test_rehash_clouds_have_exactly_m_voxels_and_the_batch_is_its_clouds(gold):
    for m in pe.S2_COUNTS:
        assert gold[f"s2.m{m}.sub_lens"].tolist() == [m]
    assert gold["s2.batch.sub_lens"].tolist() == list(pe.S2_COUNTS)
    assert sum(len(pe.s2_cloud(m)) for m in pe.S2_COUNTS) == 108289
    for name, counts in (("s2.batch", pe.S2_COUNTS), ("s2.batch.reversed", pe.S2_COUNTS[::-1])):
        assert np.array_equal(gold[f"{name}.digest"], np.stack([gold[f"s2.m{m}.digest"][0] for m in counts]))
    for k in pe.S6_MAX_P:                   # the first max_p voxels of the hash-map order, per cloud
        assert gold[f"s2.batch.max_p{k}.sub_lens"].tolist() == [min(m, k) for m in pe.S2_COUNTS]
    assert [int(gold[f"s2.batch.max_p{k}.sub_lens"].sum()) for k in pe.S6_MAX_P] == [24, 267, 289, 310, 38995]


def test_oracle_canonical_order_is_ascending_64_bit_key():
    """ORDER_CANONICAL of the oracle: the voxels of the reference order, sorted by the reference's 64-bit key --
    wrapped keys (2^64 - small) last."""
    for name in pe.S1_NAMES + pe.S3_NAMES:
        c = pe.sub_cases()[name]
        ref, _, keys, _ = native.grid_subsample(c.pts, c.lens, c.dl, return_keys=True)
        can, _, ckeys, _ = native.grid_subsample(c.pts, c.lens, c.dl, order="canonical", return_keys=True)
        order = np.argsort(keys, kind="stable")
        assert np.array_equal(ckeys, keys[order]) and len(np.unique(keys)) == len(keys)
        assert np.array_equal(can.view(np.uint32), ref[order].view(np.uint32))


def test_a_cloud_twice_in_a_batch_gives_the_single_result_twice(gold):
    one, two = gold["s5.single.rows"], gold["s5.twice.rows"]
    m = int(gold["s5.single.sub_lens"][0])
    assert gold["s5.twice.sub_lens"].tolist() == [m, m]
    assert np.array_equal(two[:m].view(np.uint32), one.view(np.uint32))
    assert np.array_equal(two[m:].view(np.uint32), one.view(np.uint32))


@pytest.mark.parametrize("name", pe.RAD_GOLDEN)
def test_oracle_rows_are_the_reference_rows_up_to_ties(gold, name):
    c = pe.radius_case(name)
    for key, q, ql, s, sl in pe.golden_searches(name):
        ref = gold[f"{key}.nb"].astype(np.int64)
        s_ext = np.concatenate([s, np.full((1, 3), 1e6, np.float32)])
        full, mc = native.radius_neighbors(q, s, ql, sl, c.radius, limit=0)
        assert mc == ref.shape[1]
        assert_rows_equal_up_to_ties(ref, full, q, s_ext, truncated=False)
        for limit in c.limits:
            got, mc = native.radius_neighbors(q, s, ql, sl, c.radius, limit=limit)
            w = min(mc, limit)
            assert_rows_equal_up_to_ties(ref[:, :w], got, q, s_ext, truncated=w < ref.shape[1])


def test_exact_radius_neighbours_are_out_and_one_step_further_in(gold):
    """R1: a lattice site two steps along an axis lies at d2 == r2 bit for bit."""
    out, inn = gold["r1.out.self.nb"].astype(np.int64), gold["r1.in.self.nb"].astype(np.int64)
    a = pe.radius_case("r1.out").sup[:256]
    assert np.array_equal(a, pe.radius_case("r1.in").sup[:256])
    d = np.linalg.norm(a[:, None, :].astype(np.float64) - a[None, :, :], axis=-1)
    assert np.array_equal((out != 256).sum(1), (d < 0.125).sum(1))
    assert np.array_equal((inn != 256).sum(1), (d <= 0.125).sum(1))
    assert ((d == 0.125).sum(1) >= 3).all()


def test_outside_queries_have_the_rows_the_distances_say(gold):
    """R2: beyond a face by r or more nothing is in range; by 0.5 r something usually is (so the set is no trivial
    all-shadow matrix), and the inside queries have neighbours."""
    c = pe.radius_case("r2")
    ref = gold["r2.cross.nb"].astype(np.int64)
    cnt = (ref != c.sup.shape[0]).sum(1)
    gap = np.maximum(np.maximum(-c.qry, c.qry - 1.0), 0.0)
    dist = np.sqrt((gap.astype(np.float64) ** 2).sum(1))          # distance to the box
    assert (cnt[dist >= c.radius] == 0).all()
    assert (cnt[:120] > 0).all() and (cnt[(dist > 0) & (dist < 0.06)] > 0).any()
    assert (dist >= 3 * c.radius).sum() >= 6 * 4 * 4
