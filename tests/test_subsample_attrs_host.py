"""CPU: grid subsampling with features and labels -- the C ABI of the new entry points, the numpy restatement of the
contract (tests/subsample_attrs_replica.py) against the reference's own results (tests/golden/subsample_attrs.npz), and
that the cases of tests/subsample_attrs_cases.py tell a right implementation from the plausible wrong ones."""
import ctypes
import os
import re

import numpy as np
import pytest

import subsample_attrs_cases as sc
import subsample_attrs_replica as R
from conftest import load_golden
from superpoints_registration_amd import _lib
from test_workspace_sizes_host import HUGE, INT_MAX, sweep_points

NEW_SYMBOLS = ("spr_grid_subsample_attrs_workspace_size", "spr_grid_subsample_attrs")


@pytest.fixture(scope="module")
def gold():
    return load_golden("subsample_attrs.npz")


@pytest.fixture(scope="module")
def voxels(gold):
    """Every (case, output row, label column) of the fixture: (labels of the voxel in point order, reference's winner)."""
    out = []
    for name in sc.REFERENCE_DEFINED:
        c = sc.cases()[name]
        if c.lab is None:
            continue
        _, _, rows = R.voxel_rows(c.pts, c.lens, c.dl, c.max_p)
        for r, members in enumerate(rows):
            for col in range(c.lab.shape[1]):
                out.append((c.lab[members, col].tolist(), int(gold[f"{name}.lab"][r, col])))
    return out


# ---- C ABI -----------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spr.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["spr_grid_subsample_attrs"][1]) == 19
    from superpoints_registration_amd import subsample_attrs
    assert callable(subsample_attrs.grid_subsample)


def test_size_query_is_monotone_and_never_below_the_plain_query():
    L = _lib.lib()
    fn, base, limits = L.spr_grid_subsample_attrs_workspace_size, [1000, 3, 4, 2], [INT_MAX, (1 << 23) - 1, INT_MAX, INT_MAX]
    for i, limit in enumerate(limits):
        prev = None
        for v in sweep_points(limit):
            args = list(base)
            args[i] = v
            r = fn(*args)
            assert r < HUGE and (prev is None or r >= prev), (args, prev, r)
            prev = r
    for n in (1, 63, 1000, 100000):
        for nb in (1, 3, 64):
            plain = L.spr_grid_subsample_workspace_bytes(n, nb)
            assert fn(n, nb, 0, 0) >= plain
            assert fn(n, nb, 33, 0) == fn(n, nb, 0, 0)                    # nothing depends on fdim
            assert fn(n, nb, 0, 3) >= fn(n, nb, 0, 1) > fn(n, nb, 0, 0)   # takes are rounded up to 256 bytes
    for args in ([-5, 3, 4, 2], [1000, -5, 4, 2], [1000, 3, -5, 2], [1000, 3, 4, -5], [-5, -5, -5, -5]):
        assert fn(*args) <= fn(*base)


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    """Status 2 with NULL device pointers, on a machine without a GPU: nothing was dereferenced or launched."""
    L = _lib.lib()
    host = (ctypes.c_char * 64)()
    some = ctypes.cast(host, ctypes.c_void_p)       # a non-NULL pointer that a refused call never follows

    def call(fdim, ldim, feat=None, lab=None, out_feat=None, out_lab=None, ws=None, ws_bytes=0, n=4, nb=1, dl=0.1):
        return L.spr_grid_subsample_attrs(None, None, n, nb, dl, 0, 0, feat, fdim, lab, ldim, None, out_feat, out_lab, None,
                                          None, ws, ws_bytes, None)
    assert call(-1, 0) == 2 and b"negative" in L.spr_last_error()
    assert call(0, -3) == 2 and b"negative" in L.spr_last_error()
    assert call(3, 0) == 2 and b"features" in L.spr_last_error()
    assert call(3, 0, feat=some) == 2 and b"features" in L.spr_last_error()
    assert call(3, 0, out_feat=some) == 2 and b"features" in L.spr_last_error()
    assert call(0, 1) == 2 and b"labels" in L.spr_last_error()
    assert call(0, 1, lab=some) == 2 and b"labels" in L.spr_last_error()
    assert call(0, 0, n=0) == 2 and call(0, 0, nb=0) == 2 and call(0, 0, dl=0.0) == 2
    assert call(0, 0) == 2 and b"workspace" in L.spr_last_error()                       # the plain call, no workspace
    assert call(3, 1, some, some, some, some) == 2 and b"workspace" in L.spr_last_error()
    need = L.spr_grid_subsample_attrs_workspace_size(4, 1, 3, 1)
    assert call(3, 1, some, some, some, some, ws=some, ws_bytes=need - 1) == 2 and b"workspace" in L.spr_last_error()


# ---- the restatement against the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.REFERENCE_DEFINED)
def test_replica_matches_the_reference(gold, name):
    c = sc.cases()[name]
    sub, lens, feat, lab = R.grid_subsample(c.pts, c.lens, c.dl, c.max_p, "reference", c.feat, c.lab)
    assert np.array_equal(lens, gold[f"{name}.lens"])
    assert np.array_equal(sub.view(np.uint32), gold[f"{name}.pts"].view(np.uint32))
    assert (feat is None) == (f"{name}.feat" not in gold) and (lab is None) == (f"{name}.lab" not in gold)
    if feat is not None:
        assert np.array_equal(feat.view(np.uint32), gold[f"{name}.feat"].view(np.uint32))
    if lab is not None:
        assert np.array_equal(lab, gold[f"{name}.lab"])


def test_every_case_outside_the_reference_is_a_batch_with_label_columns():
    rest = [n for n in sc.NAMES if n not in sc.REFERENCE_DEFINED]
    assert rest and all(sc.ldim(sc.cases()[n]) > 1 and len(sc.cases()[n].lens) > 1 for n in rest)


def test_list_rule_on_hand_made_sequences():
    assert R.umap_order([5]) == [5] and R.umap_order([1, 2, 3]) == [3, 2, 1]             # empty buckets: to the front
    assert R.umap_order([1, 14, 2]) == [2, 14, 1]                                         # 14 joins 1's bucket, in front
    assert R.umap_order([-1, 2]) == [2, -1] and (-1 % (1 << 64)) % 13 == 2                # -1 hashes as 2^64 - 1
    assert R.umap_order([-1, 2, 3]) == [3, 2, -1]                                         # ... and shares 2's bucket
    assert R.vote([7, 7, 3])[0] == 7 and R.vote([3, 7])[0] == 7 and R.vote([1, 14, 14, 1, 2])[0] == 14
    keys = list(range(100, 114))
    assert R.umap_order(keys[:13]) == keys[12::-1]
    # the 14th key: 13 -> 29 buckets; the old list is re-inserted front to back, which reverses it once more
    assert R.umap_order(keys) == [113] + keys[:13]


# ---- the cases discriminate ------------------------------------------------------------------------------------------
def test_fixture_holds_enough_tied_votes(voxels):
    tied = [(labels, win) + R.vote(labels)[1:] for labels, win in voxels if len(R.vote(labels)[1]) > 1]
    assert len(tied) >= 20, len(tied)
    for k in (2, 3, 4, 5):
        assert any(len(t[2]) == k for t in tied), k
    neither = [t for t in tied if t[1] != min(t[2]) and t[1] != t[2][0]]
    assert len(neither) >= 5, len(neither)
    assert any(t[1] != max(t[2]) and t[1] != t[2][-1] for t in neither)       # nor the largest, nor the last arrived
    all_tied = [len(t[2]) for t in tied if len(t[2]) == t[3]]
    assert any(14 <= m < 30 for m in all_tied) and any(m >= 30 for m in all_tied), sorted(all_tied)[-5:]
    negative = [t for t in tied if min(t[2]) < 0]
    assert negative and any(sc.INT_MIN in t[2] for t in tied) and any(sc.INT_MAX in t[2] for t in tied)


def test_fixture_holds_a_feature_sum_that_depends_on_the_order(gold):
    c = sc.cases()["one300"]
    _, _, rows = R.voxel_rows(c.pts, c.lens, c.dl)
    assert len(rows) == 1 and len(rows[0]) == 300
    x = c.feat[rows[0]]
    in_order, tree = R.ordered_sum(x), R.tree_sum(x)
    assert (in_order.view(np.uint32) != tree.view(np.uint32)).any()
    assert np.array_equal((in_order / np.float32(300)).view(np.uint32), gold["one300.feat"][0].view(np.uint32))
    # ... and the division is not the barycentre's multiplication by a reciprocal in at least one stored feature
    differs = 0
    for name in sc.REFERENCE_DEFINED:
        c = sc.cases()[name]
        if c.feat is None:
            continue
        _, _, rows = R.voxel_rows(c.pts, c.lens, c.dl, c.max_p)
        for r, members in enumerate(rows):
            recip = R.ordered_sum(c.feat[members]) * np.float32(1.0 / len(members))
            differs += int((recip.view(np.uint32) != gold[f"{name}.feat"][r].view(np.uint32)).sum())
    assert differs > 0


def test_cases_cover_the_shapes_the_gpu_tests_promise():
    cs = sc.cases()
    assert {len(cs[f"sizes.nb1.n{n}"].pts) for n in sc.SIZES} == set(sc.SIZES)
    assert {(sc.fdim(c), sc.ldim(c)) for c in cs.values()} >= {(f, l) for f in sc.FDIMS for l in sc.LDIMS}
    assert {len(c.lens) for c in cs.values()} == {1, 3}
    own = R.voxel_rows(cs["own"].pts, cs["own"].lens, sc.DL)[2]
    assert len(own) == 100 and all(len(m) == 1 for m in own)
    cut = cs["max_p"]
    full = R.voxel_rows(cut.pts, cut.lens, sc.DL)[1]
    kept = R.voxel_rows(cut.pts, cut.lens, sc.DL, cut.max_p)[1]
    assert (kept < full).any() and (kept == full).any() and kept.max() == cut.max_p
