"""CPU: the RANSAC contract without a GPU -- the library's host draws (spr_ransac_draw) against the numpy replica
(tests/ransac_replica.py), the replica against the reference's own ransac() (tests/golden/ransac_ops.npz,
scripts/gen_ransac_golden.py), the C ABI and the host-side argument checks of ops.ransac_pairs."""
import ctypes

import numpy as np
import pytest
import torch

import ransac_replica
from conftest import load_golden
from superpoints_registration_amd import _lib, ops

SEEDS = (0, 1, 0x123456789ABCDEF0, 2 ** 64 - 1)
KEYS = (0, 1, 7, 2 ** 31, 2 ** 31 + 5, 2 ** 40 + 3, 2 ** 63 - 1)


def test_library_exports_the_ransac_symbols():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("spr_ransac_pairs", "spr_ransac_draw"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert (ops.RANSAC_EMPTY, ops.RANSAC_BAD_INDEX, ops.RANSAC_BAD_LAYOUT) == (1, 2, 4)
    L = _lib.lib()
    # host-side refusals, before any HIP call
    rc = L.spr_ransac_pairs(None, None, None, None, 1, 0, 100, 0, None, None, None, None, None, None, None, None)
    assert rc != 0 and b"ransac_pairs" in L.spr_last_error()
    rc = L.spr_ransac_pairs(None, None, None, None, 1, 500, 100, 0, None, None, None, None, None, None, None, None)
    assert rc != 0 and b"null" in L.spr_last_error()
    # n_hyp * ceil(sample / 4) must fit the 32-bit block counter
    out = np.zeros(4, dtype=np.int32)
    key, n = np.zeros(1, dtype=np.uint64), np.ones(1, dtype=np.int32)
    rc = L.spr_ransac_draw(0, key.ctypes.data, n.ctypes.data, 1, 2 ** 30, 16, out.ctypes.data)
    assert rc != 0 and b"block counter" in L.spr_last_error()


@pytest.mark.parametrize("sample", [1, 3, 4, 5, 100])
def test_host_draws_equal_the_replica(sample):
    n_hyp = 7
    ns = [1, 2, 37, 2 ** 31 - 1]
    for seed in SEEDS:
        for key in KEYS:
            got = ops.ransac_draw(seed, [key] * len(ns), ns, n_hyp, sample)
            assert got.shape == (len(ns), n_hyp, sample) and got.dtype == np.int32
            for j, n in enumerate(ns):
                assert got[j].min() >= 0 and got[j].max() < n
                assert np.array_equal(got[j], ransac_replica.draw(seed, key, n, n_hyp, sample)), (seed, key, n)
    # the draws are not degenerate: a large n sees many distinct indices, keys and seeds decorrelate
    a = ops.ransac_draw(0, [0, 1], [2 ** 31 - 1] * 2, n_hyp, sample)
    assert len(np.unique(a)) == a.size
    assert not np.array_equal(ops.ransac_draw(1, [0], [37], 50, sample), ops.ransac_draw(0, [0], [37], 50, sample))


def test_draws_depend_on_the_pair_alone():
    """(seed, pair_key, n, n_hyp, sample) only: the same pair draws the same indices at any place of any batch; a
    hypothesis's blocks do not overlap its neighbour's."""
    one = ops.ransac_draw(5, [2 ** 31 + 5], [37], 9, 5)
    many = ops.ransac_draw(5, [3, 2 ** 31 + 5, 4], [64, 37, 2], 9, 5)
    assert np.array_equal(one[0], many[1])
    # sample = 5 uses two blocks per hypothesis: hypothesis h starts at block 2 h
    w = ransac_replica.draw(5, 3, 2 ** 31 - 1, 18, 4)          # one block per row
    s5 = ransac_replica.draw(5, 3, 2 ** 31 - 1, 9, 5)
    assert np.array_equal(s5[:, :4], w[0::2]) and np.array_equal(s5[:, 4], w[1::2, 0])


def test_ransac_draw_refuses_bad_arguments():
    with pytest.raises(ValueError, match="at least 1"):
        ops.ransac_draw(0, [0], [5], 0, 4)
    with pytest.raises(ValueError, match="at least 1"):
        ops.ransac_draw(0, [0], [5], 4, 0)
    with pytest.raises(ValueError, match="pair keys"):
        ops.ransac_draw(0, [2 ** 63], [5], 4, 4)
    with pytest.raises(ValueError, match="pair keys"):
        ops.ransac_draw(0, [0, 1], [5], 4, 4)
    with pytest.raises(ValueError, match="block counter"):
        ops.ransac_draw(0, [0], [5], 2 ** 30, 16)


def test_replica_reproduces_the_reference():
    """On the recorded draws the float64 replica reproduces the reference's float32 losses within 1e-5 relative, its
    pick exactly and the gaps the generator stored."""
    g = load_golden("ransac_ops.npz")
    assert int(g["B"]) == 3 and int(g["n_hyp"]) == 500 and int(g["sample"]) == 100
    for b, n in enumerate((37, 64, 130)):
        idx = g[f"idx{b}"].astype(np.int64)
        assert g[f"src{b}"].shape == (n, 3) and idx.shape == (500, 100) and idx.max() < n
        rep = ransac_replica.ransac_pair(g[f"src{b}"], g[f"tgt{b}"], g[f"w{b}"], idx)
        loss = g[f"loss{b}"].astype(np.float64)
        rel = np.abs(rep["score"] - loss) / loss
        print(f"n = {n}: replica vs reference loss, max relative {rel.max():.2e}")
        assert rel.max() <= 1e-5
        assert rep["best"] == int(g[f"best{b}"]) == ransac_replica.pick(g[f"loss{b}"])
        assert np.array_equal(g[f"pose{b}"], g[f"hyp_pose{b}"][int(g[f"best{b}"])])
        gap = ransac_replica.gap(rep["score"])[1]
        frac = ransac_replica.well_posed(rep["sv"]).mean()
        assert gap == pytest.approx(float(g["gap"][b]), rel=1e-9) and gap >= 1e-4
        assert frac == pytest.approx(float(g["well_posed_frac"][b])) and frac >= 0.9
        # the planted transform is found: the inputs are a registration problem, not noise
        assert np.linalg.norm(rep["pose"] - g[f"planted{b}"]) < 0.1


def test_pick_rule():
    nan = float("nan")
    assert ransac_replica.pick(np.array([3.0, 1.0, 1.0, 2.0])) == 1          # the first minimum
    assert ransac_replica.pick(np.array([1.0, nan, 0.5, nan])) == 2          # a NaN never wins
    assert ransac_replica.pick(np.array([nan, 0.5, 0.1])) == 0               # nothing compares below a NaN
    assert ransac_replica.pick(np.array([np.inf, np.inf])) == 0


def test_ransac_pairs_rejects_bad_arguments_without_a_gpu():
    n = [5, 7]
    T = sum(n)
    a, b, w = torch.rand(T, 3), torch.rand(T, 3), torch.rand(T)
    cu_h = [0, 5, 12]
    cu = torch.tensor(cu_h, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ransac_pairs(a, b, w, cu, cu_h)
    with pytest.raises(ValueError, match="at least 1"):
        ops.ransac_pairs(a, b, w, cu, cu_h, n_hyp=0)
    with pytest.raises(ValueError, match="at least 1"):
        ops.ransac_pairs(a, b, w, cu, cu_h, sample=0)
    with pytest.raises(ValueError, match="block counter"):
        ops.ransac_pairs(a, b, w, cu, cu_h, n_hyp=2 ** 30, sample=16)
    with pytest.raises(ValueError, match="set_cu_host"):
        ops.ransac_pairs(a, b, w, cu, [0, 7, 5])                                   # not ascending
    with pytest.raises(ValueError, match="set_cu_host"):
        ops.ransac_pairs(a, b, w, cu, [1, 5, 12])                                  # not from 0
    with pytest.raises(ValueError, match="set_cu_host"):
        ops.ransac_pairs(a, b, w, cu, [0])                                         # no pair
    with pytest.raises(ValueError, match="shapes"):
        ops.ransac_pairs(a, b, w, cu, [0, 5, 11])                                  # another total
    with pytest.raises(ValueError, match="shapes"):
        ops.ransac_pairs(a, b, w, cu, [0, 5, 8, 12])                               # another pair count
    with pytest.raises(ValueError, match="shapes"):
        ops.ransac_pairs(a, b[:-1], w, cu, cu_h)
    with pytest.raises(ValueError, match="shapes"):
        ops.ransac_pairs(a, b, torch.rand(T, 2), cu, cu_h)
    with pytest.raises(ValueError, match="shapes"):
        ops.ransac_pairs(a[:, :2], b, w, cu, cu_h)
    with pytest.raises(ValueError, match="pair keys"):
        ops.ransac_pairs(a, b, w, cu, cu_h, pair_keys=[0, 2 ** 63])
    with pytest.raises(ValueError, match="pair keys"):
        ops.ransac_pairs(a, b, w, cu, cu_h, pair_keys=[0, -1])
    with pytest.raises(ValueError, match="pair keys"):
        ops.ransac_pairs(a, b, w, cu, cu_h, pair_keys=[0, 1, 2])
    with pytest.raises(ValueError, match="idx"):
        ops.ransac_pairs(a, b, w, cu, cu_h, n_hyp=4, sample=3, idx=torch.zeros(2, 4, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="idx"):
        ops.ransac_pairs(a, b, w, cu, cu_h, n_hyp=4, sample=3, idx=np.zeros((2, 4, 3), dtype=np.int32))
    with pytest.raises(ValueError, match="seed"):
        ops.ransac_pairs(a, b, w, cu, cu_h, seed=-1)
