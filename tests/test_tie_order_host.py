"""CPU: neighbour ties in the reference's order (tie_order='reference') -- the host twins of the kernels, which run the
same header code (csrc/tie_order.h): the std::sort replay against the real std::sort of the platform's C++ compiler,
and spr_tie_order_host against the reference's recorded rows (tests/golden/tie_order.npz; also against the compiled
reference itself where oracle/_ref is built).  Equality is literal everywhere: np.array_equal, no tie allowance."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import tie_order_cases as tc
from oracle import native
from superpoints_registration_amd import _lib, get_config, hip_shim, ops, tie_order
from superpoints_registration_amd.kpconv import Preprocessor, PreprocessorGPU
from superpoints_registration_amd.regtr import RegTR

# std::sort of (index, key) pairs with a comparator on the key alone -- what nanoflann's IndexDist_Sorter makes of a
# result list -- on every sequence of the input: "n k0 k1 .. k(n-1)", one after the other; prints the index order.
SORT_MAIN = r"""
#include <algorithm>
#include <cstdio>
#include <utility>
#include <vector>
int main() {
  int n;
  while (std::scanf("%d", &n) == 1) {
    std::vector<std::pair<size_t, float>> v(n);
    for (int i = 0; i < n; ++i) {
      v[i].first = i;
      if (std::scanf("%f", &v[i].second) != 1) return 1;
    }
    std::sort(v.begin(), v.end(), [](const std::pair<size_t, float>& a, const std::pair<size_t, float>& b) {
      return a.second < b.second; });
    for (const auto& p : v) std::printf("%zu ", p.first);
    std::printf("\n");
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def std_sort(tmp_path_factory):
    """sequences -> the permutations the platform's std::sort leaves them in."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler here")
    d = tmp_path_factory.mktemp("std_sort")
    src, exe = os.path.join(d, "sort_main.cpp"), os.path.join(d, "sort_main")
    with open(src, "w") as f:
        f.write(SORT_MAIN)
    subprocess.run([cxx, "-O2", "-std=c++14", "-o", exe, src], check=True)

    def run(seqs):
        text = "\n".join(f"{len(s)} " + " ".join(str(int(v)) for v in s) for s in seqs) + "\n"
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
        return [np.array(line.split(), dtype=np.int64) for line in out[:len(seqs)]]
    return run


@pytest.fixture(scope="module")
def gold():
    return tc.load_golden()


def _musser(n):
    """Musser's median-of-three killer of 2 (n // 2) keys: 1, k + 1, 3, k + 3, .. then the even numbers."""
    k = n // 2
    head = [i if i % 2 == 1 else k + i - 1 for i in range(1, k + 1)]
    return head + list(range(2, 2 * k + 1, 2))


def _organ(n):
    return list(range(n // 2)) + list(range(n // 2, 0, -1))


def test_sort_replay_is_std_sort_on_random_keys(std_sort):
    """n = 0 .. 600, keys from 1, 2, 4 or n distinct values: every length around the 16-element threshold, long
    equal-key runs (where an unstable sort's order is all there is to compare) and tie-free inputs."""
    rng = np.random.default_rng(8101)
    seqs = []
    for n in range(601):
        for distinct in (1, 2, 4, max(n, 1)):
            seqs.append(rng.integers(0, distinct, n))
    want = std_sort(seqs)
    for s, w in zip(seqs, want):
        perm, _ = tie_order.std_sort_replay(s.astype(np.float32))
        assert np.array_equal(perm, w), (len(s), len(np.unique(s)))


def test_sort_replay_takes_the_heap_path_like_std_sort(std_sort):
    """Median-of-three killers and organ pipes long enough to run out of the depth limit 2 floor(log2 n): the replay
    reports the ranges it heap-sorted, and the order still is std::sort's."""
    seqs = [np.array(f(n)) for n in (500, 1000, 2000) for f in (_musser, _organ, lambda m: [0] + _musser(m))]
    seqs += [s // 3 for s in seqs]                      # the same shapes with equal keys
    want = std_sort(seqs)
    taken = 0
    for i, (s, w) in enumerate(zip(seqs, want)):
        perm, heap = tie_order.std_sort_replay(s.astype(np.float32))
        assert np.array_equal(perm, w), (i, len(s))
        if i < len(seqs) // 2:
            assert heap >= 1, f"sequence {i} of {len(s)} keys never exhausted the depth limit"
        taken += heap
    assert taken >= len(seqs) // 2
    perm, heap = tie_order.std_sort_replay(np.arange(600, dtype=np.float32))
    assert heap == 0 and np.array_equal(perm, np.arange(600))


def _host(c, limit, name=None):
    rows, mc = tc.index_rows(name or c.name, limit)
    got, st = tie_order.apply_host(rows, c.qry, c.sup, c.q_lens, c.s_lens, c.radius, mc)
    return rows, mc, got, st


@pytest.mark.parametrize("name", tc.NAMES)
def test_host_twin_gives_the_reference_rows(gold, name):
    c = tc.cases()[name]
    ref_full = native.ref_radius_neighbors(c.qry, c.sup, c.q_lens, c.s_lens, c.radius) if native.ref_available() else None
    for limit in tc.LIMITS:
        rows, mc, got, st = _host(c, limit)
        assert mc == int(gold[f"{name}.mc"])
        assert st.set_mismatch == 0 and st.rows == len(c.qry)
        assert np.array_equal(got, tc.reference_rows(gold, name, limit)), (name, limit)
        if ref_full is not None:
            assert np.array_equal(got, ref_full[:, :limit]), (name, limit, "compiled reference")
        untouched = (got == rows).all(1)
        assert st.rows_fixed >= int((~untouched).sum())


def test_the_lattice_rows_differ_from_the_reference_without_the_fix_up(gold):
    """What the option is for: in index order nearly every lattice row differs from the reference's."""
    for limit in tc.LIMITS:
        rows, _ = tc.index_rows("lat.r27", limit)
        ref = tc.reference_rows(gold, "lat.r27", limit)
        assert (rows != ref).any(1).mean() > 0.9


def test_a_cloud_without_ties_comes_back_bit_identical(gold):
    c = tc.cases()["float600"]
    for limit in tc.LIMITS:
        rows, mc, got, st = _host(c, limit)
        assert st.rows_fixed == 0 and st.set_mismatch == 0
        assert np.array_equal(got, rows)


def test_randomised_clouds(gold):
    """300 seeded clouds of 12 - 200 points on a 2^-3 grid, each at one of the limits."""
    live = native.ref_available()
    fixed = 0
    for k in range(tc.N_RANDOM):
        c, limit = tc.random_case(k)
        rows, mc, got, st = _host(c, limit, c.name)
        assert st.set_mismatch == 0
        assert np.array_equal(tc.digest(got), gold["random.digest"][k]), (k, limit)
        if live:
            ref = native.ref_radius_neighbors(c.qry, c.sup, c.q_lens, c.s_lens, c.radius)[:, :limit]
            assert np.array_equal(got, ref), (k, limit)
        fixed += st.rows_fixed
    assert fixed > 10000


def test_rows_that_are_not_the_searchs_are_reported_and_left_alone():
    c = tc.cases()["lat.r19"]
    rows, mc = tc.index_rows("lat.r19", 17)
    bad = rows.copy()
    bad[3, 1], bad[3, 2] = bad[3, 2], bad[3, 1]             # a run out of index order
    far = int(np.setdiff1d(np.arange(256), rows[7])[0])     # a support out of range in the place of a neighbour
    bad[7, 4] = far
    with pytest.raises(RuntimeError, match="set_mismatch"):
        tie_order.apply_host(bad, c.qry, c.sup, c.q_lens, c.s_lens, c.radius, mc)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    st = np.zeros(4, np.int32)
    q, s = np.ascontiguousarray(c.qry), np.ascontiguousarray(c.sup)
    cu = np.array([0, 256, 512], np.int32)
    work = bad.copy()
    _lib.check(_lib.lib().spr_tie_order_host(p(q), p(cu), 512, p(s), p(cu), 512, 2, c.radius, p(work), 17, 17, mc,
                                             p(st)), "spr_tie_order_host")
    assert st[1] == 2 and st[2] == 0 and st[3] == 0 and st[0] == 510
    assert np.array_equal(work[[3, 7]], bad[[3, 7]])
    # a max_count below the truth: rows that do not fit are counted, not written
    work = rows.copy()
    _lib.check(_lib.lib().spr_tie_order_host(p(q), p(cu), 512, p(s), p(cu), 512, 2, c.radius, p(work), 17, 17, 8,
                                             p(st)), "spr_tie_order_host")
    assert st[2] > 0 and st[1] == 0


def test_size_queries_and_argument_checks_need_no_gpu():
    L = _lib.lib()
    big = (1 << 31) - 1
    for args in ((0, 1), (1, 1), (1000, 3), (big, big)):
        assert 0 < L.spr_kdtree_replay_size(*args) < (1 << 62)
    assert L.spr_kdtree_replay_size(2000, 3) >= L.spr_kdtree_replay_size(1000, 3)
    for args in ((0, 0, 0), (1, 1, 1), (1000, 40, 12), (big, 128, 30), (big, big, big), (-5, -5, -5)):
        assert 0 < L.spr_tie_order_workspace_size(*args) < (1 << 62)
    # one lane's share grows, the lane count shrinks: at most 64 MiB beyond the first 256 lanes
    assert L.spr_tie_order_workspace_size(1 << 20, 128, 24) <= (65 << 20)
    assert L.spr_tie_order(None, None, 5, None, None, 5, 1, 0.1, None, 3, None, 4, 8, 9, None, None, 0, None) != 0
    assert b"width" in L.spr_last_error()
    assert L.spr_kdtree_replay_build(None, None, 5, 1, None, 0, None) != 0
    assert b"kdtree_replay_build" in L.spr_last_error()


def test_option_plumbing_and_the_two_value_errors():
    for name in ("3dmatch", "kitti", "modelnet"):
        assert get_config(name).tie_order == 'index'
    cfg = get_config("3dmatch")
    ref_cfg = get_config("3dmatch", tie_order='reference')
    assert Preprocessor(cfg).tie_order == 'index' and PreprocessorGPU(cfg).tie_order == 'index'
    assert Preprocessor(cfg, tie_order='reference').tie_order == 'reference'
    assert Preprocessor(ref_cfg).tie_order == 'reference'
    assert Preprocessor(ref_cfg, tie_order='index').tie_order == 'index'
    assert RegTR(ref_cfg).preprocessor.tie_order == 'reference'
    assert RegTR(cfg).preprocessor.tie_order == 'index'
    with pytest.raises(ValueError, match="tie_order"):
        Preprocessor(cfg, tie_order='tree')
    with pytest.raises(ValueError, match="no ties"):
        Preprocessor(cfg, neighbor_select='index', tie_order='reference')
    with pytest.raises(ValueError, match="no ties"):
        Preprocessor(get_config("kitti", neighbor_select='index', tie_order='reference'))
    with pytest.raises(ValueError, match="tie_order"):
        RegTR(get_config("3dmatch", tie_order='tree'))
    z = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="tie_order"):
        ops.radius_neighbors(z, z, None, None, 0.1, 8, tie_order='tree')
    with pytest.raises(ValueError, match="no ties"):
        ops.radius_neighbors(z, z, None, None, 0.1, 8, select=ops.SELECT_INDEX, tie_order='reference')
    with pytest.raises(ValueError, match="exact_width"):
        ops.radius_neighbors(z, z, None, None, 0.1, 8, exact_width=False, tie_order='reference')
    with pytest.raises(ValueError, match="ties"):
        hip_shim.cpp_neighbors.batch_query(z, z, [4], [4], radius=0.1, ties='tree')
    assert tie_order.check('index', ops.SELECT_INDEX) == 'index'


def test_a_missing_golden_is_an_error_not_a_skip(monkeypatch, tmp_path):
    monkeypatch.setattr(tc, "GOLDEN", str(tmp_path / "tie_order.npz"))
    with pytest.raises(FileNotFoundError, match="gen_tie_order_golden"):
        tc.load_golden()
