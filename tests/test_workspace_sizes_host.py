"""CPU: the size queries of the C ABI (every `*_bytes` entry of _lib.SIGNATURES; the library loads and answers them on
a machine without a GPU), and the guard-band arena of tests/workspace_arena.py on CPU tensors.

ops._workspace never hands out less than 1 MiB and every caller passes the whole buffer's size, so a query that is
too small is invisible on the GPU until tests/test_gpu_workspace.py runs every operator inside exactly what its query
returns.  What can be checked without a device is the arithmetic of the queries themselves:

  * monotone: inside the range the entry point accepts, a query never falls when one size argument grows with the others
    fixed -- a product computed in `int` before the cast to size_t, or a wrap of size_t itself, shows up as a drop;
  * related queries stay related the way include/spr.h says;
  * non-positive sizes never give a huge value (a negative int cast to size_t), and give 0 where the header says 0."""
import ctypes
import inspect

import pytest
import torch

from superpoints_registration_amd import _lib
from workspace_arena import GUARD, GUARD_BYTE, Arena

INT_MAX = (1 << 31) - 1
QUERIES = sorted(k for k in _lib.SIGNATURES if k.endswith("_bytes"))
HOST_CU = ("spr_match_workspace_bytes", "spr_sinkhorn_workspace_bytes", "spr_sinkhorn_bwd_workspace_bytes")

# name -> (base arguments, upper limit per argument).  A limit is what the matching entry point accepts (its
# SPR_REQUIREs, quoted on the right); where the entry point sets none, it is the argument type's own (INT_MAX: the sweep
# then also proves that no product leaves size_t).  None = the argument is exempt from the sweep, for the reason given.
SPECS = {
    "spr_grid_subsample_workspace_bytes": ([1000, 3], [INT_MAX, (1 << 23) - 1]),          # nb < 2^23
    "spr_voxel_downsample_workspace_bytes": ([1000], [INT_MAX]),
    "spr_radius_neighbors_workspace_bytes": ([1000, 1000, 3], [INT_MAX, INT_MAX, INT_MAX]),
    "spr_radius_table_bytes": ([1000, 3], [INT_MAX, INT_MAX]),
    "spr_radius_table_build_workspace_bytes": ([1000, 3], [INT_MAX, INT_MAX]),
    "spr_radius_table_query_workspace_bytes": ([1000], [INT_MAX]),
    "spr_gt_overlap_workspace_bytes": ([1000, 1000, 3], [1 << 25, 1 << 25, INT_MAX]),     # ns + nt <= 2^26
    "spr_augment_workspace_bytes": ([1000, 1000, 3, 1000], [1 << 25, 1 << 25, INT_MAX, INT_MAX]),   # ns + nt <= 2^26
    "spr_kpconv_workspace_bytes": ([1000, 1000, 64, 64], [INT_MAX, INT_MAX, INT_MAX, INT_MAX]),
    "spr_kpconv_plan_bytes": ([1000], [INT_MAX]),
    "spr_kpconv_wplanes_bytes": ([64, 64], [INT_MAX, 256]),                               # cout <= 256
    "spr_instnorm_workspace_bytes": ([1000, 3, 64], [INT_MAX, INT_MAX, INT_MAX]),
    # tile_rows: a taller tile means FEWER statistics tiles, so this one argument legitimately lowers the size
    "spr_block_tail_workspace_bytes": ([1000, 3, 64, 128, 64], [INT_MAX, INT_MAX, INT_MAX, INT_MAX, None]),
    "spr_block_tail_tiles_len": ([1000, 3, 64], [INT_MAX, INT_MAX, None]),                # tile_rows: as above
    "spr_cell_order_workspace_bytes": ([1000], [INT_MAX]),
    "spr_posemb_mlp_bwd_workspace_bytes": ([200], [1 << 30]),                             # t <= 2^30
    "spr_attn_workspace_bytes": ([300, 4, 8, 32], [INT_MAX, INT_MAX, INT_MAX, 32]),       # head_dim must be 32
    "spr_attn_inproj_workspace_bytes": ([300, 4, 8, 32], [INT_MAX, INT_MAX, 8, 32]),      # nhead * head_dim must be 256
    "spr_attn_probs_workspace_bytes": ([300, 8, 32], [INT_MAX, INT_MAX, None]),           # head_dim: 32 or nothing (0)
    "spr_attn_bwd_workspace_bytes": ([300, 4, 8], [INT_MAX, INT_MAX, INT_MAX]),
    "spr_attn_bwd_min_workspace_bytes": ([300, 8], [INT_MAX, INT_MAX]),
    # at most 16 layers (0 beyond); d_ff: multiples of 64 only (0 otherwise), swept in its own test below
    "spr_xenc_prepared_bytes": ([2, 1024], [16, None]),
    "spr_xenc_workspace_bytes": ([300, 4], [(1 << 22) - 1, INT_MAX]),                     # t * 256 * 4 < 2^32
    "spr_refine_pairs_workspace_bytes": ([2, 5000], [INT_MAX, 16384]),                    # SPR_REFINE_MAX_N
    "spr_loss_workspace_bytes": ([500, 400, 256], [INT_MAX, INT_MAX, 46336]),             # d * d stays an int
    "spr_tn_product_f64_workspace_bytes": ([5000, 15, 64], [INT_MAX, 1024, 4369]),        # nl * nr <= 65536
    "spr_colsum_workspace_bytes": ([256], [INT_MAX]),
    "spr_layernorm_bwd_workspace_bytes": ([256], [1024]),                                 # c <= 1024
    "spr_instnorm_bwd_workspace_bytes": ([1000, 3, 64], [INT_MAX, INT_MAX, INT_MAX]),
    "spr_scatter_workspace_bytes": ([1000, 64], [INT_MAX, INT_MAX]),
    "spr_kpconv_weighted_features_workspace_bytes": ([1000], [INT_MAX]),
    "spr_circle_loss_workspace_bytes": ([2, 300, 200], [INT_MAX, INT_MAX, INT_MAX]),
}
CONSTANT = ("spr_linear_workspace_bytes", "spr_tn_product_split_workspace_bytes", "spr_xenc_plan_bytes")
# sane ceiling of any answer inside the accepted ranges: far below what a negative int cast to size_t gives (>= 2^63)
HUGE = 1 << 62


def sweep_points(limit):
    pts = {0, 1, limit}
    k = 1
    while (1 << k) - 1 <= limit:
        pts.update(v for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if v <= limit)
        k += 1
    return sorted(pts)


def test_every_query_is_covered():
    # spr_block_tail_tiles_len counts ints, not bytes, but sizes a buffer all the same: swept with the rest
    assert set(QUERIES) | {"spr_block_tail_tiles_len"} == set(SPECS) | set(CONSTANT) | set(HOST_CU)
    for name, (base, limits) in SPECS.items():
        assert len(base) == len(limits) == len(_lib.SIGNATURES[name][1]), name


@pytest.mark.parametrize("name", sorted(SPECS))
def test_query_is_monotone_in_every_size(name):
    fn = getattr(_lib.lib(), name)
    base, limits = SPECS[name]
    for i, limit in enumerate(limits):
        if limit is None:
            continue
        prev_v, prev_r = None, None
        for v in sweep_points(limit):
            args = list(base)
            args[i] = v
            r = fn(*args)
            assert r < HUGE, f"{name}{tuple(args)} = {r}"
            assert prev_r is None or r >= prev_r, \
                f"{name} falls in argument {i}: {prev_r} at {prev_v}, {r} at {v} (others {base})"
            prev_v, prev_r = v, r


def test_constant_queries():
    L = _lib.lib()
    for name in CONSTANT:
        assert 0 < getattr(L, name)() < (1 << 20), name


def _cu(pairs):
    """The matching head's host prefix [2B + 1]: B source lengths, then B target lengths."""
    lens = [n for n, _ in pairs] + [m for _, m in pairs]
    cu = [0]
    for l in lens:
        cu.append(cu[-1] + l)
    return (ctypes.c_int * len(cu))(*cu)


@pytest.mark.parametrize("name", HOST_CU)
def test_matching_head_queries_are_monotone_in_every_cloud(name):
    """T = cu[2B] is an int and the matrices are n * m floats: one cloud grows to 2^20 tokens beside 64-token mates."""
    fn = getattr(_lib.lib(), name)
    extra = (3,) if name == "spr_sinkhorn_bwd_workspace_bytes" else ()
    for slot in range(4):                          # (pair 0 | pair 1) x (source | target)
        prev = None
        for v in [x for x in sweep_points(1 << 20) if x >= 1]:
            pairs = [[64, 64], [64, 64]]
            pairs[slot // 2][slot % 2] = v
            r = fn(_cu(pairs), 2, *extra)
            assert r < HUGE and (prev is None or r >= prev), (name, slot, v, prev, r)
            prev = r
    if extra:                                      # ... and in the number of unrolled iterations
        vals = [fn(_cu([[70, 60]]), 1, it) for it in (0, 1, 2, 3, 100)]
        assert vals == sorted(vals), vals


def test_queries_that_the_header_relates_stay_related():
    L = _lib.lib()
    for t in (1, 63, 64, 65, 300, 4097, 100000):
        for nseg in (1, 2, 6, 64):
            assert L.spr_attn_inproj_workspace_bytes(t, nseg, 8, 32) >= L.spr_attn_workspace_bytes(t, nseg, 8, 32)
            assert L.spr_xenc_workspace_bytes(t, nseg) >= L.spr_attn_workspace_bytes(t, nseg, 8, 32)
            for nhead in (1, 4, 8):
                assert L.spr_attn_bwd_workspace_bytes(t, nseg, nhead) >= L.spr_attn_bwd_min_workspace_bytes(t, nhead)
    for nq in (1, 15, 16, 17, 1000, 100000):
        for cin, cout in ((1, 64), (32, 32), (48, 24), (64, 128), (128, 256)):
            for ns in (1, 1000):
                assert L.spr_kpconv_workspace_bytes(nq, ns, cin, cout) >= \
                    L.spr_kpconv_plan_bytes(nq) + L.spr_kpconv_wplanes_bytes(cin, cout)


@pytest.mark.parametrize("name", sorted(SPECS))
def test_non_positive_sizes_never_give_a_huge_value(name):
    """With one argument at 0, -1 or INT_MIN the answer is at most what the same call gives with that argument at 1
    (the queries clamp to 1 or return 0): a negative int that reaches a size_t product unclamped gives > 2^63."""
    fn = getattr(_lib.lib(), name)
    base, _ = SPECS[name]
    for i in range(len(base)):
        one = list(base)
        one[i] = 1
        cap = max(fn(*one), fn(*base))
        for v in (0, -1, -(1 << 31)):
            args = list(base)
            args[i] = v
            assert fn(*args) <= cap, f"{name}{tuple(args)} = {fn(*args)} > {cap}"


def test_zero_where_the_header_says_zero():
    L = _lib.lib()
    assert L.spr_attn_probs_workspace_bytes(0, 8, 32) == 0 and L.spr_attn_probs_workspace_bytes(300, 0, 32) == 0
    assert L.spr_attn_probs_workspace_bytes(300, 8, 16) == 0 and L.spr_attn_probs_workspace_bytes(300, 8, 33) == 0
    assert L.spr_refine_pairs_workspace_bytes(2, 4096) == 0 and L.spr_refine_pairs_workspace_bytes(2, 4097) > 0
    assert L.spr_refine_pairs_workspace_bytes(2, 16385) == 0 and L.spr_refine_pairs_workspace_bytes(0, 5000) == 0
    assert L.spr_xenc_prepared_bytes(17, 1024) == 0 and L.spr_xenc_prepared_bytes(0, 1024) == 0
    ff = [L.spr_xenc_prepared_bytes(2, 64 * k) for k in (1, 2, 3, 16, 17, 64, 1 << 20)]
    assert ff[0] > 0 and ff == sorted(ff) and L.spr_xenc_prepared_bytes(2, 1000) == 0
    assert L.spr_xenc_workspace_bytes(0, 4) == 0 and L.spr_xenc_workspace_bytes(300, 0) == 0
    for name in ("spr_attn_workspace_bytes", "spr_attn_inproj_workspace_bytes"):
        assert getattr(L, name)(-1, 4, 8, 32) == 0 and getattr(L, name)(300, -1, 8, 32) == 0
    assert L.spr_loss_workspace_bytes(-1, 4, 32) == 0 and L.spr_gt_overlap_workspace_bytes(-1, 5, 1) == 0
    assert L.spr_augment_workspace_bytes(5, -1, 1, 0) == 0
    assert L.spr_kpconv_wplanes_bytes(0, 64) == 0 and L.spr_kpconv_wplanes_bytes(-32, 64) == 0


# ---- the arena itself, on CPU tensors ----------------------------------------------------------------------------------
def _ask(arena, nbytes):
    return arena(nbytes, "cpu"), inspect.currentframe().f_lineno


def test_arena_hands_out_exact_poisoned_views():
    arena = Arena(poison=0xFF)
    ws, line = _ask(arena, 1000)
    assert ws.numel() == 1000 and ws.dtype == torch.uint8
    assert bool((ws == 0xFF).all())
    assert ws.view(torch.float16)[:8].isnan().all() and int(ws[:4].view(torch.int32)[0]) == -1
    assert ("test_workspace_sizes_host.py", line) in arena.callers
    ws[:] = 7                                   # use of the view inside its bounds, first to last byte
    empty, _ = _ask(arena, 0)
    assert empty.numel() == 0
    zero = Arena(poison=0x00)
    assert not bool(zero(64, "cpu").any())
    arena.verify()
    zero.verify()
    assert arena.records == [] and arena.calls == 2


@pytest.mark.parametrize("side", ["before", "after"])
def test_arena_reports_the_caller_side_and_offset_of_an_overrun(side):
    arena = Arena(poison=0x00)
    ws, line = _ask(arena, 512)
    _, _, whole = arena.records[0]
    assert whole.numel() == GUARD + 512 + GUARD and int(whole[0]) == GUARD_BYTE
    if side == "before":
        whole[GUARD - 1] = 0                    # the byte just in front of the view
        where = GUARD - 1
    else:
        whole[GUARD + 512] = 0                  # the byte just behind it
        where = 0
    assert arena.damage() == [(f"test_workspace_sizes_host.py:_ask:{line}", 512, side, where)]
    with pytest.raises(AssertionError) as e:
        arena.verify()
    msg = str(e.value)
    assert f"_ask:{line}" in msg and "512 bytes" in msg and side in msg and f"offset {where}" in msg
    assert arena.records == []                  # released either way


def test_arena_sees_through_the_loss_helper():
    """_loss_ws only forwards to _workspace: the arena records the helper's own line and its caller's."""
    arena = Arena(poison=0x00)

    def _loss_ws(n):
        return arena(n, "cpu"), inspect.currentframe().f_lineno

    (_, inner), outer = _loss_ws(32), inspect.currentframe().f_lineno
    assert {("test_workspace_sizes_host.py", inner), ("test_workspace_sizes_host.py", outer)} <= arena.callers
    arena.verify()
