"""Prints one `name args value` line for every size query of the C ABI (every `*_bytes` entry of _lib.SIGNATURES plus
spr_block_tail_tiles_len) over a fixed grid; needs no GPU.  Run it on two builds and diff the outputs: a change of a
workspace layout that was meant to keep every size shows up as a changed line.

    python scripts/ws_query_dump.py > new.txt
    SPR_HIP_LIB=/path/to/other/libspr_hip.so python scripts/ws_query_dump.py > old.txt

The grid: the bases of tests/test_workspace_sizes_host.py::SPECS with each argument swept over sweep_points(limit) and
over 0, -1, INT_MIN; the host-prefix queries over that file's cloud sweeps; the shapes of tests/test_gpu_workspace.py
(SEGS, the block-tail shapes, the kpconv channel pairs and token counts of
test_queries_that_the_header_relates_stay_related); the bench shape (64 pairs of 16 384 points, 247 k tokens)."""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_workspace_sizes_host as H  # noqa: E402
from superpoints_registration_amd import _lib  # noqa: E402

# tests/test_gpu_workspace.py::SEGS and tests/test_gpu_block_tail.py::SHAPES / LENS (importing those modules needs a GPU build
# of everything they test; the numbers are restated)
SEGS = {"ragged": ([70, 129, 33], [200, 1, 64]), "one": ([1], [1]), "tiles": ([64, 64], [64, 64])}
TAIL_SHAPES = [(32, 64, 128), (32, 0, 128), (64, 128, 256), (64, 0, 256), (128, 256, 512), (128, 0, 512)]
TAIL_LENS = [1, 63, 64, 65, 700, 129, 2048, 17, 3001]
KP_CHANNELS = ((1, 64), (32, 32), (48, 24), (64, 128), (128, 256))
BENCH_PAIRS, BENCH_POINTS, BENCH_TOKENS = 64, 16384, 247000


def grid():
    """name -> set of argument tuples (ints only; the host-prefix queries are handled apart)."""
    g = {name: set() for name in list(H.SPECS) + list(H.CONSTANT)}
    for name in H.CONSTANT:
        g[name].add(())
    for name, (base, limits) in H.SPECS.items():
        g[name].add(tuple(base))
        for i, limit in enumerate(limits):
            pts = [0, -1, -(1 << 31), 1] + (H.sweep_points(limit) if limit is not None else [])
            for v in pts:
                args = list(base)
                args[i] = v
                g[name].add(tuple(args))
    # token operators: SEGS, the related-queries sweep, the bench
    tok = {(sum(s) + sum(t), 2 * len(s)) for s, t in SEGS.values()}
    tok |= set(itertools.product((1, 63, 64, 65, 300, 4097, 100000), (1, 2, 6, 64)))
    tok.add((BENCH_TOKENS, 2 * BENCH_PAIRS))
    for t, nseg in tok:
        g["spr_attn_workspace_bytes"].add((t, nseg, 8, 32))
        g["spr_attn_inproj_workspace_bytes"].add((t, nseg, 8, 32))
        g["spr_xenc_workspace_bytes"].add((t, nseg))
        g["spr_attn_probs_workspace_bytes"].add((t, 8, 32))
        g["spr_posemb_mlp_bwd_workspace_bytes"].add((t,))
        for nhead in (1, 4, 8):
            g["spr_attn_bwd_workspace_bytes"].add((t, nseg, nhead))
            g["spr_attn_bwd_min_workspace_bytes"].add((t, nhead))
    # point operators: the GPU module's clouds, the kpconv golden (600 points), the bench's level 0
    for n, nb in ((513, 3), (514, 3), (600, 1), (BENCH_PAIRS * 2 * BENCH_POINTS, 2 * BENCH_PAIRS)):
        g["spr_grid_subsample_workspace_bytes"].add((n, nb))
        g["spr_voxel_downsample_workspace_bytes"].add((n,))
        g["spr_cell_order_workspace_bytes"].add((n,))
        g["spr_radius_neighbors_workspace_bytes"].add((n, n, nb))
        g["spr_radius_table_bytes"].add((n, nb))
        g["spr_radius_table_build_workspace_bytes"].add((n, nb))
        g["spr_radius_table_query_workspace_bytes"].add((n,))
        g["spr_kpconv_weighted_features_workspace_bytes"].add((n,))
        for c in (64, 128):
            g["spr_instnorm_workspace_bytes"].add((n // nb + 1, nb, c))
            g["spr_instnorm_bwd_workspace_bytes"].add((n // nb + 1, nb, c))
            g["spr_scatter_workspace_bytes"].add((n, c))
    half = BENCH_PAIRS * BENCH_POINTS
    for ns, nt, nb in ((513, 513, 3), (514, 514, 3), (half, half, BENCH_PAIRS)):
        g["spr_gt_overlap_workspace_bytes"].add((ns, nt, nb))
        g["spr_augment_workspace_bytes"].add((ns, nt, nb, max(ns, nt) // nb + 1))
    for nq in (1, 15, 16, 17, 600, 1000, 100000, BENCH_PAIRS * 2 * BENCH_POINTS):
        g["spr_kpconv_plan_bytes"].add((nq,))
        for (cin, cout), ns in itertools.product(KP_CHANNELS + ((128, 128),), (1, 600, 1000)):
            g["spr_kpconv_workspace_bytes"].add((nq, ns, cin, cout))
    for cin, cout in KP_CHANNELS + ((128, 128),):
        g["spr_kpconv_wplanes_bytes"].add((cin, cout))
    n = sum(TAIL_LENS)
    for (ka, kb, n_out), tile_rows in itertools.product(TAIL_SHAPES, (16, 32, 64)):
        g["spr_block_tail_workspace_bytes"].add((n, len(TAIL_LENS), kb, n_out, tile_rows))
        g["spr_block_tail_tiles_len"].add((n, len(TAIL_LENS), tile_rows))
    for n in (100, 4096, 4097, 16384):
        g["spr_refine_pairs_workspace_bytes"].add((1, n))
        g["spr_refine_pairs_workspace_bytes"].add((BENCH_PAIRS, n))
    for nm, d in itertools.product(((500, 400), (1, 1), (2000, 1900)), (32, 256)):
        g["spr_loss_workspace_bytes"].add(nm + (d,))
        g["spr_circle_loss_workspace_bytes"].add((16,) + nm)
    return g


def cloud_cases():
    """(label, pairs) for the host-prefix queries: the sweeps of test_matching_head_queries_are_monotone_in_every_cloud,
    the GPU module's pairs, the bench."""
    for slot in range(4):
        for v in [x for x in H.sweep_points(1 << 20) if x >= 1]:
            pairs = [[64, 64], [64, 64]]
            pairs[slot // 2][slot % 2] = v
            yield pairs
    yield [[70, 60]]
    yield [[1, 1], [63, 65], [129, 200]]
    yield [[1, 1]]
    yield [[1930, 1930]] * BENCH_PAIRS


def main():
    L = _lib.lib()
    lines = []
    for name, tuples in sorted(grid().items()):
        fn = getattr(L, name)
        for args in sorted(tuples):
            lines.append(f"{name} {','.join(map(str, args))} {fn(*args)}")
    for name in H.HOST_CU:
        fn = getattr(L, name)
        for pairs in cloud_cases():
            label = ";".join(f"{n}x{m}" for n, m in pairs) if len(pairs) < 8 else f"{len(pairs)}*{pairs[0][0]}x{pairs[0][1]}"
            if name == "spr_sinkhorn_bwd_workspace_bytes":
                for it in (0, 1, 2, 3, 100):
                    lines.append(f"{name} {label},{it} {fn(H._cu(pairs), len(pairs), it)}")
            else:
                lines.append(f"{name} {label} {fn(H._cu(pairs), len(pairs))}")
    covered = {l.split()[0] for l in lines}
    assert covered == set(H.QUERIES) | {"spr_block_tail_tiles_len"}, set(H.QUERIES) ^ covered
    print("\n".join(lines))
    print(f"# {len(lines)} points", file=sys.stderr)


if __name__ == "__main__":
    main()
