"""Times calibrate_neighbors and the count kernel under it, in one process:

  (a) calibrate_neighbors on 64 pairs of 16 384 points (synthetic.make_pair, the bench batch), 3DMatch config, with a
      samples_threshold that is never reached so that all 64 samples are used: host clock around the call plus a
      device synchronise (the call reads status words and histograms back, so it is synchronous by itself); per level
      the device-event time of the count kernel alone on a chunk of 8 samples (16 clouds), the shape calibrate_neighbors
      launches it at.  Beside it, once, the CPU replica of the reference's procedure over the CPU oracle
      (tests/calibrate_cases.py) on the same samples in a pool of --procs processes, and whether its histograms are
      the GPU's.
  (b) on the level-0 table of the whole bench batch (128 clouds): spr_radius_table_count (counts + histogram, and
      histogram alone) against spr_radius_table_query(limit=40), both selections, as self searches, launches only
      (device events around --launches back-to-back launches), alternating inside every repetition.

One JSON line per leg: median / min / max over the repetitions after warm-up.

    python scripts/calibrate_bench.py [--reps 7] [--pairs 64] [--procs 16] [--skip-cpu]
"""
import argparse
import ctypes
import json
import multiprocessing
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from superpoints_registration_amd import _lib, calibration, get_config, ops, sharding, synthetic  # noqa: E402
from superpoints_registration_amd.kpconv import plan_pyramid  # noqa: E402

NEVER = 10 ** 15      # samples_threshold that no histogram total reaches


def _stats(ts):
    return dict(ms=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4), reps=len(ts))


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def count_launch(table, counts, hist):
    L = _lib.lib()
    st = torch.empty((1,), dtype=torch.int32, device=table.supports.device)

    def fn():
        _lib.check(L.spr_radius_table_count(_vp(table.supports), _vp(table.s_cu), table.ns, 1, table.ns, table.nb,
                                            table.radius, _vp(table.blob), _vp(counts), _vp(hist),
                                            0 if hist is None else hist.shape[1], _vp(st),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "count")
    return fn


def query_launch(table, limit, algo):
    L = _lib.lib()
    dev = table.supports.device
    ws = torch.empty((L.spr_radius_table_query_workspace_bytes(table.ns),), dtype=torch.uint8, device=dev)
    out = torch.empty((table.ns, limit), dtype=torch.int32, device=dev)
    mc = torch.empty((1,), dtype=torch.int32, device=dev)

    def fn():
        _lib.check(L.spr_radius_table_query(_vp(table.supports), _vp(table.s_cu), table.ns, 1, table.ns, table.nb,
                                            table.radius, limit, 0, _vp(table.blob), _vp(out), _vp(mc), algo, 0,
                                            _vp(ws), ws.numel(),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "query")
    return fn


def event_ms(fns, reps, launches, warm=3):
    """{name: [ms per launch]}: the legs alternate inside every repetition."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    names = list(fns)
    for rep in range(reps):
        for k in (names if rep % 2 == 0 else names[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fns[k]()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b) / launches)
    return ts


def _cpu_sample(args):
    import calibrate_cases as cc
    src, tgt = args
    return cc.sample_hists({"src_xyz": src, "tgt_xyz": tgt}, get_config("3dmatch"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--skip-cpu", action="store_true")
    args = ap.parse_args()
    assert args.reps >= 5, "the spread needs at least five repetitions"
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    dev = torch.device("cuda:0")
    cfg = get_config("3dmatch")
    pairs = [synthetic.make_pair(16384, seed=sd) for sd in sharding.pair_seeds(0, args.pairs)]
    host = [{"src_xyz": p[0], "tgt_xyz": p[1]} for p in pairs]
    data = [{k: torch.from_numpy(v).to(dev) for k, v in it.items()} for it in host]
    hist_n = calibration.hist_width(cfg)

    # (a) end to end
    for _ in range(2):
        limits, hists, used = calibration.calibrate_neighbors(data, cfg, samples_threshold=NEVER, return_hists=True)
    ts = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        calibration.calibrate_neighbors(data, cfg, samples_threshold=NEVER)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps(dict(leg="calibrate_neighbors", pairs=args.pairs, points_per_cloud=16384, chunk=8, samples_used=used,
                          limits=[int(v) for v in limits], level_totals=[int(v) for v in hists.sum(1)],
                          configured=list(cfg.neighborhood_limits),
                          coverage=[round(float(v), 4) for v in calibration.coverage(hists, limits)],
                          coverage_configured=[round(float(v), 4) for v in
                                               calibration.coverage(hists, cfg.neighborhood_limits[:len(limits)])],
                          **_stats(ts))), flush=True)
    early = calibration.calibrate_neighbors(data, cfg, return_hists=True)
    print(json.dumps(dict(leg="calibrate_neighbors_default_threshold", samples_used=early[2],
                          limits=[int(v) for v in early[0]])), flush=True)

    # per level: the count kernel at the shape of one chunk (8 samples = 16 clouds)
    _, levels, _ = plan_pyramid(cfg)
    clouds = [it[k] for it in data[:8] for k in ("src_xyz", "tgt_xyz")]
    points, cu = torch.cat(clouds).contiguous(), ops.lengths_to_cu([int(c.shape[0]) for c in clouds], dev)
    for l, lv in enumerate(levels):
        table = ops.RadiusTable(points, cu, lv.radius)
        hist = torch.zeros((table.nb, hist_n), dtype=torch.int32, device=dev)
        counts = torch.empty((table.ns,), dtype=torch.int32, device=dev)
        t = event_ms({"hist": count_launch(table, None, hist)}, args.reps, args.launches)["hist"]
        count_launch(table, counts, None)()
        torch.cuda.synchronize()
        print(json.dumps(dict(leg="count_kernel_chunk", level=l, clouds=table.nb, points=table.ns, radius=lv.radius,
                              mean_count=round(float(counts.float().mean()), 2), max_count=int(counts.max()),
                              **_stats(t))), flush=True)
        if lv.down:
            points, sub_lens = ops.grid_subsample(points, cu, 2 * lv.radius / cfg.conv_radius)
            cu = ops.lengths_to_cu(sub_lens, dev)

    # (b) level-0 table of the whole batch: count against the row-producing query
    clouds = [it[k] for it in data for k in ("src_xyz", "tgt_xyz")]
    points, cu = torch.cat(clouds).contiguous(), ops.lengths_to_cu([int(c.shape[0]) for c in clouds], dev)
    table = ops.RadiusTable(points, cu, levels[0].radius)
    hist = torch.zeros((table.nb, hist_n), dtype=torch.int32, device=dev)
    counts = torch.empty((table.ns,), dtype=torch.int32, device=dev)
    legs = {"count_counts_and_hist": count_launch(table, counts, hist), "count_hist_only": count_launch(table, None, hist),
            "query_limit40_thread": query_launch(table, 40, 0), "query_limit40_wave": query_launch(table, 40, 1)}
    ts = event_ms(legs, args.reps, args.launches)
    for k, t in ts.items():
        print(json.dumps(dict(leg=k, table="level 0, whole batch", clouds=table.nb, points=table.ns,
                              mean_count=round(float(counts.float().mean()), 2), max_count=int(counts.max()),
                              **_stats(t))), flush=True)
    print(json.dumps(dict(leg="ratio", value="count_counts_and_hist / query_limit40_thread",
                          ratio=round(statistics.median(ts["count_counts_and_hist"]) /
                                      statistics.median(ts["query_limit40_thread"]), 4))), flush=True)

    # the CPU replica over the oracle, once
    if not args.skip_cpu:
        t0 = time.perf_counter()
        with multiprocessing.get_context("spawn").Pool(args.procs) as pool:
            per_sample = pool.map(_cpu_sample, [(it["src_xyz"], it["tgt_xyz"]) for it in host], chunksize=1)
        import calibrate_cases as cc
        r_limits, r_hists, r_used = cc.replica(None, cfg, 0.8, NEVER, per_sample=per_sample)
        print(json.dumps(dict(leg="cpu_replica_over_oracle", procs=args.procs, pairs=args.pairs,
                              s=round(time.perf_counter() - t0, 2), runs=1,
                              histograms_equal_gpu=bool(np.array_equal(r_hists, hists)),
                              limits_equal_gpu=bool(np.array_equal(r_limits, limits)))), flush=True)


if __name__ == "__main__":
    main()
