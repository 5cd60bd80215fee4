"""Times Preprocessor.forward under the two neighbour selection rules -- 'nearest' (the default: the reference's CPU
Preprocessor) and 'index' (neighbor_select='index': the rows of the reference's PreprocessorGPU) -- on
  * the bench batch: 64 pairs of 16 384 points (synthetic.make_pair), 3DMatch config, and
  * 8 LiDAR-shaped pairs (synthetic.make_lidar_pair()), KITTI config,
in one process.  Every forward reads row counts back to the host, so a repetition is a host clock around the call plus
a device synchronise; the rules alternate inside every repetition (same box, same minute), after warm-up forwards of
both (the second forward of a Preprocessor picks the wave-per-query selection for the searches whose rows were dense
in the first).  One JSON line per (workload, rule): median / min / max over the repetitions; the spread of the
'nearest' rule (max - min) is the margin a difference has to exceed to mean anything.  --searches adds, per level,
device-event times of the conv self search alone under both rules and both selections of the table query.

    python scripts/ball_query_bench.py [--reps 7] [--rules nearest,index] [--searches]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from superpoints_registration_amd import get_config, ops, sharding, synthetic  # noqa: E402
from superpoints_registration_amd.kpconv import Preprocessor  # noqa: E402


def workloads(which):
    if "3dmatch" in which:
        yield "3dmatch", [synthetic.make_pair(16384, seed=sd) for sd in sharding.pair_seeds(0, 64)]
    if "kitti" in which:
        yield "kitti", [synthetic.make_lidar_pair(seed=sd) for sd in range(8)]


def event_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rules", default="nearest,index")
    ap.add_argument("--workloads", default="3dmatch,kitti")
    ap.add_argument("--searches", action="store_true")
    args = ap.parse_args()
    assert args.reps >= 5, "the spread needs at least five repetitions"
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    dev = torch.device("cuda:0")
    rules = args.rules.split(",")
    for tag, pairs in workloads(args.workloads.split(",")):
        cfg = get_config(tag)
        clouds = [torch.from_numpy(p[0]).to(dev) for p in pairs] + [torch.from_numpy(p[1]).to(dev) for p in pairs]
        # (the default rule is built without the argument, so the script also times a tree from before the switch)
        pre = {r: Preprocessor(cfg) if r == "nearest" else Preprocessor(cfg, neighbor_select=r) for r in rules}
        for _ in range(args.warmup):
            for r in rules:
                meta = pre[r](clouds)
        torch.cuda.synchronize()
        ts = {r: [] for r in rules}
        for rep in range(args.reps):
            for r in (rules if rep % 2 == 0 else rules[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                meta = pre[r](clouds)
                torch.cuda.synchronize()
                ts[r].append(1e3 * (time.perf_counter() - t0))
        for r in rules:
            print(json.dumps(dict(leg="preprocessor_forward", workload=tag, rule=r, clouds=len(clouds),
                                  points=int(sum(c.shape[0] for c in clouds)), reps=args.reps,
                                  ms=round(statistics.median(ts[r]), 3), ms_min=round(min(ts[r]), 3),
                                  ms_max=round(max(ts[r]), 3), spread_ms=round(max(ts[r]) - min(ts[r]), 3),
                                  max_counts={f"{k[0]}{k[1]}": int(v) for k, v in sorted(pre[r]._row_counts.items())})),
                  flush=True)
        if len(rules) == 2:
            a, b = (statistics.median(ts[r]) for r in rules)
            print(json.dumps(dict(leg="preprocessor_forward", workload=tag, ratio=f"{rules[1]}/{rules[0]}",
                                  value=round(b / a, 4))), flush=True)
        if not args.searches:
            continue
        for l, pts in enumerate(meta['points']):
            cu = meta['_cu'][l]
            radius, limit = cfg.first_subsampling_dl * cfg.conv_radius * 2 ** l, int(cfg.neighborhood_limits[l])
            row = dict(leg="conv_search", workload=tag, level=l, points=int(pts.shape[0]), limit=limit)
            for r in rules:
                for dense in (False, True):
                    kw = {} if r == "nearest" else dict(select=ops.SELECT_INDEX)
                    row[f"{r}_{'wave' if dense else 'thread'}_ms"] = round(event_ms(
                        lambda: ops.RadiusTable(pts, cu, radius).query(pts, cu, limit, dense=dense, **kw), 5), 4)
            row["build_ms"] = round(event_ms(lambda: ops.RadiusTable(pts, cu, radius), 5), 4)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
