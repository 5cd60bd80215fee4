"""Times registration of 64 pairs (3DMatch config, synthetic clouds of 16 384 points) by two routes, in one process:
  (a) RegTR.forward on the pair list -- every cloud goes through the pyramid and the KPConv encoder once per pair it
      appears in (the yardstick: the forward as it was before encode / register existed);
  (b) RegTR.encode of the unique clouds, then RegTR.register of the pair list over the encodings,
for three pair topologies:
  no_reuse  128 unique clouds, every cloud in one pair;
  chain     65 clouds, pairs (t, t + 1): every cloud but the two ends is a source once and a target once;
  scene     16 clouds, 64 of their 120 unordered pairs, every cloud used (a 3DMatch-scene-like pair list).
Per call: device events around the call, then a synchronise.  The two routes alternate inside every repetition (a, b,
a, b, ...) after warm-up calls of both; median, minimum and maximum over the repetitions.  Route (b) is also split by
an event between encode and register.  The pair gathers of route (b) (ops.pair_gather of the tokens and of the
points) are timed on their own.  One JSON line per topology:
  spread_a_ms        max - min of route (a) over the repetitions (its run-to-run spread in this process);
  b_over_a           median (b) / median (a);
  b_minus_a_ms       median (b) - median (a);
  within_spread_plus_gather   no reuse: b - a <= spread_a + gather;     faster_by_more_than_spread   reuse: a - b > spread_a.

    python scripts/encode_once_bench.py [--reps 15] [--points 16384] [--pairs 64]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from superpoints_registration_amd import get_config, ops, synthetic  # noqa: E402
from superpoints_registration_amd.regtr import RegTR  # noqa: E402
from superpoints_registration_amd.transformers import make_segments  # noqa: E402


def topologies(npairs):
    """name -> (number of unique clouds, pair list)."""
    scene_clouds = 16
    every = [(i, j) for i in range(scene_clouds) for j in range(i + 1, scene_clouds)]
    rng = np.random.default_rng(0)
    ring = [(i, (i + 1) % scene_clouds) for i in range(scene_clouds)]            # touches every cloud
    ring = [(min(p), max(p)) for p in ring]
    rest = [p for p in every if p not in ring]
    pick = rng.permutation(len(rest))[:npairs - len(ring)]
    scene = ring + [rest[k] for k in sorted(pick)]
    return {
        "no_reuse": (2 * npairs, [(2 * b, 2 * b + 1) for b in range(npairs)]),
        "chain": (npairs + 1, [(t, t + 1) for t in range(npairs)]),
        "scene": (scene_clouds, scene[:npairs]),
    }


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def stats(ts):
    return dict(ms=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--pairs", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("encode_once_bench.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    cfg = get_config("3dmatch")
    model = RegTR(cfg)
    synthetic.fill_parameters(model, seed=0)
    model = model.to(dev).eval()

    topo = topologies(args.pairs)
    n_clouds = max(u for u, _ in topo.values())
    made = [synthetic.make_pair(args.points, seed=1000 + k) for k in range((n_clouds + 1) // 2)]
    clouds = [torch.from_numpy(c).to(dev) for p in made for c in (p[0], p[1])]
    torch.cuda.synchronize()

    for name, (unique, pairs) in topo.items():
        assert len(pairs) == args.pairs and {i for p in pairs for i in p} == set(range(unique))
        own = clouds[:unique]

        def route_a():
            with torch.no_grad():
                return model({"src_xyz": [own[i] for i, _ in pairs], "tgt_xyz": [own[j] for _, j in pairs]})

        def route_b():
            mid = torch.cuda.Event(enable_timing=True)
            with torch.no_grad():
                enc = model.encode(own)
                mid.record()
                return model.register(enc, pairs), mid, enc

        for _ in range(args.warm):
            route_a()
            route_b()
        torch.cuda.synchronize()
        ta, tb, t_enc = [], [], []
        for _ in range(args.reps):
            ms, out_a = event_ms(route_a)
            ta.append(ms)
            beg = torch.cuda.Event(enable_timing=True)
            beg.record()
            ms, (out_b, mid, enc) = event_ms(route_b)
            tb.append(ms)
            t_enc.append(beg.elapsed_time(mid))
        pose_diff = float((out_a["pose"] - out_b["pose"]).flatten(1).norm(dim=1).max())

        # the pair gathers of route (b) alone, on the last encoding
        P = len(pairs)
        src_lens, tgt_lens = [enc.lens[i] for i, _ in pairs], [enc.lens[j] for _, j in pairs]
        cu_out = make_segments(src_lens, tgt_lens, dev)[0]
        idx = torch.tensor([i for i, _ in pairs] + [j for _, j in pairs], dtype=torch.int32, device=dev)
        rows = sum(src_lens) + sum(tgt_lens)

        def gathers():
            ops.pair_gather(enc.tokens, enc.cu, idx[:P], idx[P:], cu_out, rows=rows)
            ops.pair_gather(enc.points, enc.cu, idx[:P], idx[P:], cu_out, rows=rows)

        for _ in range(args.warm):
            gathers()
        torch.cuda.synchronize()
        tg = [event_ms(gathers)[0] for _ in range(args.reps)]

        a, b, g = stats(ta), stats(tb), stats(tg)
        spread = round(a["ms_max"] - a["ms_min"], 3)
        diff = round(b["ms"] - a["ms"], 3)
        res = dict(topology=name, pairs=P, unique_clouds=unique, points_per_cloud=args.points,
                   superpoints_encoded=int(sum(enc.lens)), rows_gathered=int(rows),
                   a_forward=a, b_encode_register=b, b_encode_ms=round(statistics.median(t_enc), 3),
                   b_register_ms=round(b["ms"] - statistics.median(t_enc), 3), gather=g,
                   gather_gbytes_per_s=round(2 * rows * (cfg.d_embed + 3) * 4 / (g["ms"] * 1e-3) / 1e9, 1),
                   spread_a_ms=spread, b_minus_a_ms=diff, b_over_a=round(b["ms"] / a["ms"], 4),
                   max_pose_difference=float(f"{pose_diff:.3e}"))
        if name == "no_reuse":
            res["within_spread_plus_gather"] = bool(diff <= spread + g["ms"])
        else:
            res["faster_by_more_than_spread"] = bool(-diff > spread)
        print(json.dumps(res), flush=True)
        del out_a, out_b, enc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
