"""Times one training step (forward, compute_loss, backward; 3DMatch config, 16 pairs of synthetic clouds of 16 384
points) by two routes, in one process:
  (a) RegTR.forward on the expanded pair lists -- every cloud goes through the pyramid, the KPConv encoder and their
      backward once per pair it appears in (the yardstick: the training step as it was before cloud / pair batches);
  (b) RegTR.forward on the batch of unique clouds and the pair list (shared_clouds.py): every cloud encoded once,
for three pair topologies:
  no_reuse  32 unique clouds, every cloud in one pair;
  chain     17 clouds, pairs (t, t + 1): every cloud but the two ends is a source once and a target once;
  scene     8 clouds, 16 of their 28 unordered pairs, every cloud used (a 3DMatch-scene-like pair list).
The labels (per-point masks, a fixed ~60 % pattern per cloud use) and the poses are made before the clock starts; no
optimizer step, so both routes see the same weights in every repetition.  Per step: device events around it, then a
synchronise.  The two routes alternate inside every repetition (a, b, a, b, ...) after warm-up steps of both; median,
minimum and maximum over the repetitions.  The two new kernels are timed on their own on the last layout: the pair
gather's backward over the token gradient, and the per-pair overlap pyramid (all levels).  One JSON line per topology:
  spread_a_ms   max - min of route (a) over the repetitions (its run-to-run spread in this process);
  b_over_a      median (b) / median (a);      b_minus_a_ms   median (b) - median (a);
  within_spread   no reuse: |b - a| <= spread_a;      faster_by_more_than_spread   reuse: a - b > spread_a.

    python scripts/shared_clouds_train_bench.py [--reps 10] [--points 16384] [--pairs 16]
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

from superpoints_registration_amd import get_config, shared_clouds, synthetic  # noqa: E402
from superpoints_registration_amd.regtr import RegTR  # noqa: E402


def topologies(npairs):
    """name -> (number of unique clouds, pair list)."""
    scene_clouds = npairs // 2
    every = [(i, j) for i in range(scene_clouds) for j in range(i + 1, scene_clouds)]
    rng = np.random.default_rng(0)
    ring = [(min(i, (i + 1) % scene_clouds), max(i, (i + 1) % scene_clouds)) for i in range(scene_clouds)]   # every cloud
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--pairs", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shared_clouds_train_bench.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    cfg = get_config("3dmatch")
    model = RegTR(cfg)
    synthetic.fill_parameters(model, seed=0)
    model = model.to(dev).train()

    topo = topologies(args.pairs)
    n_clouds = max(u for u, _ in topo.values())
    made = [synthetic.make_pair(args.points, seed=1000 + k) for k in range((n_clouds + 1) // 2)]
    clouds = [torch.from_numpy(c).to(dev) for p in made for c in (p[0], p[1])]
    pose = torch.eye(4, device=dev)[None, :3].repeat(args.pairs, 1, 1).contiguous()
    g = torch.Generator().manual_seed(777)
    torch.cuda.synchronize()

    for name, (unique, pairs) in topo.items():
        assert len(pairs) == args.pairs and {i for p in pairs for i in p} == set(range(unique))
        own = clouds[:unique]
        src_ov = [(torch.rand(own[i].shape[0], generator=g) < 0.6).to(dev) for i, _ in pairs]
        tgt_ov = [(torch.rand(own[j].shape[0], generator=g) < 0.6).to(dev) for _, j in pairs]
        labels = {"pose": pose, "src_overlap": src_ov, "tgt_overlap": tgt_ov}

        def step(batch):
            out = model(batch)
            losses = model.compute_loss(out, batch)
            model.zero_grad(set_to_none=True)
            losses["total"].backward()
            return losses, batch

        def route_a():
            return step(dict(labels, src_xyz=[own[i] for i, _ in pairs], tgt_xyz=[own[j] for _, j in pairs]))

        def route_b():
            return step(dict(labels, clouds=own, pairs=pairs))

        for _ in range(args.warm):
            route_a()
            route_b()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(args.reps):
            ms, (loss_a, _) = event_ms(route_a)
            ta.append(ms)
            ms, (loss_b, batch_b) = event_ms(route_b)
            tb.append(ms)
        loss_diff = abs(float(loss_a["total"].detach()) - float(loss_b["total"].detach()))

        # the two new kernels alone, on the last step's layout
        layout, meta = batch_b["_pair_layout"], batch_b["kpconv_meta"]
        cu = meta["_cu"][layout.levels - 1]
        gy = torch.randn(layout.rows[-1], cfg.d_embed, device=dev)
        t_in = int(sum(meta["_lens_host"][-1]))
        ov = torch.cat(src_ov + tgt_ov).float()

        def gather_bwd():
            shared_clouds.pair_gather_bwd(gy, cu, layout.use_ptr, layout.use_seg, layout.cu_out[-1], rows=t_in)

        def pyramid():
            shared_clouds.overlap_pyramid(ov, meta, layout)

        timed = {}
        for key, fn in (("gather_bwd", gather_bwd), ("overlap_pyramid", pyramid)):
            for _ in range(args.warm):
                fn()
            torch.cuda.synchronize()
            timed[key] = stats([event_ms(fn)[0] for _ in range(args.reps)])

        a, b = stats(ta), stats(tb)
        spread = round(a["ms_max"] - a["ms_min"], 3)
        diff = round(b["ms"] - a["ms"], 3)
        res = dict(topology=name, pairs=len(pairs), unique_clouds=unique, points_per_cloud=args.points,
                   superpoints_encoded=t_in, token_rows_gathered=int(layout.rows[-1]),
                   a_expanded_step=a, b_shared_step=b, gather_bwd=timed["gather_bwd"],
                   gather_bwd_gbytes_per_s=round((layout.rows[-1] + t_in) * cfg.d_embed * 4 /
                                                 (timed["gather_bwd"]["ms"] * 1e-3) / 1e9, 1),
                   overlap_pyramid=timed["overlap_pyramid"], spread_a_ms=spread, b_minus_a_ms=diff,
                   b_over_a=round(b["ms"] / a["ms"], 4), total_loss_difference=float(f"{loss_diff:.3e}"))
        if name == "no_reuse":
            res["within_spread"] = bool(abs(diff) <= spread)
        else:
            res["faster_by_more_than_spread"] = bool(-diff > spread)
        print(json.dumps(res), flush=True)
        del loss_a, loss_b, batch_b, layout, meta, gy
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
