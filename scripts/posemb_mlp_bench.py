"""Times the learned positional embedding at the bench's token count: the coarsest-level points of a real bench batch
(64 pairs of 16 384-point clouds, bench.py's seeds, 3DMatch pyramid), in one process:
  fused     ops.posemb_mlp: the five layers in one kernel (csrc/posemb_mlp.hip, exact f32);
  backward  ops.posemb_mlp_bwd: recompute + deltas, five weight-gradient products, five column sums;
  chain     the yardstick: the same MLP as five ops.linear calls (existing code: the split-fp16 GEMM with fused bias
            and ReLU, ranges handed from layer to layer), whose intermediates go through memory.
Per call: device events around the call, then a synchronise.  fused and chain alternate inside every repetition after
warm-up calls of all three; median, minimum and maximum over the repetitions.  The forward's FLOP bound is
2 * 108 640 FLOP per token over the exact-f32 matrix peak (157.3 TFLOP/s), its weight-traffic bound 434 560 bytes per
64-token workgroup over the L2 bandwidth is reported as bytes only.  Writes profiles/posemb_mlp_bench.txt.

    python scripts/posemb_mlp_bench.py [--reps 30] [--points 16384] [--pairs 64]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from superpoints_registration_amd import get_config, ops, sharding, synthetic  # noqa: E402
from superpoints_registration_amd.regtr import RegTR  # noqa: E402

MACS_PER_TOKEN = 3 * 32 + 32 * 64 + 64 * 128 + 128 * 256 + 256 * 256      # 108 640 - the biases
PEAK_F32_MATRIX = 157.3e12


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "posemb_mlp_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "posemb_mlp_bench needs the MI355X"
    dev = torch.device("cuda:0")
    model = RegTR(get_config("3dmatch", pos_emb_type="learned"))
    synthetic.fill_parameters(model, seed=0)
    model = model.to(dev).eval()
    pairs = [synthetic.make_pair(args.points, seed=s) for s in sharding.pair_seeds(0, args.pairs)]
    clouds = [torch.from_numpy(p[0]).to(dev) for p in pairs] + [torch.from_numpy(p[1]).to(dev) for p in pairs]
    with torch.no_grad():
        xyz = model.preprocessor(clouds)["points"][-1].contiguous()
    T = xyz.shape[0]
    mlp = model.pos_embed.mlp
    params = [p.detach() for i in (0, 2, 4, 6, 8) for p in (mlp[i].weight, mlp[i].bias)]
    dpe = synthetic.rand((T, 256), 1).to(dev)

    def chain():
        h = xyz
        for l in range(5):
            h = ops.linear(h, params[2 * l], params[2 * l + 1], act=ops.ACT_RELU if l < 4 else ops.ACT_NONE)
        return h

    fused = lambda: ops.posemb_mlp(xyz, params)
    bwd = lambda: ops.posemb_mlp_bwd(xyz, params, dpe)
    with torch.no_grad():
        for _ in range(3):
            a, b, _ = fused(), chain(), bwd()
        torch.cuda.synchronize()
        diff = float((a - b).abs().max() / b.abs().max())
        t = {"fused": [], "chain": [], "backward": []}
        for _ in range(args.reps):
            t["fused"].append(event_ms(fused)[0])
            t["chain"].append(event_ms(chain)[0])
            t["backward"].append(event_ms(bwd)[0])
    res = {k: stats(v) for k, v in t.items()}
    bound_ms = 2.0 * MACS_PER_TOKEN * T / PEAK_F32_MATRIX * 1e3
    res.update(tokens=T, pairs=args.pairs, points=args.points, reps=args.reps,
               fused_vs_chain_max_rel_diff=diff,
               fused_flop_bound_ms=round(bound_ms, 4),
               fused_fraction_of_flop_bound=round(bound_ms / res["fused"]["median_ms"], 4),
               fused_weight_bytes_from_l2=int((T + 63) // 64 * MACS_PER_TOKEN * 4),
               chain_intermediate_bytes=int(T * (32 + 64 + 128 + 256) * 4 * 2),
               fused_over_chain=round(res["fused"]["median_ms"] / res["chain"]["median_ms"], 4))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
