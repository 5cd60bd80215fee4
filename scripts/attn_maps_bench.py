"""Times spr_attn_probs (the attention-map kernel behind record_attn) at the bench shape: 128 segments of
~1 930 tokens (64 pairs of the bench's superpoint clouds), self and cross maps, head mean, against
  * the store bound: the maps' bytes at 6.29 TB/s (measured HBM copy rate, MI355X_MICROARCH);
  * the matrix-pipe bound: two passes of 3 split-fp16 products at the dense fp16 MFMA peak (2.5 PFLOP/s);
  * a torch baseline: per segment bmm + softmax + mean over the heads into the same padded tensor;
and the 64-pair RegTR forward with and without record_attn.  HIP events; one JSON line per result.

    python scripts/attn_maps_bench.py [--skip-model]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from superpoints_registration_amd import get_config, ops, sharding, synthetic  # noqa: E402
from superpoints_registration_amd.regtr import RegTR  # noqa: E402


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=128)
    ap.add_argument("--tokens", type=int, default=1930)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    nseg = args.segments
    lens = [int(args.tokens + rng.integers(-40, 41)) for _ in range(nseg)]
    L, T = max(lens), sum(lens)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(T, 768, generator=g).to(dev)          # q, k as column slices of an in-projection output
    q, k = x[:, :256], x[:, 256:512]
    cu = ops.lengths_to_cu(lens, dev)
    B = nseg // 2
    kv_self = torch.arange(nseg, dtype=torch.int32, device=dev)
    kv_cross = torch.cat([torch.arange(B, nseg), torch.arange(0, B)]).to(dev, torch.int32)
    out = torch.empty(nseg, L, L, device=dev)
    place = np.zeros((nseg, 5), np.int64)
    place[:, 0] = np.arange(nseg) * L * L
    place[:, 1:] = [L, L * L, L, L]
    place_d = torch.from_numpy(place).to(dev)
    map_bytes = 4.0 * nseg * L * L
    flops = 2 * 3 * 2.0 * 32 * 8 * sum(lens[s] * lens[s] for s in range(nseg))   # 2 passes x 3 products
    for name, kv in (("self", kv_self), ("cross", kv_cross)):
        ms = timed(lambda: ops.attention_probs(q, k, cu, kv, L, 8, out=out, place=place_d, max_rows=L, max_cols=L),
                   args.reps)
        print(json.dumps(dict(leg=f"attn_probs_{name}", ms=round(ms, 4), segments=nseg, max_len=L, tokens=T,
                              map_gb=round(map_bytes / 1e9, 3), store_bound_ms=round(map_bytes / 6.29e12 * 1e3, 3),
                              mfma_bound_ms=round(flops / 2.5e15 * 1e3, 3),
                              store_rate_tbs=round(map_bytes / ms / 1e9, 2))), flush=True)

    kvh = kv_cross.tolist()
    cuh = [0] + list(np.cumsum(lens))

    def torch_maps():
        for s in range(nseg):
            qs = q[cuh[s]:cuh[s + 1]].view(-1, 8, 32).transpose(0, 1)
            ks = k[cuh[kvh[s]]:cuh[kvh[s] + 1]].view(-1, 8, 32).transpose(0, 1)
            p = torch.softmax(torch.bmm(qs, ks.transpose(1, 2)) / math.sqrt(32), dim=-1).mean(0)
            out[s, :p.shape[0], :p.shape[1]] = p

    ms = timed(torch_maps, max(2, args.reps // 4), warm=1)
    print(json.dumps(dict(leg="torch_bmm_softmax_mean_cross", ms=round(ms, 3), segments=nseg)), flush=True)

    if args.skip_model:
        return
    cfg = get_config("3dmatch")
    pairs = [synthetic.make_pair(16384, seed=sd) for sd in sharding.pair_seeds(0, 64)]
    batch = {"src_xyz": [torch.from_numpy(p[0]).to(dev) for p in pairs],
             "tgt_xyz": [torch.from_numpy(p[1]).to(dev) for p in pairs]}
    model = RegTR(cfg)
    synthetic.fill_parameters(model, seed=0)
    model = model.to(dev).eval()
    for record in (False, True):
        model.transformer_encoder.record_attn = record
        with torch.no_grad():
            ms = timed(lambda: model(dict(batch)), 3, warm=1)
        extra = {}
        if record:
            (ss, ts), (sx, tx) = model.transformer_encoder.get_attentions()
            extra = dict(maps_gb=round(sum(m.numel() for m in (ss, ts, sx, tx)) * 4 / 1e9, 2),
                         shapes=[list(m.shape) for m in (ss, ts, sx, tx)])
        print(json.dumps(dict(leg=f"regtr_64_pairs_record_{int(record)}", ms=round(ms, 2),
                              pairs_per_s=round(64e3 / ms, 1), **extra)), flush=True)


if __name__ == "__main__":
    main()
