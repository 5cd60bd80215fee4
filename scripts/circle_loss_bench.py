"""Times the circle feature loss (ops.circle_loss: csrc/circle_loss.hip + two spr_bgemm calls in the
backward) at the train-step shape: 16 pairs of ~1 930 superpoints, D = 256, LayerNorm-scale features,
against
  * the f32 vector bound: 3 passes (forward, backward statistics, backward G) of 3 flops per
    (row, column, k) direct difference at 157 TFLOP/s, plus the two backward products at the same peak;
  * a torch baseline: the reference's formula per pair with fd from torch.cdist (matmul expansion; the
    reference's own cdist builds an [N, D, M] difference tensor, ~3.8 GB per pair at this shape);
and, unless --skip-model, one 16-pair training step (forward + compute_loss + backward) of RegTR with
feature_loss_type infonce and circle.  HIP events; one JSON line per result.

    python scripts/circle_loss_bench.py [--skip-model]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

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


def torch_circle(fs, ft, xa, xb, r_p, r_n):
    """The reference's get_circle_loss (feature_loss.py:191-233) with fd = torch.cdist(...)."""
    tot = 0
    for a, b, x, y in zip(fs, ft, xa, xb):
        cd = torch.cdist(x, y)
        fd = torch.cdist(a, b)
        pos, neg = cd < r_p, cd > r_n
        row_sel = (pos.sum(-1) > 0) & (neg.sum(-1) > 0)
        col_sel = (pos.sum(-2) > 0) & (neg.sum(-2) > 0)
        p = fd - 1e5 * (~pos).float()
        wp = torch.clamp_min(p - 0.1, 0).detach()
        lp = 10 * (p - 0.1) * wp
        q = fd + 1e5 * (~neg).float()
        wn = torch.clamp_min(1.4 - q, 0).detach()
        ln = 10 * (1.4 - q) * wn
        lr = F.softplus(torch.logsumexp(lp, -1) + torch.logsumexp(ln, -1)) / 10
        lc = F.softplus(torch.logsumexp(lp, -2) + torch.logsumexp(ln, -2)) / 10
        tot = tot + (lr[row_sel].mean() + lc[col_sel].mean()) / 2
    return tot / len(fs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--tokens", type=int, default=1930)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    B, D = args.pairs, 256
    ns = [int(args.tokens + rng.integers(-40, 41)) for _ in range(B)]
    ms_ = [int(args.tokens + rng.integers(-40, 41)) for _ in range(B)]
    g = torch.Generator().manual_seed(0)

    def ln(n):
        x = torch.randn(n, D, generator=g)
        return ((x - x.mean(1, keepdim=True)) / x.std(1, keepdim=True)).to(dev)

    fs, ft = [ln(n) for n in ns], [ln(m) for m in ms_]
    xs = [(torch.rand(n, 3, generator=g) * 2.5).to(dev) for n in ns]      # superpoints of a ~2.5 m scene
    xt = [(torch.rand(m, 3, generator=g) * 2.5).to(dev) for m in ms_]
    pose = torch.eye(4)[:3].expand(B, 3, 4).contiguous().to(dev)
    r_p, r_n = 0.2, 0.4
    fs_g = [f.clone().requires_grad_(True) for f in fs]
    ft_g = [f.clone().requires_grad_(True) for f in ft]
    a_pk = torch.cat(fs).requires_grad_(True)
    b_pk = torch.cat(ft).requires_grad_(True)
    xs_pk, xt_pk = torch.cat(xs), torch.cat(xt)

    entries = sum(n * m for n, m in zip(ns, ms_))
    bound_ms = (3 * 3.0 * entries * D + 2 * 2.0 * entries * D) / 157e12 * 1e3

    with torch.no_grad():
        ms = timed(lambda: ops.circle_loss_packed(a_pk, b_pk, xs_pk, pose, xt_pk, ns, ms_, r_p, r_n), args.reps)
    print(json.dumps(dict(leg="circle_fwd", ms=round(ms, 4), pairs=B, entries=entries)), flush=True)

    def fwd_bwd():
        ops.circle_loss_packed(a_pk, b_pk, xs_pk, pose, xt_pk, ns, ms_, r_p, r_n).mean().backward()

    ms = timed(fwd_bwd, args.reps)
    print(json.dumps(dict(leg="circle_fwd_bwd", ms=round(ms, 4), pairs=B, f32_vector_bound_ms=round(bound_ms, 3),
                          target_ms=1.5)), flush=True)

    def torch_fwd_bwd():
        torch_circle(fs_g, ft_g, xs, xt, r_p, r_n).backward()

    ms = timed(torch_fwd_bwd, max(2, args.reps // 2), warm=1)
    print(json.dumps(dict(leg="torch_cdist_fwd_bwd", ms=round(ms, 3), pairs=B)), flush=True)
    a_ = ops.circle_loss_packed(a_pk.detach(), b_pk.detach(), xs_pk, pose, xt_pk, ns, ms_, r_p, r_n).mean()
    with torch.no_grad():
        t_ = torch_circle(fs, ft, xs, xt, r_p, r_n)
    print(json.dumps(dict(leg="loss_values", hip=float(a_), torch_cdist=float(t_))), flush=True)

    if args.skip_model:
        return
    pairs = [synthetic.make_pair(16384, seed=sd) for sd in sharding.pair_seeds(0, B)]
    orng = np.random.default_rng(1)
    batch = {"src_xyz": [torch.from_numpy(p[0]).to(dev) for p in pairs],
             "tgt_xyz": [torch.from_numpy(p[1]).to(dev) for p in pairs],
             "pose": torch.from_numpy(np.stack([p[2] for p in pairs]).astype(np.float32)).to(dev),
             "src_overlap": [torch.from_numpy(orng.random(len(p[0])) < 0.6).to(dev) for p in pairs],
             "tgt_overlap": [torch.from_numpy(orng.random(len(p[1])) < 0.6).to(dev) for p in pairs]}
    for ftype in ("infonce", "circle"):
        cfg = get_config("3dmatch")
        cfg.feature_loss_type = ftype
        model = RegTR(cfg)
        synthetic.fill_parameters(model, seed=0)
        model = model.to(dev).train()

        def step():
            b = dict(batch)                      # the forward leaves kpconv_meta in the batch for compute_loss
            out = model(b)
            losses = model.compute_loss(out, b)
            model.zero_grad(set_to_none=True)
            losses["total"].backward()
            return losses

        ms = timed(step, 3, warm=1)
        losses = step()
        print(json.dumps(dict(leg=f"train_step_{ftype}", ms=round(ms, 2), pairs=B,
                              feature=float(losses["feature"]), total=float(losses["total"]))), flush=True)


if __name__ == "__main__":
    main()
