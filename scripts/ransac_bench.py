"""Times RANSAC (cfg.use_ransac) through
  * new     ops.ransac_pairs: all pairs in one call (two launches);
  * parent  the per-pair loop it replaced: RegTR._ransac for every pair (torch.randint, three gathers, one
            ops.weighted_procrustes launch over the 500 sample sets, one ops.pose_scores launch, argmin, index) and a
            torch.stack, exactly as RegTR._refined_pose ran it;
at two levels:
  operator   B = --pairs sets of --n correspondences each (1 200: the bench batch's superpoint counts), --hyp x --sample;
  register   RegTR._register of the 64-pair bench batch (bench.py's pairs: 16 384-point box clouds, 3DMatch config,
             use_sinkhorn off so that the arg-max correspondences carry the pose) with use_ransac, the parent loop
             swapped in for the RANSAC step in the same process, on the same encodings; and without use_ransac, for scale.
Every leg is timed with HIP events over --reps calls after --warm warm-up calls, legs interleaved --rounds times, the
median round reported.  One JSON line per leg.

    python scripts/ransac_bench.py [--pairs 64] [--n 1200] [--reps 5] [--rounds 5] [--no-register]
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

from superpoints_registration_amd import get_config, ops, sharding, synthetic  # noqa: E402
from superpoints_registration_amd.regtr import RegTR  # noqa: E402
from superpoints_registration_amd.transformers import make_segments  # noqa: E402


def timed(fn, reps, warm):
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


def report(leg, ms, **extra):
    print(json.dumps(dict(leg=leg, ms=round(statistics.median(ms), 3), ms_min=round(min(ms), 3),
                          ms_max=round(max(ms), 3), rounds=len(ms), **extra)), flush=True)


def parent_ransac(src_pts, tgt_pts, val, n_hyp, sample):
    return torch.stack([RegTR._ransac(src_pts[b].contiguous(), tgt_pts[b].contiguous(), val[b].contiguous(), n_hyp,
                                      sample) for b in range(len(val))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--n", type=int, default=1200)
    ap.add_argument("--hyp", type=int, default=500)
    ap.add_argument("--sample", type=int, default=100)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-register", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, n, H, S = args.pairs, args.n, args.hyp, args.sample

    # ---- operator level ----
    rng = np.random.default_rng(0)
    a = rng.uniform(-12, 12, (B * n, 3)).astype(np.float32)
    th = 0.2
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    b = (a @ R.T + np.array([0.4, -0.2, 0.05]) + rng.normal(0, 0.024, a.shape)).astype(np.float32)
    b[rng.permutation(B * n)[:B * n // 10]] += 2.0
    da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    dw = torch.from_numpy(rng.uniform(0.05, 1, B * n).astype(np.float32)).to(dev)
    cu_host = [n * i for i in range(B + 1)]
    cu = torch.tensor(cu_host, dtype=torch.int32, device=dev)
    sa, sb, sw = list(da.split(n)), list(db.split(n)), list(dw.split(n))
    legs = {"ransac_parent_loop": lambda: parent_ransac(sa, sb, sw, H, S),
            "ransac_pairs": lambda: ops.ransac_pairs(da, db, dw, cu, cu_host, n_hyp=H, sample=S)}
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            ms[k].append(timed(fn, args.reps, args.warm))
    for k in legs:
        report(k, ms[k], pairs=B, n=n, n_hyp=H, sample=S)
    print(json.dumps(dict(leg="ratio", value="ransac_parent_loop / ransac_pairs", ratio=round(
        statistics.median(ms["ransac_parent_loop"]) / statistics.median(ms["ransac_pairs"]), 2))), flush=True)
    if args.no_register:
        return

    # ---- _register of the bench batch ----
    Bb = 64
    pairs = [synthetic.make_pair(args.points, seed=sd) for sd in sharding.pair_seeds(0, Bb)]
    clouds = [torch.from_numpy(p[0]).to(dev) for p in pairs] + [torch.from_numpy(p[1]).to(dev) for p in pairs]
    models = {}
    for case in ("none", "ransac"):
        cfg = get_config("3dmatch")
        cfg.update(dict(use_ransac=case == "ransac"))
        cfg.use_sinkhorn = False
        m = RegTR(cfg)
        synthetic.fill_parameters(m, seed=0)
        models[case] = m.to(dev).eval()
    with torch.no_grad():
        enc = models["none"].encode(clouds)
        src_lens, tgt_lens = enc.lens[:Bb], enc.lens[Bb:]
        segments = make_segments(src_lens, tgt_lens, dev)
        tok, xyz = enc.tokens, enc.points
    current = RegTR._refined_pose

    def former(self, *a_, **k_):          # the refinements as they stand, then RANSAC pair by pair as the parent ran it
        self.cfg.update(dict(use_ransac=False))
        try:
            out = current(self, *a_, **k_)
        finally:
            self.cfg.update(dict(use_ransac=True))
        out['pose'] = parent_ransac(out['src_pts'], out['tgt_pts'], out['val'], H, S)
        return out

    def run(case, route):
        RegTR._refined_pose = former if route == "parent" else current
        try:
            with torch.no_grad():
                return models[case]._register(tok, xyz, src_lens, tgt_lens, segments)
        finally:
            RegTR._refined_pose = current

    rlegs = [("none", "new"), ("ransac", "new"), ("ransac", "parent")]
    rms = {leg: [] for leg in rlegs}
    for _ in range(args.rounds):
        for leg in rlegs:
            rms[leg].append(timed(lambda: run(*leg), args.reps, args.warm))
    for case, route in rlegs:
        report(f"register_{case}_{route}", rms[(case, route)], pairs=Bb, tokens=int(tok.shape[0]),
               entries_per_pair=[min(src_lens), max(src_lens)])


if __name__ == "__main__":
    main()
