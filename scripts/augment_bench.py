"""Times the training augmentation (augment.augment_batch -> ops.augment_pairs: csrc/augment.hip) on 16 and on 64
pairs of 16 384 points (synthetic.make_pair, the 3DMatch config: perturb_pose small, augment_noise 0.005),
  (a) with labels (masks + correspondences from overlap.label_batch) and without, beside label_batch on the same pairs;
  (b) unless --skip-model, one Trainer.train_step of RegTR on 16 labelled pairs with augment=True against augment=False
      (the step as it was before the operator existed), alternating, with the spread of each;
  (c) for context, the same four transforms restated in torch on the host CPUs, per pair (this script's own code).
HIP events around every device call, warm-up, median of the repeats; one JSON line per result.

    python scripts/augment_bench.py [--skip-model] [--reps 20]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/augment_bench.py --profile-only
(--profile-only: five labelled 64-pair calls and nothing else, for the per-launch breakdown.)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from superpoints_registration_amd import augment, get_config, overlap, sharding, synthetic  # noqa: E402


def timed(fn, reps, warm=3):
    """Median (and min / max) of per-call device-event times in ms."""
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
    return statistics.median(ts), min(ts), max(ts)


def host_transforms(pair, mask, corr, scale, max_pts, gen):
    """RigidPerturb(small) -> Jitter -> ShufflePoints -> RandomSwap of one pair in torch on the CPU."""
    src, tgt, pose = pair
    ang = torch.randn(3, generator=gen) * 0.1
    K = torch.tensor([[0, -ang[2], ang[1]], [ang[2], 0, -ang[0]], [-ang[1], ang[0], 0]])
    R = torch.linalg.matrix_exp(K)
    t = torch.randn(3, generator=gen) * 0.1 / 3 ** 0.5
    c = src.mean(0)
    t = t + c - R @ c
    src = src @ R.T + t
    Rp, tp = pose[:, :3] @ R.T, pose[:, 3] - pose[:, :3] @ R.T @ t
    src = src + torch.randn(src.shape, generator=gen) * scale
    tgt = tgt + torch.randn(tgt.shape, generator=gen) * scale
    si, ti = torch.randperm(src.shape[0], generator=gen)[:max_pts], torch.randperm(tgt.shape[0], generator=gen)[:max_pts]
    srev, trev = torch.full((src.shape[0],), -1, dtype=torch.long), torch.full((tgt.shape[0],), -1, dtype=torch.long)
    srev[si], trev[ti] = torch.arange(si.shape[0]), torch.arange(ti.shape[0])
    corr = torch.stack([srev[corr[0]], trev[corr[1]]])
    corr = corr[:, (corr >= 0).all(0)]
    src, tgt, ms, mt = src[si], tgt[ti], mask[0][si], mask[1][ti]
    if float(torch.rand((), generator=gen)) > 0.5:
        src, tgt, ms, mt, corr = tgt, src, mt, ms, corr.flip(0)
        Rp, tp = Rp.T, -Rp.T @ tp
    return src, tgt, torch.cat([Rp, tp[:, None]], 1), ms, mt, corr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--profile-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    T = torch.from_numpy
    cfg = get_config("3dmatch")
    pairs = [synthetic.make_pair(16384, seed=sd) for sd in sharding.pair_seeds(0, 64)]

    def raw(n):
        return {"src_xyz": [T(p[0]).to(dev) for p in pairs[:n]], "tgt_xyz": [T(p[1]).to(dev) for p in pairs[:n]],
                "pose": T(np.stack([p[2] for p in pairs[:n]]).astype(np.float32)).to(dev)}

    for n in (64, 16):
        plain = raw(n)
        labelled = overlap.label_batch(raw(n), cfg.overlap_radius)
        keys = list(range(n))
        if args.profile_only:
            if n == 64:
                for i in range(5):
                    augment.augment_batch(labelled, cfg, 1, [k + 100 * i for k in keys])
                torch.cuda.synchronize()
            continue
        lab_ms = timed(lambda: overlap.label_batch({k: plain[k] for k in ("src_xyz", "tgt_xyz", "pose")},
                                                   cfg.overlap_radius), args.reps)
        for tag, batch in (("labelled", labelled), ("unlabelled", plain)):
            med, lo, hi = timed(lambda: augment.augment_batch(batch, cfg, 1, keys), args.reps)
            out = augment.augment_batch(batch, cfg, 1, keys)
            print(json.dumps(dict(leg="augment_batch", pairs=n, points=n * 2 * 16384, labels=tag, ms=round(med, 4),
                                  ms_min=round(lo, 4), ms_max=round(hi, 4), label_batch_ms=round(lab_ms[0], 4),
                                  correspondences=int(sum(c.shape[1] for c in out.get("correspondences", []))))),
                  flush=True)
    if args.profile_only:
        return

    # (c) the same transforms on the host CPUs, per pair as a loader worker would run them
    cpu = overlap.label_batch(raw(16), cfg.overlap_radius)
    host = [((cpu["src_xyz"][b].cpu(), cpu["tgt_xyz"][b].cpu(), cpu["pose"][b].cpu()),
             (cpu["src_overlap"][b].cpu(), cpu["tgt_overlap"][b].cpu()), cpu["correspondences"][b].cpu()) for b in range(16)]
    gen = torch.Generator().manual_seed(0)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        for pair, mask, corr in host:
            host_transforms(pair, mask, corr, cfg.augment_noise, 30000, gen)
        ts.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(leg="host_torch_transforms", pairs=16, threads=torch.get_num_threads(),
                          ms=round(statistics.median(ts), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3))),
          flush=True)
    if args.skip_model:
        return

    # (b) the consumer: one training step on 16 labelled pairs, augmentation on against off, alternating
    from superpoints_registration_amd.regtr import RegTR
    from superpoints_registration_amd.training import Trainer
    batch = overlap.label_batch(raw(16), cfg.overlap_radius)
    times = {False: [], True: []}
    trainers = {}
    for aug in (False, True):
        model = RegTR(cfg)
        synthetic.fill_parameters(model, seed=0)
        model = model.to(dev)
        trainers[aug] = (Trainer(cfg, augment=aug, seed=1).setup(model), model)
        for _ in range(2):
            trainers[aug][0].train_step(model, dict(batch))
    torch.cuda.synchronize()
    for _ in range(6):
        for aug in (False, True):
            tr, model = trainers[aug]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            tr.train_step(model, dict(batch))
            b.record()
            torch.cuda.synchronize()
            times[aug].append(a.elapsed_time(b))
    off, on = statistics.median(times[False]), statistics.median(times[True])
    print(json.dumps(dict(leg="train_step", pairs=16, augment_off_ms=round(off, 2),
                          augment_off_min_max=[round(min(times[False]), 2), round(max(times[False]), 2)],
                          augment_on_ms=round(on, 2),
                          augment_on_min_max=[round(min(times[True]), 2), round(max(times[True]), 2)],
                          difference_ms=round(on - off, 2))), flush=True)


if __name__ == "__main__":
    main()
