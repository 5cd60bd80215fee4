"""Times ICP for all pairs in one call (icp.icp_pairs: csrc/icp.hip) on 64 pairs of KITTI-sized synthetic scans
(synthetic.make_lidar_pair(120000, voxel=0.02): about 120 000 points each, as good as un-voxelised) at max_dist 0.2,
from the ground-truth pose perturbed by 0.3 degrees and 5 cm, against the same loop composed from the operators the
library had before: per iteration one ops.gt_overlap (both clouds' cell table rebuilt, both directions searched), torch
glue for fitness and RMSE, one ops.weighted_procrustes_raw over the matched points, and one host check of the
convergence test.  Legs, one JSON line each:
  evaluate      icp.evaluate: the table build and one association pass
  fixed_passes  icp_pairs with the convergence test off (rel = -1) and max_iter = 8: per pass = (this - evaluate) / 8
  fixed_passes_cell_order  the same with every source cloud re-ordered by the 0.25 m cell of its moved points (the
                synthetic scans come in random point order, the worst case for the walk; a real scan comes in
                sensor order)
  icp_pairs     the call as the loader would make it (rel 1e-6, max_iter 200), passes made per pair
  gt_overlap    one ops.gt_overlap on the batch: the search of one iteration of the composed loop
  composed      the composed loop under the same stopping rule
HIP events around every call, warm-up, median of the repeats.

    python scripts/icp_bench.py [--pairs 64] [--reps 5]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/icp_bench.py --profile-only
(--profile-only: three icp_pairs calls and nothing else, for the kernel breakdown.)
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

from superpoints_registration_amd import icp, ops, synthetic  # noqa: E402

MAX_DIST, MAX_ITER, REL = 0.2, 200, 1e-6


def timed(fn, reps, warm=2):
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


def perturbed(pose, rng):
    """pose [3,4] composed with a rotation of 0.3 degrees about a random axis and 5 cm."""
    k = rng.normal(size=3)
    k /= np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = np.deg2rad(0.3)
    dR = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    dt = rng.normal(size=3)
    dt *= 0.05 / np.linalg.norm(dt)
    p = pose.astype(np.float64)
    return np.hstack([dR @ p[:, :3], (dR @ p[:, 3] + dt)[:, None]])


def composed_icp(src, src_cu, tgt, tgt_cu, pair_of_src, n_src, pose0, max_dist, max_iter, rel):
    """The same loop from ops.gt_overlap + ops.weighted_procrustes_raw, float32 poses, one host check per iteration
    (every pair iterates until all have stopped: the operators have no per-pair switch)."""
    cu = src_cu.long()
    pose = pose0.clone()
    tgt_off = tgt_cu[:-1].long()[pair_of_src]
    prev = None
    for k in range(max_iter + 1):
        src_corr, _, src_mask, _, _, _ = ops.gt_overlap(src, src_cu, tgt, tgt_cu, pose, max_dist)
        w = src_mask.to(torch.float32)
        partner = tgt[(tgt_off + src_corr.clamp(min=0).long())]
        R, t = pose[pair_of_src, :, :3], pose[pair_of_src, :, 3]
        moved = (R * src[:, None, :]).sum(2) + t
        d2 = ((moved - partner) ** 2).sum(1) * w
        run = torch.nn.functional.pad(torch.cumsum(torch.stack([w.double(), d2.double()]), 1), (1, 0))
        count, sq = (run[:, cu[1:]] - run[:, cu[:-1]]).unbind(0)              # per-pair sums without atomics
        fit, rmse = count / n_src, torch.sqrt(sq / count.clamp(min=1))
        now = torch.stack([fit, rmse]).cpu()                                  # the host check of this iteration
        if k == max_iter or (prev is not None and bool(((now - prev).abs() < rel).all())):
            return pose, fit, rmse, k
        prev = now
        pose = ops.weighted_procrustes_raw(src, partner, w, src_cu)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    T = torch.from_numpy
    rng = np.random.default_rng(0)
    pairs = [synthetic.make_lidar_pair(120000, seed=sd, voxel=0.02) for sd in range(args.pairs)]
    src_l, tgt_l = [T(p[0]).to(dev) for p in pairs], [T(p[1]).to(dev) for p in pairs]
    init = np.stack([perturbed(p[2], rng) for p in pairs])
    pose64 = T(init).to(dev)
    points = sum(len(p[0]) + len(p[1]) for p in pairs)

    def full():
        return icp.icp_pairs(src_l, tgt_l, pose64, MAX_DIST, MAX_ITER, REL, REL)

    if args.profile_only:
        for _ in range(3):
            full()
        torch.cuda.synchronize()
        return
    base = dict(pairs=len(pairs), points=points, max_dist=MAX_DIST)

    def line(leg, t, **kw):
        print(json.dumps(dict(leg=leg, **base, ms=round(t[0], 3), ms_min=round(t[1], 3), ms_max=round(t[2], 3), **kw)),
              flush=True)

    t_eval = timed(lambda: icp.evaluate(src_l, tgt_l, pose64, MAX_DIST), args.reps)
    ev = icp.evaluate(src_l, tgt_l, pose64, MAX_DIST)
    line("evaluate", t_eval, fitness=round(float(ev['fitness'].mean()), 4), rmse=round(float(ev['inlier_rmse'].mean()), 5))
    t_fix = timed(lambda: icp.icp_pairs(src_l, tgt_l, pose64, MAX_DIST, 8, -1.0, -1.0), args.reps)
    line("fixed_passes", t_fix, passes=9, ms_per_pass=round((t_fix[0] - t_eval[0]) / 8, 3))
    order = []
    for p, T0 in zip(pairs, init):                       # by the cell of the moved point, x fastest: the table's order
        c = np.floor((p[0].astype(np.float64) @ T0[:, :3].T + T0[:, 3]) / 0.25).astype(np.int64)
        order.append(np.lexsort((c[:, 0], c[:, 1], c[:, 2])))
    src_sorted = [T(p[0][o]).to(dev) for p, o in zip(pairs, order)]
    t_sort = timed(lambda: icp.icp_pairs(src_sorted, tgt_l, pose64, MAX_DIST, 8, -1.0, -1.0), args.reps)
    t_eval_s = timed(lambda: icp.evaluate(src_sorted, tgt_l, pose64, MAX_DIST), args.reps)
    line("fixed_passes_cell_order", t_sort, passes=9, ms_per_pass=round((t_sort[0] - t_eval_s[0]) / 8, 3))
    del src_sorted
    t_full = timed(full, args.reps)
    r = full()
    gt = T(np.stack([p[2] for p in pairs]).astype(np.float64)).to(dev)
    passes = (r['iterations'] + 1).tolist()
    line("icp_pairs", t_full, passes_min=min(passes), passes_max=max(passes), passes_sum=sum(passes),
         fitness=round(float(r['fitness'].mean()), 4), rmse=round(float(r['inlier_rmse'].mean()), 5),
         pose_err_init=round(float((pose64 - gt).abs().amax()), 5), pose_err=round(float((r['pose64'] - gt).abs().amax()), 5))

    src, tgt = torch.cat(src_l), torch.cat(tgt_l)
    s_lens, t_lens = [len(p[0]) for p in pairs], [len(p[1]) for p in pairs]
    src_cu, tgt_cu = ops.lengths_to_cu(s_lens, dev), ops.lengths_to_cu(t_lens, dev)
    pair_of_src = torch.repeat_interleave(torch.arange(len(pairs), device=dev), torch.tensor(s_lens, device=dev))
    n_src = torch.tensor(s_lens, dtype=torch.float64, device=dev)
    pose32 = pose64.to(torch.float32)

    def composed():
        return composed_icp(src, src_cu, tgt, tgt_cu, pair_of_src, n_src, pose32, MAX_DIST, MAX_ITER, REL)

    t_ov = timed(lambda: ops.gt_overlap(src, src_cu, tgt, tgt_cu, pose32, MAX_DIST), args.reps)
    line("gt_overlap", t_ov)
    t_comp = timed(composed, max(2, args.reps // 2), warm=1)
    cp, cfit, crmse, ck = composed()
    line("composed", t_comp, passes=ck + 1, ms_per_pass=round(t_comp[0] / (ck + 1), 3),
         fitness=round(float(cfit.mean()), 4), rmse=round(float(crmse.mean()), 5),
         pose_err=round(float((cp.double() - gt).abs().amax()), 5), composed_over_call=round(t_comp[0] / t_full[0], 2))


if __name__ == "__main__":
    main()
