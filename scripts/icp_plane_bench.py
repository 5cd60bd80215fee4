"""Times point-to-plane ICP for all pairs in one call (icp_plane.icp_pairs: csrc/icp.hip) on the batch of
scripts/icp_bench.py -- 64 pairs of synthetic.make_lidar_pair(120000, voxel=0.02) scans, max_dist 0.2, the ground-truth
pose moved by 0.3 degrees and 5 cm -- with target normals from normals.estimate (radius 0.5, 40 neighbours, facing the
sensor), against point-to-point ICP from the same starts and against the same point-to-plane loop composed from the
operators the library had before: per iteration one ops.gt_overlap for the association, torch for the residuals and
the 6 x 6 normal equations (index_add_ per pair), the solve and the pose update on the host.  Legs, one JSON line each:
  normals            the target normals of the batch (one search, one kernel): paid once, outside the legs below
  evaluate           icp_plane with max_iter = 0: the table build and one association pass
  fixed_passes       max_iter = 8 with the convergence test off (rel = -1): per pass = (this - evaluate) / 8
  fixed_passes_p2p   the same for icp.icp_pairs, in the same run: the per-pass cost beside it
  plane_l2 / plane_huber / plane_tukey   the call as a user would make it (rel 1e-6, max_iter 200); passes per pair
  p2p                icp.icp_pairs under the same rule from the same starts
  composed           the composed point-to-plane loop (L2) under the same stopping rule
HIP events around every call, warm-up, median of the repeats.

    python scripts/icp_plane_bench.py [--pairs 64] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from icp_bench import perturbed, timed  # noqa: E402
from superpoints_registration_amd import icp, icp_plane, ops, synthetic  # noqa: E402

MAX_DIST, MAX_ITER, REL, RADIUS, LIMIT, KERNEL_K = 0.2, 200, 1e-6, 0.5, 40, 0.05


def euler_step(x, c):
    """U [3, 4] of the contract (spr.h): Rz Ry Rx and t = v - omega x c, float64 on the host."""
    sx, cx, sy, cy, sz, cz = np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]), np.sin(x[2]), np.cos(x[2])
    R = np.array([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
                  [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx], [-sy, cy * sx, cy * cx]])
    return np.hstack([R, (x[3:] - np.cross(x[:3], c))[:, None]])


def composed_plane(src, src_cu, tgt, nrm, tgt_cu, pair_of_src, n_src, pose0, max_dist, max_iter, rel):
    """The point-to-plane loop from ops.gt_overlap + torch, L2 kernel; every pair iterates until all have stopped."""
    nb = len(n_src)
    tgt_off = tgt_cu[:-1].long()[pair_of_src]
    c = torch.stack([tgt[a:b].double().amin(0) for a, b in zip(tgt_cu[:-1].tolist(), tgt_cu[1:].tolist())])
    pose = pose0.clone()                                                      # float64 [B, 3, 4] on the device
    prev = None
    for k in range(max_iter + 1):
        src_corr, _, src_mask, _, _, _ = ops.gt_overlap(src, src_cu, tgt, tgt_cu, pose.float(), max_dist)
        w = src_mask.double()
        j = tgt_off + src_corr.clamp(min=0).long()
        b, n = tgt[j].double(), nrm[j].double()
        R, t = pose[pair_of_src, :, :3], pose[pair_of_src, :, 3]
        a = (R * src[:, None, :].double()).sum(2) + t
        e = a - b
        J = torch.cat([torch.linalg.cross(a - c[pair_of_src], n), n], 1) * w[:, None]
        r = (e * n).sum(1)
        rows = torch.cat([(J[:, :, None] * J[:, None, :]).reshape(-1, 36), J * r[:, None], w[:, None],
                          ((e * e).sum(1) * w)[:, None]], 1)
        S = torch.zeros((nb, 44), dtype=torch.float64, device=src.device).index_add_(0, pair_of_src, rows).cpu().numpy()
        count, sq = S[:, 42], S[:, 43]
        now = np.stack([count / n_src, np.sqrt(sq / np.maximum(count, 1))])    # the host check of this iteration
        if k == max_iter or (prev is not None and bool((np.abs(now - prev) < rel).all())):
            return pose, now[0], now[1], k
        prev = now
        x = np.linalg.solve(S[:, :36].reshape(nb, 6, 6), -S[:, 36:42, None])[:, :, 0]
        P = pose.cpu().numpy()
        cc = c.cpu().numpy()
        new = []
        for p, xi, ci in zip(P, x, cc):
            U = euler_step(xi, ci)
            new.append(np.hstack([U[:, :3] @ p[:, :3], (U[:, :3] @ p[:, 3] + U[:, 3])[:, None]]))
        pose = torch.from_numpy(np.stack(new)).to(src.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    T = torch.from_numpy
    rng = np.random.default_rng(0)
    pairs = [synthetic.make_lidar_pair(120000, seed=sd, voxel=0.02) for sd in range(args.pairs)]
    src_l, tgt_l = [T(p[0]).to(dev) for p in pairs], [T(p[1]).to(dev) for p in pairs]
    init = np.stack([perturbed(p[2], rng) for p in pairs])
    pose64 = T(init).to(dev)
    gt = T(np.stack([p[2] for p in pairs]).astype(np.float64)).to(dev)
    points = sum(len(p[0]) + len(p[1]) for p in pairs)
    base = dict(pairs=len(pairs), points=points, max_dist=MAX_DIST)

    def line(leg, t, **kw):
        print(json.dumps(dict(leg=leg, **base, ms=round(t[0], 3), ms_min=round(t[1], 3), ms_max=round(t[2], 3), **kw)),
              flush=True)

    view = torch.zeros((len(pairs), 3), dtype=torch.float32, device=dev)
    t_nrm = timed(lambda: icp_plane.estimate_target_normals(tgt_l, RADIUS, LIMIT, view), max(2, args.reps // 2), warm=1)
    nrm_l = icp_plane.estimate_target_normals(tgt_l, RADIUS, LIMIT, view)
    line("normals", t_nrm, radius=RADIUS, limit=LIMIT,
         zero_share=round(float((torch.cat(nrm_l).abs().amax(1) == 0).double().mean()), 5))

    def plane(max_iter=MAX_ITER, rel=REL, kernel="l2"):
        return icp_plane.icp_pairs(src_l, tgt_l, nrm_l, pose64, MAX_DIST, max_iter, rel, rel, kernel=kernel,
                                   kernel_k=None if kernel == "l2" else KERNEL_K)

    def p2p(max_iter=MAX_ITER, rel=REL):
        return icp.icp_pairs(src_l, tgt_l, pose64, MAX_DIST, max_iter, rel, rel)

    def summary(r):
        passes = (r['iterations'] + 1).tolist()
        return dict(passes_min=min(passes), passes_max=max(passes), passes_sum=sum(passes),
                    fitness=round(float(r['fitness'].mean()), 4), rmse=round(float(r['inlier_rmse'].mean()), 5),
                    pose_err=round(float((r['pose64'] - gt).abs().amax()), 5),
                    pose_err_median=round(float((r['pose64'] - gt).abs().amax((1, 2)).median()), 5))

    t_eval = timed(lambda: plane(0), args.reps)
    line("evaluate", t_eval, pose_err_init=round(float((pose64 - gt).abs().amax()), 5))
    t_fix = timed(lambda: plane(8, -1.0), args.reps)
    line("fixed_passes", t_fix, passes=9, ms_per_pass=round((t_fix[0] - t_eval[0]) / 8, 3))
    t_eval_p = timed(lambda: p2p(0), args.reps)
    t_fix_p = timed(lambda: p2p(8, -1.0), args.reps)
    line("fixed_passes_p2p", t_fix_p, passes=9, ms_evaluate=round(t_eval_p[0], 3),
         ms_per_pass=round((t_fix_p[0] - t_eval_p[0]) / 8, 3))
    t_full = None
    for kernel in ("l2", "huber", "tukey"):
        t = timed(lambda: plane(kernel=kernel), args.reps)
        t_full = t if kernel == "l2" else t_full
        line("plane_" + kernel, t, **summary(plane(kernel=kernel)), **({} if kernel == "l2" else dict(kernel_k=KERNEL_K)))
    t_p = timed(p2p, args.reps)
    line("p2p", t_p, **summary(p2p()), plane_l2_over_p2p=round(t_full[0] / t_p[0], 3))

    src, tgt, nrm = torch.cat(src_l), torch.cat(tgt_l), torch.cat(nrm_l)
    s_lens, t_lens = [len(p[0]) for p in pairs], [len(p[1]) for p in pairs]
    src_cu, tgt_cu = ops.lengths_to_cu(s_lens, dev), ops.lengths_to_cu(t_lens, dev)
    pair_of_src = torch.repeat_interleave(torch.arange(len(pairs), device=dev), torch.tensor(s_lens, device=dev))
    n_src = np.asarray(s_lens, dtype=np.float64)

    def composed():
        return composed_plane(src, src_cu, tgt, nrm, tgt_cu, pair_of_src, n_src, pose64, MAX_DIST, MAX_ITER, REL)

    t_comp = timed(composed, max(2, args.reps // 2), warm=1)
    cp, cfit, crmse, ck = composed()
    line("composed", t_comp, passes=ck + 1, ms_per_pass=round(t_comp[0] / (ck + 1), 3), fitness=round(float(cfit.mean()), 4),
         rmse=round(float(crmse.mean()), 5), pose_err=round(float((cp - gt).abs().amax()), 5),
         composed_over_call=round(t_comp[0] / t_full[0], 2))


if __name__ == "__main__":
    main()
