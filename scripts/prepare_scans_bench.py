"""Times the KITTI loader's point path (kitti_pred.py:203-230: first-point voxel filter, crop, ground cut) for the raw
scans of a batch through
  * per_cloud   the route the library offered before: for every scan ops.voxel_downsample (three kernels between two
                rocPRIM radix sorts, one device->host read of the count) and torch masks in float64;
  * batched     ops.prepare_scans: all scans in one call (one memset, five launches, one device->host copy);
  * prepare_pairs  kitti.prepare_pairs on the lists of scans: the concatenation, ops.prepare_scans, the split into
                views;
on --pairs pairs of synthetic ring-shaped scans (64 beams x 1 875 azimuth steps = 120 000 returns: ground rings out
to where a beam meets the ground, facades in between), 4 columns like the raw Velodyne records, voxel --voxel, with
crop_radius 0 and --crop.  Both routes run in one process on the same device tensors; their outputs are compared bit
for bit before anything is timed.  Every leg is timed with HIP events over --reps calls after --warm warm-up calls,
legs interleaved --rounds times, the median round reported.  One JSON line per leg.

    python scripts/prepare_scans_bench.py [--pairs 64] [--voxel 0.3] [--crop 50] [--reps 10] [--rounds 5]
                                          [--only batched]
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

from superpoints_registration_amd import get_config, kitti, ops  # noqa: E402

BEAMS, STEPS = 64, 1875


def ring_scan(seed: int) -> np.ndarray:
    """[120 000, 4] float32, x y z reflectance, in the order a spinning sensor writes them (azimuth major)."""
    rng = np.random.default_rng(seed)
    elev = np.deg2rad(np.linspace(2.0, -24.8, BEAMS))
    az = np.linspace(0.0, 2 * np.pi, STEPS, endpoint=False)
    # facades: piecewise-constant distance over 48 sectors, 8 .. 70 m
    wall = rng.uniform(8.0, 70.0, 48)[(az / (2 * np.pi) * 48).astype(int)]
    a, e = np.meshgrid(az, elev, indexing="ij")
    w = np.broadcast_to(wall[:, None], a.shape)
    ground = np.where(e < 0, 1.73 / np.tan(np.maximum(-e, 1e-3)), np.inf)
    rng_m = np.minimum(ground, w / np.cos(e)) + rng.normal(0.0, 0.02, a.shape)
    xyz = np.stack([rng_m * np.cos(e) * np.cos(a), rng_m * np.cos(e) * np.sin(a), rng_m * np.sin(e)], -1)
    refl = rng.uniform(0.0, 1.0, a.shape + (1,))
    return np.concatenate([xyz, refl], -1).reshape(-1, 4).astype(np.float32)


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


def per_cloud(scans, voxel, crop, ground):
    out = []
    for s in scans:
        v = ops.voxel_downsample(s[:, :3], voxel)
        d = v.double()
        if crop > 0:
            keep = torch.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2) <= crop
            v, d = v[keep], d[keep]
        if ground:
            v = v[d[:, 2] > -1]
        out.append(v)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--voxel", type=float, default=0.3)
    ap.add_argument("--crop", type=float, default=50.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["batched", "per_cloud", "prepare_pairs"], default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    scans = [torch.from_numpy(ring_scan(1000 + i)).to(dev) for i in range(2 * args.pairs)]
    lens = [int(s.shape[0]) for s in scans]
    packed, cu = torch.cat(scans), ops.lengths_to_cu(lens, dev)

    for crop, ground in ((0.0, False), (args.crop, False), (args.crop, True)):
        xyz, out_cu, _ = ops.prepare_scans(packed, cu, args.voxel, crop, ground)
        loop = per_cloud(scans, args.voxel, crop, ground)
        same = torch.equal(xyz, torch.cat(loop)) and out_cu[1:] == np.cumsum([len(v) for v in loop]).tolist()
        print(json.dumps(dict(leg="outputs_equal", crop_radius=crop, remove_ground=ground, equal=bool(same),
                              points_in=sum(lens), points_out=out_cu[-1])), flush=True)
        if not same:
            raise SystemExit("the two routes disagree")

    for crop in (0.0, args.crop):
        cfg = get_config('kitti', first_subsampling_dl=args.voxel, crop_radius=crop)
        legs = {"per_cloud": lambda: per_cloud(scans, args.voxel, crop, False),
                "batched": lambda: ops.prepare_scans(packed, cu, args.voxel, crop, False),
                "prepare_pairs": lambda: kitti.prepare_pairs(scans[:args.pairs], scans[args.pairs:], cfg)}
        if args.only:
            legs = {args.only: legs[args.only]}
        ms = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, fn in legs.items():
                ms[k].append(timed(fn, args.reps, args.warm))
        for k in legs:
            report(k, ms[k], scans=len(scans), points=sum(lens), voxel=args.voxel, crop_radius=crop)
        if not args.only:
            print(json.dumps(dict(leg="ratio", value="per_cloud / batched", crop_radius=crop, ratio=round(
                statistics.median(ms["per_cloud"]) / statistics.median(ms["batched"]), 2))), flush=True)


if __name__ == "__main__":
    main()
