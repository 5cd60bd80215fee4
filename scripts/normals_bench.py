"""Times the normals subpackage on the bench batch: 64 pairs of 16 384 points (synthetic.make_pair, 128 clouds, 2.1 M
points).

  search          ops.radius_neighbors(points, points, r, limit) at its full width (no device-to-host read)
  kernel          normals.from_neighbors on that [N, limit] matrix (spr_estimate_normals alone), no viewpoint
  kernel_view     the same with one viewpoint per cloud and the curvature output
  search+kernel   the two back to back
  estimate        normals.estimate: the search at its exact width (one device-to-host read), then the kernel
  The kernel legs are set beside the byte count N * (kmax * 4 + kmax * 12 + 24) -- the row of indices, one 12-byte
  gather per column, the query point and the normal -- at the HBM rate and at the L2 rate of MI355X_MICROARCH.md.

  gather_rotate   normals.gather_rotate for C = 4, triple at column 1, rows = a shuffle inside every cloud (what
                  augment.augment_batch asks for), one rotation per cloud
  index_select    packed.index_select(0, rows): the path the augmentation takes without direction columns
  Both beside the bytes of one read and one write of every row plus the index.

Device events around --launches back-to-back launches, the legs alternating inside every repetition; one JSON line per
leg with median / min / max over the repetitions after warm-up.

    python scripts/normals_bench.py [--reps 7] [--pairs 64] [--radius 0.1] [--limit 40]
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

from superpoints_registration_amd import normals, ops, sharding, synthetic  # noqa: E402

HBM_TBS, L2_TBS = 6.3, 34.5          # achievable HBM3E rate and aggregate L2 rate


def _stats(ts):
    return dict(ms=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4), reps=len(ts))


def event_ms(fns, reps, launches, warm=2):
    """{name: [ms per launch]}: the legs alternate inside every repetition."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    names = list(fns)
    for rep in range(reps):
        for k in (names if rep % 2 == 0 else names[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fns[k]()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b) / launches)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--radius", type=float, default=0.1)
    ap.add_argument("--limit", type=int, default=40)
    args = ap.parse_args()
    assert args.reps >= 5, "the spread needs at least five repetitions"
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    dev = torch.device("cuda:0")
    pairs = [synthetic.make_pair(16384, seed=sd) for sd in sharding.pair_seeds(0, args.pairs)]
    clouds = [c for p in pairs for c in (p[0], p[1])]
    host = np.concatenate(clouds).astype(np.float32)
    lens = [len(c) for c in clouds]
    n, nb = len(host), len(lens)
    pts, cu = torch.from_numpy(host).to(dev), ops.lengths_to_cu(lens, dev)
    view = torch.from_numpy(np.stack([c.mean(0) + [0, 0, 5] for c in clouds]).astype(np.float32)).to(dev)
    r, limit = args.radius, args.limit

    def search():
        return ops.radius_neighbors(pts, pts, cu, cu, r, limit, exact_width=False)[0]
    nbr = search()
    valid = (nbr != n).sum(1)
    common = dict(points=n, clouds=nb, radius=r, limit=limit, mean_neighbours=round(float(valid.float().mean()), 2),
                  rows_at_the_limit=round(float((valid == limit).float().mean()), 4),
                  rows_below_3=int((valid < 3).sum()))
    legs = {"search": search,
            "kernel": lambda: normals.from_neighbors(pts, nbr),
            "kernel_view": lambda: normals.from_neighbors(pts, nbr, cu, view, curvature=True),
            "search+kernel": lambda: normals.from_neighbors(pts, search()),
            "estimate": lambda: normals.estimate(pts, cu, r, limit)}
    ts = event_ms(legs, args.reps, args.launches)
    nbytes = n * (limit * 4 + limit * 12 + 24)
    for k, t in ts.items():
        rec = dict(leg=k, **common, **_stats(t))
        if k.startswith("kernel"):
            ms = statistics.median(t)
            rec.update(bytes=nbytes, ms_at_hbm_rate=round(nbytes / (HBM_TBS * 1e12) * 1e3, 4),
                       ms_at_l2_rate=round(nbytes / (L2_TBS * 1e12) * 1e3, 4), tb_per_s=round(nbytes / (ms * 1e-3) / 1e12, 3))
        print(json.dumps(rec), flush=True)

    # ---- gather + rotate against index_select ---------------------------------------------------------------------------
    rng = np.random.default_rng(0)
    off = np.concatenate([[0], np.cumsum(lens)])
    rows = torch.from_numpy(np.concatenate([o + rng.permutation(m) for o, m in zip(off[:-1], lens)]).astype(np.int64)).to(dev)
    rows32 = rows.to(torch.int32)
    packed = torch.cat([torch.ones((n, 1), device=dev), normals.from_neighbors(pts, nbr)], dim=1)
    rot = torch.from_numpy(np.stack([synthetic.rotation_z(0.1 * b) for b in range(nb)]).astype(np.float32)).to(dev)
    legs = {"gather_rotate": lambda: normals.gather_rotate(packed, rows32, cu, rot, (1,)),
            "gather_rotate_int64_rows": lambda: normals.gather_rotate(packed, rows, cu, rot, (1,)),
            "gather_no_triples": lambda: normals.gather_rotate(packed, rows32, cu, rot, ()),
            "index_select": lambda: packed.index_select(0, rows)}
    ts = event_ms(legs, args.reps, args.launches)
    base = statistics.median(ts["index_select"])
    nbytes = n * (16 + 16 + 4)
    for k, t in ts.items():
        ms = statistics.median(t)
        print(json.dumps(dict(leg=k, rows=n, c=4, **_stats(t), over_index_select=round(ms / base, 4), bytes=nbytes,
                              tb_per_s=round(nbytes / (ms * 1e-3) / 1e12, 3))), flush=True)


if __name__ == "__main__":
    main()
