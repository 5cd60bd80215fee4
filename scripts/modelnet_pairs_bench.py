"""Times the ModelNet pair generator (modelnet.make_pairs -> modelnet.modelnet_pairs: csrc/modelnet_pairs.hip) on 256
raw shapes of 2048 points -> 256 pairs of 717 + 717 points (get_config('modelnet'): partial [0.7, 0.7], rot_mag 45,
trans_mag 0.5),
  (a) make_pairs, the Python entry point (host draws of the decisions, list concatenation, one device-to-host read);
  (b) modelnet_pairs alone, the library call on packed tensors with the decisions already drawn;
  (c) for context, the numpy float64 replica of the same chain (tests/modelnet_replica.py: Philox draws and the apply
      contract) on the host CPUs, per pair as a loader worker would run it, on the first --host-pairs shapes.
HIP events around every device call, warm-up, median / min / max of the repeats; one JSON line per result, written to
--out as well.

    python scripts/modelnet_pairs_bench.py [--reps 20] [--out profiles/modelnet_pairs_bench.txt]
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
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import modelnet_replica as mr  # noqa: E402
from superpoints_registration_amd import get_config, modelnet, ops  # noqa: E402

HEADER = """ModelNet pair generator (csrc/modelnet_pairs.hip), MI355X, scripts/modelnet_pairs_bench.py
HIP events around every call, 3 warm-up calls, median / min / max of {reps}.  get_config('modelnet'): partial [0.7, 0.7],
rot_mag 45, trans_mag 0.5, jitter 0.01 clipped at 0.05; {pairs} raw shapes of {n} points -> pairs of 717 + 717 points.
make_pairs is the Python entry point (host draws of the decisions, concatenation, one device-to-host read included);
modelnet_pairs is the library call alone.  host_numpy_replica is the float64 numpy restatement of the same chain
(tests/modelnet_replica.py), one pair after the other on the host.
"""


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


def shape(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True) * (0.5 + 0.4 * rng.random((n, 1)))).astype(np.float32)


def host_pair(x, cfg, seed, key, k):
    """One pair on the host: the draws (numpy Philox; float64 Box-Muller for the noise) and the apply contract."""
    n, p = x.shape[0], float(cfg.partial[0])
    dirs, tf = mr.decide(seed, key, cfg.rot_mag, cfg.trans_mag)
    rk = [mr.resample_keys(seed, key, s, n) for s in range(2)]
    ex = [mr.extra_words(seed, key, s, k) for s in range(2)]
    sk = [mr.shuffle_keys(seed, key, s, k) for s in range(2)]
    nz = [mr.noise64(seed, key, s, k)[0].astype(np.float32) for s in range(2)]
    q = mr.percentile_q(p)
    return mr.make_pair(x, (p, p), (q, q), k, modelnet.JITTER_SCALE, modelnet.JITTER_CLIP, tf, dirs, rk, ex, nz, sk)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--host-pairs", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "modelnet_pairs_bench.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = get_config("modelnet")
    nb, n, seed = args.pairs, args.points, 1
    k = modelnet.output_size(cfg)
    host = [shape(n, 1000 + b) for b in range(nb)]
    points = torch.from_numpy(np.stack(host)).to(dev)
    keys = list(range(nb))
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    med, lo, hi = timed(lambda: modelnet.make_pairs(points, cfg, seed, keys), args.reps)
    out = modelnet.make_pairs(points, cfg, seed, keys)
    emit(leg="make_pairs", pairs=nb, points_in=nb * n, points_out=2 * nb * k, ms=round(med, 4), ms_min=round(lo, 4),
         ms_max=round(hi, 4), correspondences=int(sum(c.shape[1] for c in out["correspondences"])))

    xyz, cu = points.reshape(-1, 3).contiguous(), ops.lengths_to_cu([n] * nb, dev)
    dirs, tf = modelnet.modelnet_draw(seed, keys, cfg.rot_mag, cfg.trans_mag)
    dirs_d, tf_d = torch.from_numpy(dirs).to(dev), torch.from_numpy(tf).to(dev)
    p = (float(cfg.partial[0]),) * 2
    med, lo, hi = timed(lambda: modelnet.modelnet_pairs(xyz, cu, n, p, k, tf_d, dirs_d, seed=seed, pair_keys=keys), args.reps)
    emit(leg="modelnet_pairs", pairs=nb, points_in=nb * n, points_out=2 * nb * k, ms=round(med, 4), ms_min=round(lo, 4),
         ms_max=round(hi, 4))

    m = min(args.host_pairs, nb)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        for b in range(m):
            host_pair(host[b], cfg, seed, keys[b], k)
        ts.append((time.perf_counter() - t0) * 1e3)
    emit(leg="host_numpy_replica", pairs=m, ms=round(statistics.median(ts), 3), ms_min=round(min(ts), 3),
         ms_max=round(max(ts), 3), ms_per_pair=round(statistics.median(ts) / m, 4),
         ms_scaled_to_all_pairs=round(statistics.median(ts) / m * nb, 2))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(HEADER.format(reps=args.reps, pairs=nb, n=n) + "\n" + "\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
