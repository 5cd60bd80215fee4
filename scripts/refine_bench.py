"""Times RegTR._register of the 64-pair bench batch (bench.py's pairs: 16 384-point box clouds, 3DMatch config) with the
refinement switches of the `lgr` and the `all` case of oracle.gen_golden.REFINE_CASES (use_sinkhorn off: the arg-max
correspondences carry the pose, as in the KITTI config), through
  * new     RegTR._refined_pose as it stands: one ops.refine_pairs call for all pairs;
  * parent  the per-pair loop it replaced (tests/test_gpu_refine.py keeps it as parent_loop), swapped in for
            _refined_pose in the same process, on the same encodings, in the same session;
and `none`: the same _register without any switch, for scale.  The clouds are encoded once (RegTR.encode); every leg
is timed with HIP events over --reps calls after --warm warm-up calls, legs interleaved --rounds times and the median
round reported.  "calls" counts what the refinement head hands the device per _register: ATen operators (a dispatch
mode counts them) plus library calls -- the launch count up to the few operators that launch twice or not at all.
One JSON line per leg.

    python scripts/refine_bench.py [--pairs 64] [--points 16384] [--reps 5] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle.gen_golden import REFINE_CASES  # noqa: E402
from superpoints_registration_amd import _lib, get_config, ops, sharding, synthetic  # noqa: E402
from superpoints_registration_amd.regtr import RegTR  # noqa: E402
from superpoints_registration_amd.transformers import make_segments  # noqa: E402
from test_gpu_refine import parent_loop  # noqa: E402


class CountOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        if not any(s in name for s in ("aten.view", "aten.slice", "aten.select", "aten.unsqueeze", "aten.detach",
                                       "aten.alias", "aten.expand", "aten.empty", "aten.as_strided", "aten.t.")):
            self.n += 1                                   # views and allocations launch nothing
        return func(*args, **(kwargs or {}))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B = args.pairs
    pairs = [synthetic.make_pair(args.points, seed=sd) for sd in sharding.pair_seeds(0, B)]
    clouds = [torch.from_numpy(p[0]).to(dev) for p in pairs] + [torch.from_numpy(p[1]).to(dev) for p in pairs]

    models = {}
    for case in ("none", "lgr", "all"):
        cfg = get_config("3dmatch")
        cfg.update(REFINE_CASES.get(case, {}))
        cfg.use_sinkhorn = False      # LGR over the unpruned Sinkhorn sets needs clouds of equal length
        m = RegTR(cfg)
        synthetic.fill_parameters(m, seed=0)
        models[case] = m.to(dev).eval()
    with torch.no_grad():
        enc = models["none"].encode(clouds)
        src_lens, tgt_lens = enc.lens[:B], enc.lens[B:]
        segments = make_segments(src_lens, tgt_lens, dev)
        tok, xyz = enc.tokens, enc.points                 # already laid out [src_0.., tgt_0..]

    lib_calls = [0]
    real_check = _lib.check

    def counting_check(rc, what):
        lib_calls[0] += 1
        return real_check(rc, what)

    def former(self, xyz_c, overlap, val, val2, ind, cu, cu_host, Bn, cond):
        return parent_loop(self.cfg, xyz_c, overlap, val, val2, ind, cu_host, Bn)

    legs = [("none", "new")] + [(c, r) for c in ("lgr", "all") for r in ("new", "parent")]
    current = RegTR._refined_pose

    def run(case, route):
        RegTR._refined_pose = former if route == "parent" else current
        try:
            with torch.no_grad():
                return models[case]._register(tok, xyz, src_lens, tgt_lens, segments)
        finally:
            RegTR._refined_pose = current

    ms = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg in legs:
            ms[leg].append(timed(lambda: run(*leg), args.reps, args.warm))
    for case, route in legs:
        _lib.check, lib_calls[0] = counting_check, 0
        ops._lib.check = counting_check
        with CountOps() as c:
            out = run(case, route)
        _lib.check = ops._lib.check = real_check
        torch.cuda.synchronize()
        print(json.dumps(dict(leg=f"register_{case}_{route}", ms=round(statistics.median(ms[(case, route)]), 3),
                              rounds=[round(x, 3) for x in ms[(case, route)]], pairs=B,
                              tokens=int(tok.shape[0]), calls=c.n + lib_calls[0],
                              pose_t0=[round(float(x), 5) for x in out["pose"][0, :, 3]])), flush=True)


if __name__ == "__main__":
    main()
