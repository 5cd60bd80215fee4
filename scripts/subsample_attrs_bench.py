"""Times grid subsampling with and without attributes on the level-0 points of the bench batch: 64 pairs of 16 384
points (synthetic.make_pair, 128 clouds, 2.1 M points), first_subsampling_dl of the 3DMatch config, reference order.

  plain        spr_grid_subsample of this build and, with --parent-lib, of a library built from the parent commit,
               alternating inside every repetition; whether the two outputs are the same bits
  attrs        spr_grid_subsample_attrs at fdim 3 / ldim 1 and at fdim 32 / ldim 0: time, time over the plain call, and
               achieved bytes/s against the algorithmic bytes (inputs read once, outputs written once)
  replica      the numpy restatement (tests/subsample_attrs_replica.py) on the same input, host time, once

Device events around --launches back-to-back launches; one JSON line per leg with median / min / max over the
repetitions after warm-up.  The first attrs call with labels measures the bucket schedule on the host; it falls in the
warm-up.

    python scripts/subsample_attrs_bench.py [--reps 7] [--pairs 64] [--parent-lib PATH] [--skip-replica]
"""
import argparse
import ctypes
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

from superpoints_registration_amd import _lib, get_config, ops, sharding, synthetic  # noqa: E402


def _stats(ts):
    return dict(ms=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4), reps=len(ts))


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bind(lib, name):
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return fn


class Call:
    """One entry point on fixed buffers.  fdim = ldim = None: the plain call of `lib`."""

    def __init__(self, lib, pts, cu, dl, feat=None, lab=None, plain=False):
        n, nb, dev = pts.shape[0], cu.numel() - 1, pts.device
        self.n, self.nb, self.pts, self.cu, self.dl, self.feat, self.lab, self.plain = n, nb, pts, cu, dl, feat, lab, plain
        self.fdim = 0 if feat is None else feat.shape[1]
        self.ldim = 0 if lab is None else lab.shape[1]
        if plain:
            self.fn = _bind(lib, "spr_grid_subsample")
            size = _bind(lib, "spr_grid_subsample_workspace_bytes")(n, nb)
        else:
            self.fn = _bind(lib, "spr_grid_subsample_attrs")
            size = _bind(lib, "spr_grid_subsample_attrs_workspace_size")(n, nb, self.fdim, self.ldim)
        self.ws = torch.empty((size,), dtype=torch.uint8, device=dev)
        self.out = torch.empty((n, 3), dtype=torch.float32, device=dev)
        self.out_feat = torch.empty((n, self.fdim), dtype=torch.float32, device=dev) if self.fdim else None
        self.out_lab = torch.empty((n, self.ldim), dtype=torch.int32, device=dev) if self.ldim else None
        self.lens = torch.empty((nb,), dtype=torch.int32, device=dev)
        self.total = torch.empty((1,), dtype=torch.int32, device=dev)

    def __call__(self):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        head = (_vp(self.pts), _vp(self.cu), self.n, self.nb, self.dl, 0, ops.ORDER_REFERENCE)
        tail = (_vp(self.lens), _vp(self.total), _vp(self.ws), self.ws.numel(), stream)
        if self.plain:
            rc = self.fn(*head, _vp(self.out), *tail)
        else:
            rc = self.fn(*head, _vp(self.feat), self.fdim, _vp(self.lab), self.ldim, _vp(self.out), _vp(self.out_feat),
                         _vp(self.out_lab), *tail)
        assert rc == 0, rc

    def result(self):
        self()
        m = int(self.total.item())
        return [t[:m] for t in (self.out, self.out_feat, self.out_lab) if t is not None] + [self.lens]

    def algorithmic_bytes(self):
        """Inputs read once, outputs written once: points, cu, attributes in; M rows of each and the lengths out."""
        m = int(self.total.item())
        row = 4 * (3 + self.fdim + self.ldim)
        return self.n * row + 4 * (self.nb + 1) + m * row + 4 * self.nb + 4


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
    ap.add_argument("--parent-lib", default=None, help="libspr_hip.so built from the parent commit")
    ap.add_argument("--skip-replica", action="store_true")
    args = ap.parse_args()
    assert args.reps >= 5, "the spread needs at least five repetitions"
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    dev = torch.device("cuda:0")
    cfg = get_config("3dmatch")
    dl = float(cfg.first_subsampling_dl)
    pairs = [synthetic.make_pair(16384, seed=sd) for sd in sharding.pair_seeds(0, args.pairs)]
    clouds = [c for p in pairs for c in (p[0], p[1])]
    host = np.concatenate(clouds).astype(np.float32)
    lens = [len(c) for c in clouds]
    n = len(host)
    rng = np.random.default_rng(0)
    feat3 = rng.uniform(0, 1, (n, 3)).astype(np.float32)                 # colours
    feat32 = rng.normal(0, 1, (n, 32)).astype(np.float32)
    lab1 = rng.integers(0, 20, (n, 1)).astype(np.int32)                  # 20 classes
    pts, cu = torch.from_numpy(host).to(dev), ops.lengths_to_cu(lens, dev)
    d3, d32, dlab = (torch.from_numpy(a).to(dev) for a in (feat3, feat32, lab1))

    here = _lib.lib()
    legs = {"plain": Call(here, pts, cu, dl, plain=True)}
    if args.parent_lib:
        legs["plain_parent"] = Call(ctypes.CDLL(args.parent_lib), pts, cu, dl, plain=True)
    legs["attrs_f3_l1"] = Call(here, pts, cu, dl, d3, dlab)
    legs["attrs_f32_l0"] = Call(here, pts, cu, dl, d32, None)
    results = {k: c.result() for k, c in legs.items()}
    m = results["plain"][0].shape[0]
    ts = event_ms(legs, args.reps, args.launches)
    plain = statistics.median(ts["plain"])
    common = dict(points=n, clouds=len(lens), dl=dl, voxels=m)
    for k, t in ts.items():
        c = legs[k]
        rec = dict(leg=k, **common, **_stats(t))
        same = all(torch.equal(a, b) for a, b in zip((results[k][0], results[k][-1]), (results["plain"][0], results["plain"][-1])))
        rec["points_and_lengths_equal_plain"] = bool(same)
        if not c.plain:
            nbytes = c.algorithmic_bytes()
            rec.update(fdim=c.fdim, ldim=c.ldim, over_plain=round(statistics.median(t) / plain, 4),
                       algorithmic_bytes=nbytes, gb_per_s=round(nbytes / (statistics.median(t) * 1e-3) / 1e9, 2))
        print(json.dumps(rec), flush=True)
    if args.parent_lib:
        spread = (max(ts["plain"]) - min(ts["plain"])) / plain
        print(json.dumps(dict(leg="plain_vs_parent", ratio=round(plain / statistics.median(ts["plain_parent"]), 4),
                              spread_of_plain=round(spread, 4),
                              spread_of_parent=round((max(ts["plain_parent"]) - min(ts["plain_parent"])) /
                                                     statistics.median(ts["plain_parent"]), 4))), flush=True)
    else:
        print(json.dumps(dict(leg="plain_vs_parent", ratio="not measured")), flush=True)

    if not args.skip_replica:
        import subsample_attrs_replica as R
        t0 = time.perf_counter()
        sub, sub_lens, r_feat, r_lab = R.grid_subsample(host, lens, dl, 0, "reference", feat3, lab1)
        s = time.perf_counter() - t0
        got = results["attrs_f3_l1"]
        print(json.dumps(dict(leg="numpy_replica_f3_l1", s=round(s, 2), runs=1,
                              equal_gpu=bool(np.array_equal(got[0].cpu().numpy().view(np.uint32), sub.view(np.uint32)) and
                                             np.array_equal(got[1].cpu().numpy().view(np.uint32), r_feat.view(np.uint32)) and
                                             np.array_equal(got[2].cpu().numpy(), r_lab)))), flush=True)


if __name__ == "__main__":
    main()
