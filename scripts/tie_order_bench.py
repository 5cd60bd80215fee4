"""What tie_order='reference' costs and how many rows it touches -- nobody chooses it for speed; it is for parity.
  * the bench batch: --pairs 64 synthetic pairs of --points 16 384 (synthetic.make_pair), 3DMatch config;
  * the worst case: the 8 x 8 x 4 lattices of tests/tie_order_cases.py (every row ties), one search per limit.
Per pyramid level and search (conv / pool / up): the kd-tree replay's build time (once per support set), the fix-up
time, rows_fixed / rows and the scratch the fix-up asked for; host clock around each call plus a device synchronise,
on the second forward (the first one grows the workspace).  Then Preprocessor.forward and the RegTR forward with the
option off and on, alternating inside every repetition.  One JSON line per record.

    python scripts/tie_order_bench.py [--pairs 64] [--points 16384] [--reps 5]
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

import tie_order_cases as tc  # noqa: E402
from superpoints_registration_amd import get_config, ops, sharding, synthetic, tie_order  # noqa: E402
from superpoints_registration_amd.kpconv import Preprocessor  # noqa: E402
from superpoints_registration_amd.regtr import RegTR  # noqa: E402


class Tap:
    """Times every ReplayTree build and apply of the forwards run inside it, in call order."""

    def __enter__(self):
        self.events = []
        self._init, self._apply = tie_order.ReplayTree.__init__, tie_order.ReplayTree.apply
        tap = self

        def init(tree, supports, s_cu):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tap._init(tree, supports, s_cu)
            torch.cuda.synchronize()
            tap.events.append(dict(kind="build", ns=tree.ns, clouds=tree.nb, depth=tree.depth,
                                   tree_bytes=tree.blob.numel(), ms=1e3 * (time.perf_counter() - t0)))

        def apply(tree, nbr, queries, q_cu, radius, max_count):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = tap._apply(tree, nbr, queries, q_cu, radius, max_count)
            torch.cuda.synchronize()
            tap.events.append(dict(kind="fix", rows=st.rows, width=int(nbr.shape[1]), max_count=int(max_count),
                                   rows_fixed=st.rows_fixed, set_mismatch=st.set_mismatch,
                                   scratch_bytes=tree.scratch_bytes(nbr.shape[0], max_count),
                                   ms=1e3 * (time.perf_counter() - t0)))
            return st

        tie_order.ReplayTree.__init__, tie_order.ReplayTree.apply = init, apply
        return self

    def __exit__(self, *exc):
        tie_order.ReplayTree.__init__, tie_order.ReplayTree.apply = self._init, self._apply


def alternate(fns, reps):
    ts = {k: [] for k in fns}
    keys = list(fns)
    for rep in range(reps):
        for k in (keys if rep % 2 == 0 else keys[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fns[k]()
            torch.cuda.synchronize()
            ts[k].append(1e3 * (time.perf_counter() - t0))
    return {k: dict(ms=round(statistics.median(v), 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-model", action="store_true", help="skip the RegTR forward (pyramid only)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU"
    dev = torch.device("cuda:0")
    pairs = [synthetic.make_pair(args.points, seed=sd) for sd in sharding.pair_seeds(0, args.pairs)]
    src = [torch.from_numpy(p[0]).to(dev) for p in pairs]
    tgt = [torch.from_numpy(p[1]).to(dev) for p in pairs]
    cfg = get_config("3dmatch")
    pre = {"index": Preprocessor(cfg), "reference": Preprocessor(cfg, tie_order='reference')}
    for _ in range(2):
        for p in pre.values():
            p(src + tgt)
    with Tap() as tap:
        pre["reference"](src + tgt)
    keys = list(pre["reference"].tie_status)
    fixes = [e for e in tap.events if e["kind"] == "fix"]
    assert len(fixes) == len(keys)
    it = iter(fixes)
    for e in tap.events:
        if e["kind"] == "build":
            print(json.dumps(dict(leg="tree_build", workload="3dmatch", **{k: (round(v, 3) if k == "ms" else v)
                                                                           for k, v in e.items() if k != "kind"})), flush=True)
    for key, e in zip(keys, it):
        print(json.dumps(dict(leg="fix_up", workload="3dmatch", level=key[0], search=key[1], rows=e["rows"],
                              rows_fixed=e["rows_fixed"], share=round(e["rows_fixed"] / max(e["rows"], 1), 5),
                              width=e["width"], max_count=e["max_count"], set_mismatch=e["set_mismatch"],
                              scratch_bytes=e["scratch_bytes"], ms=round(e["ms"], 3))), flush=True)
    res = alternate({k: (lambda p=p: p(src + tgt)) for k, p in pre.items()}, args.reps)
    for k, v in res.items():
        print(json.dumps(dict(leg="preprocessor_forward", workload="3dmatch", tie_order=k, clouds=2 * args.pairs,
                              points=2 * args.pairs * args.points, reps=args.reps, **v)), flush=True)
    if not args.no_model:
        models = {}
        for k in pre:
            m = RegTR(get_config("3dmatch", tie_order=k))
            synthetic.fill_parameters(m, seed=0)
            models[k] = m.to(dev).eval()
        batch = {"src_xyz": src, "tgt_xyz": tgt}
        with torch.no_grad():
            for _ in range(2):
                for m in models.values():
                    m(batch)
            res = alternate({k: (lambda m=m: m(batch)) for k, m in models.items()}, args.reps)
        for k, v in res.items():
            print(json.dumps(dict(leg="regtr_forward", workload="3dmatch", tie_order=k, pairs=args.pairs, reps=args.reps,
                                  **v)), flush=True)

    # worst case: every row of the lattice ties
    for name in ("lat.r27", "lat.r123", "latdup.r57"):
        c = tc.cases()[name]
        s, scu = torch.tensor(c.sup).to(dev), ops.lengths_to_cu(list(c.s_lens), dev)
        for limit in tc.LIMITS:
            ops.radius_neighbors(s, s, scu, scu, c.radius, limit, tie_order='reference')
            with Tap() as tap:
                ops.radius_neighbors(s, s, scu, scu, c.radius, limit, tie_order='reference')
            b, f = tap.events
            print(json.dumps(dict(leg="lattice", case=name, limit=limit, rows=f["rows"], rows_fixed=f["rows_fixed"],
                                  max_count=f["max_count"], depth=b["depth"], scratch_bytes=f["scratch_bytes"],
                                  build_ms=round(b["ms"], 3), fix_ms=round(f["ms"], 3))), flush=True)


if __name__ == "__main__":
    main()
