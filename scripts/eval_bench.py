"""Times the registration metrics for all pairs in one call (evaluation.eval_pairs: csrc/evaluate.hip) against the same
metrics composed from torch operators the way the reference writes them (benchmark_modelnet.compute_metrics:
se3_cat / se3_inv / se3_transform, square_distance as a materialised [B, n, m, 3] difference, min, mean -- in float32
on the same device, batched over pairs and chunked so that one difference tensor stays below 1 GiB; the Euler angles
from the same closed form on the device, where the reference goes through scipy on the host).  Shapes:
  modelnet   256 pairs of 717 / 717 / 2048 points (source / reference / raw shape)
  large      64 pairs of 4096 / 4096 / 16384 points
Per shape one JSON line per leg -- call (evaluation.eval_pairs_raw on the lists), composed, library (spr_eval_pairs on
tensors packed once outside the timed region: the call without the host layer's per-cloud work) -- and one with the
float64 cost model of the search:
  9 float64 VALU instructions per (query, target) -- 3 subtractions, 3 multiplications, 2 additions, 1 compare --
  at 256 CUs x 4 SIMDs x 16 float64 lanes per clock x 2.4 GHz = 39.3e12 lane-instructions per second
  (the 78.6 TFLOPS float64 vector peak counts an FMA as two; the contract allows none)
and the fraction of it the call achieves.  HIP events around every call, warm-up, median of the repeats.  Writes
profiles/eval_bench.txt.

    python scripts/eval_bench.py [--reps 5]
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

from superpoints_registration_amd import evaluation as E  # noqa: E402
from superpoints_registration_amd.se3 import se3_cat, se3_inv, se3_transform  # noqa: E402

SHAPES = {"modelnet": (256, 717, 717, 2048), "large": (64, 4096, 4096, 16384)}
F64_LANE_INSTR_PER_S = 256 * 4 * 16 * 2.4e9
INSTR_PER_PAIR = 9
CHUNK_BYTES = 1 << 30


def timed(fn, reps, warm=2):
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


def rigid(rng, angle, trans):
    k = rng.normal(size=3)
    k /= np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = np.deg2rad(angle)
    t = rng.normal(size=3)
    return np.hstack([np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K), (t * trans / np.linalg.norm(t))[:, None]])


def make(nb, ns, nt, nr, dev, seed=0):
    rng = np.random.default_rng(seed)
    gt = np.stack([rigid(rng, rng.uniform(5, 45), 0.5) for _ in range(nb)])
    d = np.stack([rigid(rng, rng.uniform(1, 5), 0.05) for _ in range(nb)])
    pred = np.stack([np.hstack([d[b][:, :3] @ gt[b][:, :3], (d[b][:, :3] @ gt[b][:, 3] + d[b][:, 3])[:, None]]) for b in range(nb)])
    raw = rng.uniform(-1, 1, (nb, nr, 3))
    ref = raw[:, rng.integers(0, nr, nt)] + rng.normal(0, 0.01, (nb, nt, 3))
    back = raw[:, rng.integers(0, nr, ns)] + rng.normal(0, 0.01, (nb, ns, 3))
    src = np.einsum('bij,bnj->bni', np.transpose(gt[:, :, :3], (0, 2, 1)), back - gt[:, None, :, 3])
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    return f(src), f(ref), f(raw), f(gt), f(pred)


def euler_deg(rot):
    return torch.rad2deg(torch.stack([torch.atan2(rot[:, 2, 1], rot[:, 2, 2]), -torch.asin(rot[:, 2, 0].clamp(-1, 1)),
                                      torch.atan2(rot[:, 1, 0], rot[:, 0, 0])], dim=1))


def min_sq(a, b):
    """min over b of the reference's square_distance(a, b), a [B,n,3], b [B,m,3]; chunked over pairs, then queries."""
    B, n, m = a.shape[0], a.shape[1], b.shape[1]
    per_pair = n * m * 3 * 4
    out = torch.empty((B, n), dtype=a.dtype, device=a.device)
    if per_pair <= CHUNK_BYTES:
        step = max(1, CHUNK_BYTES // per_pair)
        for s in range(0, B, step):
            out[s:s + step] = torch.sum((a[s:s + step, :, None, :] - b[s:s + step, None, :, :]) ** 2, dim=-1).min(dim=-1)[0]
    else:
        qstep = max(1, CHUNK_BYTES // (m * 3 * 4))
        for s in range(B):
            for q in range(0, n, qstep):
                out[s, q:q + qstep] = torch.sum((a[s:s + 1, q:q + qstep, None, :] - b[s:s + 1, None, :, :]) ** 2, dim=-1).min(dim=-1)[0][0]
    return out


def composed(src, ref, raw, gt, pred):
    e = euler_deg(gt[:, :, :3]) - euler_deg(pred[:, :, :3])
    t = gt[:, :, 3] - pred[:, :, 3]
    cat = se3_cat(se3_inv(gt), pred)
    trace = cat[:, 0, 0] + cat[:, 1, 1] + cat[:, 2, 2]
    moved_raw = se3_transform(se3_cat(pred, se3_inv(gt)), raw)
    return {'r_mse': (e ** 2).mean(1), 'r_mae': e.abs().mean(1), 't_mse': (t ** 2).mean(1), 't_mae': t.abs().mean(1),
            'err_r_deg': torch.acos(torch.clamp(0.5 * (trace - 1), min=-1.0, max=1.0)) * 180.0 / np.pi,
            'err_t': cat[:, :, 3].norm(dim=-1),
            'chamfer_dist': min_sq(se3_transform(pred, src), raw).mean(1) + min_sq(ref, moved_raw).mean(1)}


def packed_call(src, ref, raw, gt, pred):
    """spr_eval_pairs itself on tensors packed once outside the timed region: what the library costs without the host
    layer's per-cloud checks, concatenations and allocations (the `call` leg has them: 768 list entries on `modelnet`)."""
    from superpoints_registration_amd import _lib, ops
    nb, dev = src.shape[0], src.device
    flat = lambda x: x.reshape(-1, 3).contiguous()
    cu = lambda x: ops.lengths_to_cu([x.shape[1]] * nb, dev)
    s, t, r = flat(src), flat(ref), flat(raw)
    s_cu, t_cu, r_cu = cu(src), cu(ref), cu(raw)
    g64, p64 = gt.double().contiguous(), pred.double().contiguous()
    ns, nt, nr = s.shape[0], t.shape[0], r.shape[0]
    L = _lib.lib()
    ws = torch.empty(L.spr_eval_pairs_workspace_size(ns, nt, nr, 0, nb), dtype=torch.uint8, device=dev)
    metrics = torch.empty((nb, len(E.COLUMNS)), dtype=torch.float64, device=dev)
    status = torch.empty((nb,), dtype=torch.int32, device=dev)
    d2s, d2r = torch.empty(ns, dtype=torch.float64, device=dev), torch.empty(nt, dtype=torch.float64, device=dev)
    nns, nnr = torch.empty(ns, dtype=torch.int32, device=dev), torch.empty(nt, dtype=torch.int32, device=dev)
    keep = (s, t, r, s_cu, t_cu, r_cu, g64, p64, ws, metrics, status, d2s, d2r, nns, nnr)

    def call():
        _lib.check(L.spr_eval_pairs(ops._ptr(s), ops._ptr(s_cu), ns, ops._ptr(t), ops._ptr(t_cu), nt, ops._ptr(r),
                                    ops._ptr(r_cu), nr, None, None, None, 0, ops._ptr(g64), ops._ptr(p64), nb, 0.0,
                                    ops._ptr(metrics), ops._ptr(d2s), ops._ptr(nns), ops._ptr(d2r), ops._ptr(nnr),
                                    ops._ptr(status), ops._ptr(ws), ws.numel(), ops._stream(s)), "spr_eval_pairs")
        return keep
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    for name, (nb, ns, nt, nr) in SHAPES.items():
        src, ref, raw, gt, pred = make(nb, ns, nt, nr, dev)
        src_l, ref_l, raw_l = list(src), list(ref), list(raw)
        call = lambda: E.eval_pairs_raw(src_l, ref_l, gt, pred, raw_list=raw_l)
        t_call = timed(call, args.reps)
        t_lib = timed(packed_call(src, ref, raw, gt, pred), args.reps)
        t_comp = timed(lambda: composed(src, ref, raw, gt, pred), max(2, args.reps // 2), warm=1)
        ours, theirs = E.eval_pairs(src_l, ref_l, gt, pred, raw_list=raw_l), composed(src, ref, raw, gt, pred)
        diff = {k: float(((ours[k] - theirs[k].double()).abs() / theirs[k].double().abs().clamp(min=1e-9)).max())
                for k in E.MODELNET_KEYS}
        base = dict(shape=name, pairs=nb, n_src=ns, n_ref=nt, n_raw=nr)
        emit(leg="call", **base, ms=round(t_call[0], 3), ms_min=round(t_call[1], 3), ms_max=round(t_call[2], 3))
        emit(leg="composed", **base, ms=round(t_comp[0], 3), ms_min=round(t_comp[1], 3), ms_max=round(t_comp[2], 3),
             composed_over_call=round(t_comp[0] / t_call[0], 2),
             worst_relative_difference_to_float32_torch={k: float(f"{v:.2e}") for k, v in diff.items()})
        evals = nb * (ns + nt) * nr
        model_ms = evals * INSTR_PER_PAIR / F64_LANE_INSTR_PER_S * 1e3
        emit(leg="library", **base, ms=round(t_lib[0], 3), ms_min=round(t_lib[1], 3), ms_max=round(t_lib[2], 3))
        emit(leg="f64_cost_model", **base, pair_evaluations=evals, model_ms=round(model_ms, 3),
             achieved_fraction_call=round(model_ms / t_call[0], 3), achieved_fraction_library=round(model_ms / t_lib[0], 3))
        del src, ref, raw, src_l, ref_l, raw_l
        torch.cuda.empty_cache()
    out = os.path.join(REPO, "profiles", "eval_bench.txt")
    with open(out, "w") as f:
        f.write("# scripts/eval_bench.py on one MI355X; see the script's docstring for the legs\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
