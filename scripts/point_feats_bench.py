"""Per-point input features: what the first KPConv costs at 1, 2, 4 and 8 input channels, and the whole forward with
in_feats_dim 1 and 4.

  * the level-0 call of a batch of PAIRS pairs of 16 384 points (3DMatch pyramid, its own neighbour matrix, 64 output
    channels): C = 1 (k_kpconv_cin1), C = 2, 4, 8 with impl = 0 (k_kpconv_few<C>, records pass included) and C = 4
    with impl = 1 (the generic kernel, what a hand-fed 4-channel input ran on before);
  * RegTR.forward of the same batch in inference with in_feats_dim = 1 (column of ones, fused stem) and 4.

Every shape is warmed up, every figure is the median of ROUNDS alternating rounds of HIP-event windows (min .. max
beside it); outputs of impl 0 and 1 at C = 4 are compared at the timed size.

    python scripts/point_feats_bench.py [--out profiles/point_feats_bench.txt] [--pairs 64]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from superpoints_registration_amd import get_config, ops, synthetic  # noqa: E402
from superpoints_registration_amd.regtr import RegTR  # noqa: E402

ROUNDS = 5


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternating(cases):
    """cases: name -> (fn, reps).  Warm-up of every case, then ROUNDS rounds over all of them in turn; ms per call as
    (median, min, max)."""
    for fn, _ in cases.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in cases}
    for _ in range(ROUNDS):
        for k, (fn, reps) in cases.items():
            got[k].append(window(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "point_feats_bench.txt"))
    ap.add_argument("--pairs", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("point_feats_bench: needs the GPU (no figure is estimated)")
    dev = torch.device('cuda:0')
    cfg = get_config('3dmatch')
    model = RegTR(cfg)
    synthetic.fill_parameters(model, 0)
    model = model.to(dev).eval()
    pairs = [synthetic.make_pair(16384, seed=i) for i in range(args.pairs)]
    src = [torch.from_numpy(p[0]).to(dev) for p in pairs]
    tgt = [torch.from_numpy(p[1]).to(dev) for p in pairs]
    with torch.no_grad():
        meta = model.preprocessor(src + tgt)
    nb = meta['neighbors'][0].to(torch.int32)
    pts = meta['points'][0]
    n = pts.shape[0]
    conv = model.kpf_encoder.encoder_blocks[0].KPConv
    kp, ext = conv.kernel_points.detach(), cfg.first_subsampling_dl * cfg.KP_extent
    g = torch.Generator(device=dev).manual_seed(1)

    def feats(c):
        x = torch.rand((n, c), device=dev, generator=g)
        x[:, 0] = 1.0
        return x

    lines = [f"{args.pairs} pairs of 16384 points, 3DMatch pyramid; level-0 call: {n} queries, {nb.shape[1]} columns, "
             f"{float((nb < n).sum()) / n:.1f} valid per row, 64 output channels; ms per call, median of {ROUNDS} "
             "alternating rounds (min .. max)"]
    cases, outs = {}, {}
    with torch.no_grad():
        operands = {c: (feats(c), (torch.rand((15, c, 64), device=dev, generator=g) - 0.5) * 0.2) for c in (1, 2, 4, 8)}
        for c, impl, reps in ((1, 0, 20), (2, 0, 20), (4, 0, 20), (8, 0, 20), (4, 1, 3)):
            x, w = operands[c]          # C = 4: the same operands on both routes
            fn = (lambda x=x, w=w, impl=impl: ops.kpconv_raw(pts, pts, nb, x, w, kp, ext, rows_sorted=True, impl=impl))
            cases[(c, impl)] = (fn, reps)
            if c == 4:
                outs[impl] = fn()
        res = alternating(cases)
    diff = float((outs[0] - outs[1]).abs().max() / outs[1].abs().max())
    kernel = {(1, 0): "k_kpconv_cin1", (2, 0): "k_kpconv_few<2>", (4, 0): "k_kpconv_few<4>", (8, 0): "k_kpconv_few<8>",
              (4, 1): "k_kpconv_simple"}
    lines.append("  C  impl  kernel             ms/call    (min .. max)     vs next smaller C")
    prev = None
    for key in ((1, 0), (2, 0), (4, 0), (8, 0), (4, 1)):
        med, lo, hi = res[key]
        ratio = "" if key[1] == 1 or prev is None else f"{med / prev:.2f}x"
        lines.append(f"  {key[0]}  {key[1]}     {kernel[key]:<17} {med:8.3f}   ({lo:.3f} .. {hi:.3f})   {ratio}")
        if key[1] == 0:
            prev = med
    lines.append(f"  C = 4: impl 0 is {res[(4, 1)][0] / res[(4, 0)][0]:.1f}x faster than impl 1; outputs differ by {diff:.1e} of scale")

    # the forward in inference, in_feats_dim 1 and 4
    fwd = {}
    with torch.no_grad():
        for c in (1, 4):
            m = RegTR(get_config('3dmatch', in_feats_dim=c))
            synthetic.fill_parameters(m, 0)
            m = m.to(dev).eval()
            batch = {"src_xyz": src, "tgt_xyz": tgt}
            if c > 1:
                fs = list(torch.split(feats(c), [int(t.shape[0]) for t in src + tgt]))    # level 0 is the input cloud
                batch.update(src_point_feats=fs[:len(src)], tgt_point_feats=fs[len(src):])
            fwd[c] = ((lambda m=m, batch=batch: m(dict(batch))), 2)
        res = alternating(fwd)
    lines.append(f"RegTR.forward, inference, {args.pairs} pairs: ms per forward, median of {ROUNDS} alternating rounds (min .. max)")
    for c in (1, 4):
        med, lo, hi = res[c]
        lines.append(f"  in_feats_dim = {c}   {med:9.2f}   ({lo:.2f} .. {hi:.2f})")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
