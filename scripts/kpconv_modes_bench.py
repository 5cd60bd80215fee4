"""The six KPConv modes through the mode kernel (spr_kpconv_modes_fwd, csrc/kpconv_modes.hip) beside the shipped
linear / sum kernels (spr_kpconv_fwd: ring kernel at 32 / 64 channels, tile kernel at 128) on the same tensors: the
neighbour matrices of the bench pyramid (PAIRS pairs of 16 384 points, 3DMatch config), 32 -> 32 at level 0, 64 -> 64 at
level 1, 128 -> 128 at level 2.  Time per launch with the weight planes and the operand ranges cached, as in the model.

    python scripts/kpconv_modes_bench.py [--out profiles/kpconv_modes_bench.txt] [--pairs 64]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from superpoints_registration_amd import get_config, kpconv_modes, ops, synthetic  # noqa: E402
from superpoints_registration_amd.regtr import RegTR  # noqa: E402

MODES = [(i, a) for a in ('sum', 'closest') for i in ('constant', 'linear', 'gaussian')]


def timed(fn, reps=10):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "kpconv_modes_bench.txt"))
    ap.add_argument("--pairs", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    cfg = get_config('3dmatch')
    model = RegTR(cfg)
    synthetic.fill_parameters(model, 0)
    model = model.to(dev).eval()
    pairs = [synthetic.make_pair(16384, seed=i) for i in range(args.pairs)]
    with torch.no_grad():
        meta = model.preprocessor([torch.from_numpy(p[0]).to(dev) for p in pairs] +
                                  [torch.from_numpy(p[1]).to(dev) for p in pairs])
    kp0 = model.kpf_encoder.encoder_blocks[1].KPConv.kernel_points.detach()
    lines = [f"{args.pairs} pairs of 16384 points, 3DMatch pyramid, same-level neighbour matrices; us per launch",
             "level  cin->cout       nq  valid/row | shipped linear/sum | " + " | ".join("%8s/%-7s" % m for m in MODES)]
    for lvl, c in ((0, 32), (1, 64), (2, 128)):
        nb = meta['neighbors'][lvl].to(torch.int32)
        pts = meta['points'][lvl]
        n = pts.shape[0]
        x = torch.rand((n, c), device=dev) - 0.3
        ops.ensure_range(x)
        w = (torch.rand((15, c, c), device=dev) - 0.5) * 0.2
        kp, ext = kp0 * (2 ** lvl), cfg.first_subsampling_dl * cfg.KP_extent * (2 ** lvl)
        with torch.no_grad():
            shipped = lambda: ops.kpconv_raw(pts, pts, nb, x, w, kp, ext, rows_sorted=True)
            y0 = shipped()
            t0 = timed(shipped)
            row, ratios = [], []
            for infl, agg in MODES:
                codes = kpconv_modes.mode_codes(infl, agg)
                f = lambda: kpconv_modes.kpconv_raw(pts, pts, nb, x, w, kp, ext, *codes)
                y = f()
                t = timed(f)
                row.append(t)
                ratios.append(t / t0)
                if (infl, agg) == ('linear', 'sum'):
                    diff = float((y - y0).abs().max() / y0.abs().max())
        lines.append("L%d    %4d->%-4d %8d %10.1f | %18.1f | " % (lvl, c, c, n, float((nb < n).sum()) / n, t0) +
                     " | ".join("%16.1f" % t for t in row))
        lines.append("       ratio to the shipped kernel%28s" % "" + " | ".join("%16.2f" % r for r in ratios) +
                     "   (linear/sum outputs differ by %.1e of scale)" % diff)
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
