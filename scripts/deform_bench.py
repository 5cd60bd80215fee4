"""Deformable KPConv (csrc/kpconv_deform.hip) beside the rigid mode kernel (spr_kpconv_modes_*, linear / sum) on the same
rows: the fused forward, the weighted-features and d x kernels, the offset-gradient kernel (no rigid counterpart), and the
offset convolution at its own width (45 / 60 columns) beside the same convolution on weights zero-padded to 64 columns.
Rows are the conv matrices of levels 1 and 2 of a 3DMatch pyramid whose blocks there are deformable (search radius =
deform_radius / conv_radius = 2 x the rigid one), PAIRS pairs of 16 384 points: 64 -> 64 and 128 -> 128 channels.

Device-event times per launch, weight planes and operand ranges cached as in the model; every leg is warmed up, the legs
of a comparison alternate over ROUNDS rounds and the median is reported with the spread (max - min) / median.

    python scripts/deform_bench.py [--out profiles/deform_bench.txt] [--pairs 64]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from superpoints_registration_amd import deformable, get_config, kpconv_modes, ops, synthetic  # noqa: E402
from superpoints_registration_amd.kernel_points import load_kernels  # noqa: E402
from superpoints_registration_amd.kpconv import Preprocessor  # noqa: E402

ARCH = ['simple', 'resnetb', 'resnetb_strided', 'resnetb_deformable', 'resnetb_deformable', 'resnetb_strided',
        'resnetb_deformable', 'resnetb_deformable', 'resnetb']
ROUNDS, REPS = 5, 10
LIN_SUM = (1, 0)


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / REPS * 1e3


def compare(legs):
    """{name: fn} -> {name: (median us, spread)}; the legs alternate inside every round."""
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, fn in legs.items():
            times[k].append(window(fn))
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "deform_bench.txt"))
    ap.add_argument("--pairs", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    cfg = get_config('3dmatch', deformable_kpconv=True, architecture=ARCH)
    pairs = [synthetic.make_pair(16384, seed=i) for i in range(args.pairs)]
    with torch.no_grad():
        meta = Preprocessor(cfg)([torch.from_numpy(p[0]).to(dev) for p in pairs] +
                                 [torch.from_numpy(p[1]).to(dev) for p in pairs])
    gen = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *s: torch.rand(s, device=dev, generator=gen)
    lines = [f"{args.pairs} pairs of 16384 points, 3DMatch pyramid with deformable blocks on levels 1 and 2 (conv search at "
             f"twice the rigid radius); us per launch, median of {ROUNDS} alternating rounds of {REPS} (spread)"]
    fmt = lambda r: "%9.1f (%2.0f%%)" % (r[0], 100 * r[1])
    for lvl, c in ((1, 64), (2, 128)):
        nb = meta['neighbors'][lvl].to(torch.int32)
        pts = meta['points'][lvl]
        n, kmax = pts.shape[0], nb.shape[1]
        r = cfg.first_subsampling_dl * cfg.conv_radius * 2 ** lvl
        ext = r * cfg.KP_extent / cfg.conv_radius
        kp = torch.tensor(load_kernels(r, 15, dimension=3, fixed='center'), dtype=torch.float32, device=dev)
        x = rand(n, c) - 0.3
        ops.ensure_range(x)
        w = (rand(15, c, c) - 0.5) * 0.2
        dwfm = rand(n, 15 * c) - 0.5
        ops.ensure_range(dwfm)
        res = {}
        with torch.no_grad():
            for modulated in (False, True):
                od = 60 if modulated else 45
                of = (rand(n, od) - 0.5) * 0.6                # offsets up to 0.3 extents, modulations 2 sigmoid(+-0.3)
                w_off = (rand(15, c, od) - 0.5) * 0.05
                w_pad = torch.zeros((15, c, 64), device=dev)
                w_pad[:, :, :od] = w_off
                fwd = lambda: deformable.kpconv_deform_raw(pts, pts, nb, x, w, kp, ext, of, modulated)
                rigid = lambda: kpconv_modes.kpconv_raw(pts, pts, nb, x, w, kp, ext, *LIN_SUM)
                tag = "modulated" if modulated else "plain"
                res[tag] = compare({
                    "fwd rigid": rigid, "fwd deform": fwd,
                    "wf rigid": lambda: kpconv_modes.weighted_features(pts, pts, nb, x, kp, ext, *LIN_SUM),
                    "wf deform": lambda: deformable.weighted_features(pts, pts, nb, x, kp, ext, of),
                    "dx rigid": lambda: kpconv_modes.bwd_dx(pts, pts, nb, c, kp, ext, *LIN_SUM, dwfm),
                    "dx deform": lambda: deformable.bwd_dx(pts, pts, nb, c, kp, ext, of, modulated, dwfm),
                    "offsets deform": lambda: deformable.bwd_offsets(pts, pts, nb, x, kp, ext, of, modulated, dwfm),
                    "offset conv own width": lambda: ops.kpconv_raw(pts, pts, nb, x, w_off, kp, ext, rows_sorted=True),
                    "offset conv padded 64": lambda: ops.kpconv_raw(pts, pts, nb, x, w_pad, kp, ext, rows_sorted=True)[:, :od],
                })
                own = ops.kpconv_raw(pts, pts, nb, x, w_off, kp, ext, rows_sorted=True)
                pad = ops.kpconv_raw(pts, pts, nb, x, w_pad, kp, ext, rows_sorted=True)[:, :od]
                res[tag + " pad diff"] = float((own - pad).abs().max() / own.abs().max())
            d = (pts[nb.clamp(max=n - 1).long()] - pts.unsqueeze(1)).norm(dim=2)
            valid = nb < n
            in_rigid = float(((d < 2 * ext) & valid).sum()) / n      # neighbours within two extents of their query
        lines.append(f"L{lvl}  {c}->{c}  nq {n}  kmax {kmax}  valid/row {float(valid.sum()) / n:.1f}  "
                     f"within 2 extents/row {in_rigid:.1f}  x gather {n * float(valid.sum()) / n * c * 4 / 1e6:.0f} MB if every valid row is read")
        for tag in ("plain", "modulated"):
            t = res[tag]
            lines.append(f"  {tag:9s} forward        rigid {fmt(t['fwd rigid'])}  deformable {fmt(t['fwd deform'])}  "
                         f"ratio {t['fwd deform'][0] / t['fwd rigid'][0]:.2f}")
            lines.append(f"  {tag:9s} wf + count     rigid {fmt(t['wf rigid'])}  deformable {fmt(t['wf deform'])}  "
                         f"ratio {t['wf deform'][0] / t['wf rigid'][0]:.2f}")
            lines.append(f"  {tag:9s} d x scatter    rigid {fmt(t['dx rigid'])}  deformable {fmt(t['dx deform'])}  "
                         f"ratio {t['dx deform'][0] / t['dx rigid'][0]:.2f}")
            lines.append(f"  {tag:9s} d offsets                              deformable {fmt(t['offsets deform'])}  "
                         f"ratio to the rigid wf kernel {t['offsets deform'][0] / t['wf rigid'][0]:.2f}")
            lines.append(f"  {tag:9s} offset conv    own width {fmt(t['offset conv own width'])}  padded to 64 + slice "
                         f"{fmt(t['offset conv padded 64'])}  ratio {t['offset conv padded 64'][0] / t['offset conv own width'][0]:.2f}"
                         f"  (outputs differ by {res[tag + ' pad diff']:.1e} of scale)")
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
