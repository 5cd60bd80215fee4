"""The regulariser of deformable KPConv (csrc/deform_reg.hip) on the deformable level-1 rows of scripts/deform_bench.py
(a 3DMatch pyramid whose level-1 blocks are deformable, PAIRS pairs of 16 384 points), three things on the same rows:

    the fused launch           spr_deform_reg, value only and value + d offset_features
    k_kpconv_deform_min_d2     the launch behind the module's min_d2 attribute, which does a strict subset of the work (the
                               minimum, no argmin, no repulsion, no gradient).  It has no entry point of its own: its time
                               is the forward with min_d2 minus the forward without, on a 1 -> 1 channel convolution
                               (the one-thread-per-output route) so that the forward itself is small beside it
    the torch restatement      the same value and gradient from torch operators on the device: index_select, a broadcast
                               [nq, kmax, K, 3] difference, min, autograd

Device-event times per call, every leg warmed up, the legs alternate over ROUNDS rounds and the median is reported with
the spread (max - min) / median.  The fused results are compared with the torch ones on the rows that are timed.

    python scripts/deform_reg_bench.py [--out profiles/deform_reg_bench.txt] [--pairs 16]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from superpoints_registration_amd import deform_reg, deformable, get_config, synthetic  # noqa: E402
from superpoints_registration_amd.kernel_points import load_kernels  # noqa: E402
from superpoints_registration_amd.kpconv import Preprocessor  # noqa: E402

ARCH = ['simple', 'resnetb', 'resnetb_strided', 'resnetb_deformable', 'resnetb_deformable', 'resnetb_strided',
        'resnetb_deformable', 'resnetb_deformable', 'resnetb']
ROUNDS, REPS = 5, 10
R = 1.2


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def compare(legs):
    """{name: (fn, reps)} -> {name: (median us, spread)}; the legs alternate inside every round."""
    for fn, _ in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, (fn, reps) in legs.items():
            times[k].append(window(fn, reps))
    return {k: (statistics.median(v), (max(v) - min(v)) / statistics.median(v)) for k, v in times.items()}


def torch_reg(q, s, idx, of, kp, e, repulse):
    """include/spr.h's contract with torch operators (float32, on the device); differentiable in of."""
    nq, kmax, K, ns = q.shape[0], idx.shape[1], kp.shape[0], s.shape[0]
    valid = (idx >= 0) & (idx < ns)
    y = s.index_select(0, idx.clamp(0, ns - 1).reshape(-1).long()).view(nq, kmax, 3) - q.unsqueeze(1)
    D = kp + e * of[:, :3 * K].view(nq, K, 3)
    d2 = ((y.unsqueeze(2) - D.unsqueeze(1)) ** 2).sum(3)                                # from [nq, kmax, K, 3]
    d2 = d2.masked_fill(~valid.unsqueeze(2), float('inf'))
    m = torch.where(valid.any(1, keepdim=True), d2.min(1)[0], torch.zeros_like(D[:, :, 0]))
    fit = (m / e ** 2).sum() / (nq * K)
    L = D / e
    sq = ((L.unsqueeze(2) - L.detach().unsqueeze(1)) ** 2).sum(3)
    pos = sq > 0
    dist = torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))
    off_diag = ~torch.eye(K, dtype=torch.bool, device=q.device).unsqueeze(0)
    rep = ((torch.clamp(dist - repulse, max=0.0) * off_diag) ** 2).sum() / (nq * K)
    return 2 * fit + rep, fit, rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "deform_reg_bench.txt"))
    ap.add_argument("--pairs", type=int, default=16)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    cfg = get_config('3dmatch', deformable_kpconv=True, architecture=ARCH)
    pairs = [synthetic.make_pair(16384, seed=i) for i in range(args.pairs)]
    with torch.no_grad():
        meta = Preprocessor(cfg)([torch.from_numpy(p[0]).to(dev) for p in pairs] +
                                 [torch.from_numpy(p[1]).to(dev) for p in pairs])
    gen = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *s: torch.rand(s, device=dev, generator=gen)
    lvl = 1
    nb = meta['neighbors'][lvl].to(torch.int32)
    pts = meta['points'][lvl]
    n, kmax = pts.shape[0], nb.shape[1]
    r = cfg.first_subsampling_dl * cfg.conv_radius * 2 ** lvl
    ext = r * cfg.KP_extent / cfg.conv_radius
    kp = torch.tensor(load_kernels(r, 15, dimension=3, fixed='center'), dtype=torch.float32, device=dev)
    x1, w1 = rand(n, 1) + 0.1, rand(15, 1, 1) - 0.5
    fmt = lambda t: "%9.1f (%2.0f%%)" % (t[0], 100 * t[1])
    lines = [f"{args.pairs} pairs of 16384 points, 3DMatch pyramid with deformable blocks on level 1 (conv search at twice "
             f"the rigid radius): nq {n}, kmax {kmax}, valid/row {float((nb < n).sum()) / n:.1f}, 15 kernel points; "
             f"us per call, median of {ROUNDS} alternating rounds (spread)"]
    for modulated in (False, True):
        od = 60 if modulated else 45
        of = (rand(n, od) - 0.5) * 0.6                        # offsets up to 0.3 extents, as scripts/deform_bench.py
        leaf = of.clone().requires_grad_(True)

        def torch_grad():
            leaf.grad = None
            torch_reg(pts, pts, nb, leaf, kp, ext, R)[0].backward()
            return leaf.grad

        def torch_value():
            with torch.no_grad():
                return torch_reg(pts, pts, nb, of, kp, ext, R)

        with torch.no_grad():
            fwd_min = lambda: deformable.kpconv_deform_raw(pts, pts, nb, x1, w1, kp, ext, of, modulated, want_min_d2=True)
            fwd = lambda: deformable.kpconv_deform_raw(pts, pts, nb, x1, w1, kp, ext, of, modulated)
            t = compare({
                "value": (lambda: deform_reg.deform_reg_raw(pts, pts, nb, of, kp, ext, R), REPS),
                "value + grad": (lambda: deform_reg.deform_reg_raw(pts, pts, nb, of, kp, ext, R, want_grad=True), REPS),
                "fwd 1->1 + min_d2": (fwd_min, REPS), "fwd 1->1": (fwd, REPS),
            })
        t.update(compare({"torch value": (torch_value, 2), "torch value + grad": (torch_grad, 2)}))
        with torch.no_grad():
            out, d_of = deform_reg.deform_reg_raw(pts, pts, nb, of, kp, ext, R, want_grad=True)
            _, min_d2 = fwd_min()
        ref = [float(v) for v in torch_value()]
        g_ref = torch_grad()
        e_val = max(abs(float(a) - b) / b for a, b in zip(out, ref))
        # The minimum's gradient jumps where two neighbours are equally near.  Entries on which the two float32
        # evaluations disagree are listed with the float64 gap between their two nearest neighbours: a gap at float32
        # rounding says the two picked different neighbours of a tie, anything larger would be an error.
        diff = (d_of - g_ref).abs()[:, :45].view(n, 15, 3).amax(2) / g_ref.abs().max()
        flips = (diff > 1e-5).nonzero()
        gaps = []
        for row, p in flips[:64].tolist():
            ok = nb[row] < n
            if int(ok.sum()) < 2:
                continue
            y = (pts[nb[row][ok].long()] - pts[row]).double()
            D = kp[p].double() + ext * of[row, 3 * p:3 * p + 3].double()
            two = torch.topk(((y - D) ** 2).sum(1), 2, largest=False)[0]
            gaps.append(float((two[1] - two[0]) / ext ** 2))
        e_grad = float(diff[diff <= 1e-5].max())
        ties = f"{len(flips)} of {n * 15} entries apart" + (f", their two nearest neighbours within {max(gaps):.1e} e^2 "
                                                            f"of each other in float64" if gaps else "")
        has = (nb < n).any(1)
        implied = float(min_d2[has].double().sum()) / ext ** 2 / (n * 15)
        min_us = t["fwd 1->1 + min_d2"][0] - t["fwd 1->1"][0]
        tag = "modulated" if modulated else "plain"
        lines += [
            f"  {tag:9s} fused launch            value {fmt(t['value'])}   value + gradient {fmt(t['value + grad'])}",
            f"  {tag:9s} k_kpconv_deform_min_d2  {min_us:9.1f}   = forward 1->1 with min_d2 {fmt(t['fwd 1->1 + min_d2'])}"
            f" - without {fmt(t['fwd 1->1'])}",
            f"  {tag:9s} torch restatement       value {fmt(t['torch value'])}   value + gradient {fmt(t['torch value + grad'])}",
            f"  {tag:9s} fused value + gradient / min_d2 kernel {t['value + grad'][0] / min_us:.2f};  torch value + gradient / "
            f"fused {t['torch value + grad'][0] / t['value + grad'][0]:.0f}",
            f"  {tag:9s} fused vs torch (float32): value, fit, rep within {e_val:.1e}, gradient within {e_grad:.1e} of its "
            f"largest entry ({ties}); fit {float(out[1]):.5f}, from min_d2 on rows with a neighbour {implied:.5f}; rep {float(out[2]):.5f}",
        ]
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
