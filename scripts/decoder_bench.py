"""Times the KPConv decoder at the bench shape: 64 synthetic pairs of 16 384 points (bench.py's seeds), 3DMatch
architecture + ['nearest_upsample', 'unary', 'nearest_upsample', 'unary'], inference, in one process:

  per level   decoder.upsample_unary on the encoder's real tensors, route 'fused' (one spr_upsample_unary call) against
              route 'operator' (ops.gather_rows + two ops.linear calls), alternating inside every repetition; the
              operator route is timed twice per repetition, and the difference of the two series' medians is the
              spread a route shows against itself;
  decoder     KPFDecoder.forward with the fused call as the default and with the operator route forced, beside
              KPFEncoder.forward on the same pyramid.

HIP events around each call, then a synchronise; warm-up calls first; median, minimum and maximum over the repetitions.
Per level the algorithmic bytes (skip rows + one coarse row per fine row + indices + weights read, result written; the
lower bound with every coarse row read once is given beside it) and the matrix FLOPs of the split product (three fp16
MFMAs per product: 6 n K n_out) give the time at the HBM peak (8 TB/s) and at the fp16 matrix peak (2.5 PFLOP/s); the
larger of the two binds.  Writes profiles/decoder_bench.txt.

    python scripts/decoder_bench.py [--reps 20] [--points 16384] [--pairs 64]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from superpoints_registration_amd import decoder, get_config, sharding, synthetic  # noqa: E402
from superpoints_registration_amd.kpconv import KPFDecoder, KPFEncoder, Preprocessor  # noqa: E402
from superpoints_registration_amd.kpconv_blocks import _idx_of  # noqa: E402

DECODER = ['nearest_upsample', 'unary', 'nearest_upsample', 'unary']
HBM_PEAK = 8.0e12
F16_MATRIX_PEAK = 2.5e15


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "decoder_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "decoder_bench needs the MI355X"
    dev = torch.device("cuda:0")
    cfg = get_config("3dmatch")
    cfg["architecture"] = list(cfg.architecture) + DECODER

    class Backbone(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder = KPFEncoder(cfg, cfg.d_embed)
            self.decoder = KPFDecoder(cfg, self.encoder.encoder_skip_dims[-1], self.encoder.encoder_skip_dims)

    model = Backbone()
    synthetic.fill_parameters(model, seed=0)
    model = model.to(dev).eval()
    pairs = [synthetic.make_pair(args.points, seed=s) for s in sharding.pair_seeds(0, args.pairs)]
    clouds = [torch.from_numpy(p[0]).to(dev) for p in pairs] + [torch.from_numpy(p[1]).to(dev) for p in pairs]
    lines = []
    with torch.no_grad():
        meta = Preprocessor(cfg)(clouds)
        feats = torch.ones((meta["points"][0].shape[0], 1), device=dev)
        x, skips = model.encoder(feats, meta)
        rows = [int(p.shape[0]) for p in meta["points"]]
        lines.append(json.dumps({"what": "shape", "pairs": args.pairs, "points": args.points, "rows_per_level": rows,
                                 "reps": args.reps}))

        def time_level(what, xc, xs, idx, w):
            (nc, kc), (n, ks), n_out = xc.shape, xs.shape, w.shape[0]
            fused = lambda: decoder.upsample_unary(xc, xs, idx, w, route="fused")
            oper = lambda: decoder.upsample_unary(xc, xs, idx, w, route="operator")
            for _ in range(3):
                a, b = fused(), oper()
            torch.cuda.synchronize()
            diff = float((a - b).abs().max() / b.abs().max())
            t = {"fused": [], "operator": [], "operator_again": []}
            for _ in range(args.reps):
                t["fused"].append(event_ms(fused)[0])
                t["operator"].append(event_ms(oper)[0])
                t["operator_again"].append(event_ms(oper)[0])
            res = {k: stats(v) for k, v in t.items()}
            spread = abs(res["operator"]["median_ms"] - res["operator_again"]["median_ms"])
            gain = min(res["operator"]["median_ms"], res["operator_again"]["median_ms"]) - res["fused"]["median_ms"]
            K = kc + ks
            bytes_fused = 4 * (n * ks + n * kc + n + n_out * K + n * n_out)
            bytes_fused_min = 4 * (n * ks + nc * kc + n + n_out * K + n * n_out)
            # gather writes and the second product re-reads the gathered rows; the second product re-reads the first's result
            bytes_oper = bytes_fused + 4 * (2 * n * kc + 2 * n * n_out)
            flops = 6.0 * n * K * n_out
            hbm_ms, mat_ms = bytes_fused / HBM_PEAK * 1e3, flops / F16_MATRIX_PEAK * 1e3
            res.update(what=what, n=n, nc=nc, kc=kc, ks=ks, n_out=n_out,
                       fused_vs_operator_max_rel_diff=diff, spread_ms=round(spread, 4), fused_gain_ms=round(gain, 4),
                       fused_is_faster_beyond_spread=bool(gain > spread),
                       bytes_fused=bytes_fused, bytes_fused_unique_coarse_rows=bytes_fused_min, bytes_operator=bytes_oper,
                       matrix_flops=flops, hbm_bound_ms=round(hbm_ms, 4), f16_matrix_bound_ms=round(mat_ms, 4),
                       binds="hbm" if hbm_ms > mat_ms else "matrix",
                       fused_share_of_hbm_bound=round(hbm_ms / res["fused"]["median_ms"], 4),
                       fused_share_of_matrix_bound=round(mat_ms / res["fused"]["median_ms"], 4))
            lines.append(json.dumps(res))
            return a

        # ---- per level: the decoder's own tensors, level 1 first ---------------------------------------------------
        xc = x
        for j, level in ((1, 1), (3, 0)):
            unary = model.decoder.decoder_blocks[j]
            a = time_level(f"level {level}", xc, skips[level], _idx_of(meta, "upsamples", level), unary.mlp.weight.detach())
            xc = unary.batch_norm(a, meta["stack_lengths"][level], cu=meta["_cu"][level], slope=0.1,
                                  max_len=max(meta["_lens_host"][level]))
        del xc, a

        # ---- the other widths spr_upsample_unary_supported answers for (a KITTI- or ModelNet-width pyramid, and
        # reduce_channel_when_upsample=False), on seeded tensors at this pyramid's row counts; indices ascending
        # like a pyramid's (neighbouring fine rows share coarse rows)
        for kc, ks, n_out, n, nc in ((1024, 512, 512, rows[2], rows[2] // 4), (1024, 512, 1024, rows[2], rows[2] // 4),
                                     (512, 256, 512, rows[1], rows[2]), (256, 128, 256, rows[0], rows[1])):
            g = torch.Generator(device=dev).manual_seed(kc + n_out)
            sxc = torch.rand((nc, kc), generator=g, device=dev) * 2 - 1
            sxs = torch.rand((n, ks), generator=g, device=dev) * 2 - 1
            sw = (torch.rand((n_out, kc + ks), generator=g, device=dev) * 2 - 1) * (3.0 / (kc + ks)) ** 0.5
            sidx = (torch.arange(n, device=dev, dtype=torch.int64) * nc // n).to(torch.int32)
            time_level(f"synthetic {kc}+{ks}->{n_out}", sxc, sxs, sidx, sw)
            del sxc, sxs, sw, sidx

        # ---- the decoder as a whole, beside the encoder ---------------------------------------------------------------
        real = decoder.supported
        run_dec = lambda: model.decoder(x, list(skips), meta)
        run_enc = lambda: model.encoder(feats, meta)
        t = {"decoder_default": [], "decoder_operator_route": [], "encoder": []}
        for rep in range(-3, args.reps):
            for key, fn, sup in (("decoder_default", run_dec, real), ("decoder_operator_route", run_dec, lambda *a: False),
                                 ("encoder", run_enc, real)):
                decoder.supported = sup
                ms = event_ms(fn)[0]
                if rep >= 0:
                    t[key].append(ms)
        decoder.supported = real
        res = {k: stats(v) for k, v in t.items()}
        res.update(what="whole", default_route_per_level={f"level {l}": ("fused" if real(kc_, ks_, no_) else "operator")
                                                          for l, (kc_, ks_, no_) in ((1, (512, 256, 256)), (0, (256, 128, 128)))})
        lines.append(json.dumps(res))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
