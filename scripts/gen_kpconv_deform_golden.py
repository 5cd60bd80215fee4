"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/kpconv_deform.npz and tests/golden/deform_encoder.npz by running the
reference's own KPConv class with deformable=True and its KPFEncoder / Preprocessor with deformable block names
(models/backbone_kpconv, loaded through oracle.ref_harness) in float32 on the CPU.  Run from the repo root in the dev
container:

    python scripts/gen_kpconv_deform_golden.py [reference src]

kpconv_deform.npz: inputs are tests/deform_cases.golden_case(modulated) (regenerable from their seeds, not stored) except
both convolutions' kernel points: the reference draws them itself (load_kernels: the global numpy RNG, seeded here; the
offset convolution's first), so they are stored.  Per modulated off / on: the output, d x, d offset_bias, min_d2 and
deformed_KP whole; every GOLDEN_DW_STEP-th entry of d W and of the offset convolution's d W with their norms, for the
output gradient kpconv_modes_cases.golden_go().

deform_encoder.npz: two small clouds (stored), the reference Preprocessor's pyramid for each architecture of
deform_cases.ENCODER_ARCHS (points, conv and pool index matrices as int16, lengths) and its KPFEncoder's features with
the parameters of synthetic.fill_parameters(encoder, ENCODER_SEED) on an all-ones input feature.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_harness  # noqa: E402
import deform_cases as dc  # noqa: E402
import kpconv_modes_cases as kc  # noqa: E402
from superpoints_registration_amd import synthetic  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden")
KP_SEED = 5


def operator_fixture(blocks):
    go = kc.golden_go()
    fx = {}
    for modulated in (False, True):
        probe = dc.golden_case(modulated)
        n_kp, cin, cout = probe["w"].shape
        np.random.seed(KP_SEED)                     # the same kernel points with and without modulation
        conv = blocks.KPConv(n_kp, 3, cin, cout, probe["extent"], dc.GOLDEN_R / 2, deformable=True, modulated=modulated)
        with torch.no_grad():
            conv.weights.copy_(probe["w"])
            conv.offset_conv.weights.copy_(probe["off_w"])
            conv.offset_bias.copy_(probe["off_b"])
        kp, off_kp = conv.kernel_points.detach().clone(), conv.offset_conv.kernel_points.detach().clone()
        assert not torch.equal(kp, off_kp), "the offset convolution draws its own kernel points"
        for key, val in (("kp", kp), ("off_kp", off_kp)):
            assert key not in fx or np.array_equal(fx[key], val.numpy())
            fx[key] = val.numpy()
        case = dc.golden_case(modulated, kp=kp, off_kp=off_kp)
        print("modulated" if modulated else "plain", dc.check_conditions(case))
        x = case["x"].clone().requires_grad_(True)
        out = conv(case["q"], case["s"], case["idx"].long(), x)
        out.backward(go)
        tag = "mod|" if modulated else "plain|"
        fx[tag + "out"] = out.detach().numpy()
        fx[tag + "dx"] = x.grad.numpy()
        fx[tag + "d_off_b"] = conv.offset_bias.grad.numpy()
        fx[tag + "min_d2"] = conv.min_d2.detach().numpy()
        fx[tag + "deformed_KP"] = conv.deformed_KP.detach().numpy()
        for name, g in (("dw", conv.weights.grad), ("d_off_w", conv.offset_conv.weights.grad)):
            g = g.reshape(-1)
            fx[tag + name + "|samples"] = g[::dc.GOLDEN_DW_STEP].numpy()
            fx[tag + name + "|norm"] = np.float64(g.double().norm())
        ref, aux, grads = dc.ref64(case, go)
        rel = lambda a, b: float((a.detach().double() - b).abs().max() / b.abs().max())
        print("  float64 restatement vs the reference: out %.2e dx %.2e dW %.2e offset dW %.2e d offset_bias %.2e min_d2 %.2e"
              % (rel(out, ref), rel(x.grad, grads["dx"]), rel(conv.weights.grad, grads["dw"]),
                 rel(conv.offset_conv.weights.grad, grads["d_off_w"]), rel(conv.offset_bias.grad, grads["d_off_b"]),
                 float(((conv.min_d2.detach().double() - aux["min_d2"]).abs() / aux["min_d2"]).max())))
    fx["extent"] = np.float64(dc.golden_case(False)["extent"])
    return fx


def encoder_fixture(ns):
    src, tgt = dc.encoder_clouds()
    fx = {"seed": np.int32(dc.ENCODER_SEED), "src": src, "tgt": tgt}
    pyramids = {}
    for name, (arch, modulated) in dc.ENCODER_ARCHS.items():
        cfg = ns["EasyDict"](ns["misc"].load_config(os.path.join(ref_harness.REF_SRC, "conf", "qk_regtr_full_3dmatch.yaml")))
        cfg.architecture, cfg.modulated = list(arch), modulated
        np.random.seed(0)
        torch.manual_seed(0)
        enc = ns["kpconv"].KPFEncoder(cfg, cfg.d_embed)
        synthetic.fill_parameters(enc, seed=dc.ENCODER_SEED)
        enc.eval()
        with torch.no_grad():
            meta = ns["kpconv"].Preprocessor(cfg)([torch.from_numpy(src), torch.from_numpy(tgt)])
            feats, _ = enc(torch.ones((meta["points"][0].shape[0], 1)), meta)
        fx[f"{name}|feats"] = feats.numpy()
        key = tuple(arch)                            # one stored pyramid per architecture (modulation does not move it)
        if key not in pyramids:
            pyramids[key] = name
            for l, pts in enumerate(meta["points"]):
                fx[f"{name}|points{l}"] = pts.numpy()
                fx[f"{name}|lens{l}"] = meta["stack_lengths"][l].numpy().astype(np.int32)
                for kind in ("neighbors", "pools"):
                    idx = meta[kind][l].numpy()
                    assert idx.max(initial=0) < 2 ** 15
                    fx[f"{name}|{kind}{l}"] = idx.astype(np.int16)
        fx[f"{name}|pyramid"] = np.str_(pyramids[key])
        print(name, [tuple(p.shape) for p in meta["points"]], [tuple(n.shape) for n in meta["neighbors"]],
              [tuple(n.shape) for n in meta["pools"]], "feats", tuple(feats.shape), "max %.3e" % float(feats.abs().max()))
    return fx


def main():
    if len(sys.argv) > 1:
        ref_harness.REF_SRC = sys.argv[1]
    ns = ref_harness.load()
    for name, fx in (("kpconv_deform.npz", operator_fixture(ns["blocks"])), ("deform_encoder.npz", encoder_fixture(ns))):
        out = os.path.join(GOLDEN, name)
        np.savez_compressed(out, **fx)
        size = os.path.getsize(out)
        print(name, size // 1024, "KB")
        assert size < 512 << 10, "the fixture is meant to stay under 512 KB"


if __name__ == "__main__":
    main()
