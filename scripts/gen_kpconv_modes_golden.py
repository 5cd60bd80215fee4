"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/kpconv_modes.npz by running the reference's own KPConv class
(models/backbone_kpconv/kpconv_blocks.py, loaded through oracle.ref_harness) in float32 on the CPU, forward and
backward, for the five mode combinations beside linear / sum.  Run from the repo root in the dev container:

    python scripts/gen_kpconv_modes_golden.py [reference src]

Inputs are tests/kpconv_modes_cases.golden_case() (regenerable from its seed, not stored) except the kernel points:
the reference draws them itself (load_kernels: the global numpy RNG, seeded here), so they are stored and the tests
read them from the file.  Per mode: the output and d x whole, every GOLDEN_DW_STEP-th entry of d W and its norm, for the
output gradient golden_go().
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
import kpconv_modes_cases as kc  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "kpconv_modes.npz")
RADIUS = 0.2
KP_SEED = 5


def main():
    if len(sys.argv) > 1:
        ref_harness.REF_SRC = sys.argv[1]
    blocks = ref_harness.load()["blocks"]
    case, go = kc.golden_case(), kc.golden_go()
    n_kp, cin, cout = case["w"].shape
    fx = {}
    for influence, aggregation in kc.NEW_MODES:
        np.random.seed(KP_SEED)                     # the same kernel points in every mode
        conv = blocks.KPConv(n_kp, 3, cin, cout, case["extent"], RADIUS, KP_influence=influence,
                             aggregation_mode=aggregation)
        with torch.no_grad():
            conv.weights.copy_(case["w"])
        kp = conv.kernel_points.detach().clone()
        if "kp" in fx:
            assert np.array_equal(fx["kp"], kp.numpy())
        fx["kp"] = kp.numpy()
        probe = dict(case, kp=kp)
        kc.check_conditions(probe)                  # the arg-min gap and the row sums, with the reference's kernel points
        x = case["x"].clone().requires_grad_(True)
        out = conv(case["q"], case["s"], case["idx"].long(), x)
        out.backward(go)
        tag = f"{influence}|{aggregation}|"
        fx[tag + "out"] = out.detach().numpy()
        fx[tag + "dx"] = x.grad.numpy()
        dw = conv.weights.grad.reshape(-1)
        fx[tag + "dw|samples"] = dw[::kc.GOLDEN_DW_STEP].numpy()     # 122 KB per mode whole: every 4th entry + the norm
        fx[tag + "dw|norm"] = np.float64(dw.double().norm())
        ref = kc.ref64(probe, influence, aggregation)
        print(tag, "max |out| %.3e, float64 restatement differs by %.2e of it" %
              (float(out.abs().max()), float((out.detach().double() - ref).abs().max() / ref.abs().max())))
    fx["extent"] = np.float64(case["extent"])
    np.savez_compressed(OUT, **fx)
    size = os.path.getsize(OUT)
    print(os.path.basename(OUT), size // 1024, "KB")
    assert size < 512 << 10, "the fixture is meant to stay at a few hundred KB"


if __name__ == "__main__":
    main()
