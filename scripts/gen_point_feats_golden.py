"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/point_feats.npz by running the reference's own KPFEncoder
(models/backbone_kpconv/kpconv.py, loaded through oracle.ref_harness) with the 3DMatch config and in_feats_dim = 4 on
its CPU Preprocessor, in float32, forward and backward, for one small pair.  Run from the repo root in the dev
container:

    python scripts/gen_point_feats_golden.py [reference src]

Inputs are tests/point_feats_cases.golden_inputs() / golden_cotangent() (regenerable from their seeds, not stored).
Parameters are synthetic.fill_parameters(encoder, GOLDEN_SEED), which overwrites the kernel points the reference drew
as well; the first block's are stored so that the test can see that its model holds the same.  Stored: the encoder's
un-projected output, the first block's weight gradient whole, and for every other parameter the gradient's norm and 64
pinned entries.
"""
import copy
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_harness  # noqa: E402
import point_feats_cases as pc  # noqa: E402
from superpoints_registration_amd import synthetic  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "point_feats.npz")
FIRST = "encoder_blocks.0.KPConv.weights"


def main():
    if len(sys.argv) > 1:
        ref_harness.REF_SRC = sys.argv[1]
    ns = ref_harness.load()
    cfg = ns["EasyDict"](ns["misc"].load_config(os.path.join(ref_harness.REF_SRC, "conf", "qk_regtr_full_3dmatch.yaml")))
    cfg.in_feats_dim = pc.GOLDEN_C
    np.random.seed(0)
    torch.manual_seed(0)
    enc = ns["kpconv"].KPFEncoder(cfg, cfg.d_embed)
    pre = ns["kpconv"].Preprocessor(cfg)
    synthetic.fill_parameters(enc, seed=pc.GOLDEN_SEED)
    enc.train()
    assert tuple(dict(enc.named_parameters())[FIRST].shape) == (15, pc.GOLDEN_C, 64)

    src, tgt, fs, ft = pc.golden_inputs()
    for f in (fs, ft):
        pc.check_conditions(f)
    with torch.no_grad():
        meta = pre([torch.from_numpy(src), torch.from_numpy(tgt)])
    x = torch.from_numpy(np.concatenate([fs, ft]))
    assert x.shape[0] == meta["points"][0].shape[0], "level 0 is the input cloud"
    out, _ = enc(x, meta)
    go = pc.golden_cotangent(out.shape)
    out.backward(go)

    fx = {"seed": np.int32(pc.GOLDEN_SEED), "feats_un": out.detach().numpy(),
          "kernel_points0": enc.encoder_blocks[0].KPConv.kernel_points.detach().numpy(),
          "lens": np.asarray([int(v) for v in meta["stack_lengths"][-1]], np.int32)}
    for name, p in enc.named_parameters():
        if p.grad is None:
            fx[f"{name}|none"] = np.int32(1)
            continue
        g = p.grad.detach().double().reshape(-1).numpy()
        fx[f"{name}|norm"] = np.float64(np.linalg.norm(g))
        if name == FIRST:
            fx[f"{name}|full"] = g.astype(np.float32)
        else:
            fx[f"{name}|samples"] = g[pc.grad_sample_indices(name, g.size)].astype(np.float32)

    # the same modules in float64 on the same float32 inputs: how far float32 itself is from the exact result
    enc64 = copy.deepcopy(enc).double()
    meta64 = dict(meta, points=[p.double() for p in meta["points"]])
    with torch.no_grad():
        out64, _ = enc64(x.double(), meta64)
    print("max |out| %.3e, the float64 evaluation differs by %.2e of it" %
          (float(out.detach().abs().max()), float((out.detach().double() - out64).abs().max() / out64.abs().max())))
    np.savez_compressed(OUT, **fx)
    size = os.path.getsize(OUT)
    print(os.path.basename(OUT), size // 1024, "KB", [tuple(p.shape) for p in meta["points"]], "out", tuple(out.shape))
    assert size < 512 << 10, "the fixture is meant to stay at a few hundred KB"


if __name__ == "__main__":
    main()
