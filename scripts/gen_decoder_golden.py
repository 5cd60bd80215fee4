"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/decoder_3dmatch.npz by running the reference's Preprocessor ->
KPFEncoder -> KPFDecoder (models/backbone_kpconv/kpconv.py:22-168, loaded through oracle.ref_harness) on the 3DMatch
architecture + ['nearest_upsample', 'unary', 'nearest_upsample', 'unary'].  Run from the repo root in the dev container:

    python scripts/gen_decoder_golden.py [reference src]

The cases, what is kept whole and what is row-sampled (every 16th row of the big case's x_all; the small case whole) are
described in tests/decoder_cases.py, which also holds the seeds.  Weights are not stored: both sides draw them with
synthetic.fill_parameters(Backbone(encoder, decoder), seed); the file pins each decoder weight's norm and sum instead.

The script refuses a cloud seed at which some row's nearest coarse point is not unique: column 0 of every upsamples
matrix must lie strictly nearer than column 1 (float64 distances), so that the order of equal distances cannot enter
the end-to-end test.  It then tries the next seed.
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
from oracle.gen_golden import grad_sample_indices  # noqa: E402
from superpoints_registration_amd import synthetic  # noqa: E402
import decoder_cases as dc  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "decoder_3dmatch.npz")


def ref_config(ns, use_batch_norm=True):
    cfg = ref_harness._EasyDict(ns["misc"].load_config(os.path.join(ref_harness.REF_SRC, "conf",
                                                                     "qk_regtr_full_3dmatch.yaml")))
    cfg.architecture = list(cfg.architecture) + dc.DECODER
    cfg.use_batch_norm = use_batch_norm
    return cfg


def backbone(ns, cfg, reduce=True):
    kp = ns["kpconv"]
    enc = kp.KPFEncoder(cfg, cfg.d_embed)
    dec = kp.KPFDecoder(cfg, enc.encoder_skip_dims[-1], enc.encoder_skip_dims, reduce_channel_when_upsample=reduce)
    model = dc.Backbone(enc, dec)
    synthetic.fill_parameters(model, seed=dc.SEED)
    return model


def nearest_is_unique(meta):
    for l in range(len(meta["points"]) - 1):
        up = meta["upsamples"][l].numpy()
        fine, coarse = meta["points"][l].double().numpy(), meta["points"][l + 1].double().numpy()
        if up.shape[1] < 2:
            continue
        d0 = ((fine - coarse[up[:, 0]]) ** 2).sum(1)
        has1 = up[:, 1] < coarse.shape[0]
        d1 = ((fine - coarse[np.where(has1, up[:, 1], 0)]) ** 2).sum(1)
        if (up[:, 0] >= coarse.shape[0]).any() or not (d0[has1] < d1[has1]).all():
            return False
    return True


def run(ns, case, cloud_seed):
    cfg = ref_config(ns)
    pts = [torch.from_numpy(c) for c in dc.clouds(case, cloud_seed)]
    meta = ns["kpconv"].Preprocessor(cfg)(pts)
    if not nearest_is_unique(meta):
        return None
    model = backbone(ns, cfg).eval()
    feats = torch.ones((meta["points"][0].shape[0], 1))
    with torch.no_grad():
        x, skips = model.encoder(feats, meta)
    return cfg, meta, model, x, skips


def bookkeeping(ns):
    """Constructor bookkeeping of the three shipped architectures + decoder, both channel rules."""
    fx = {}
    for tag in ("3dmatch", "kitti", "modelnet"):
        cfg = ref_harness._EasyDict(ns["misc"].load_config(os.path.join(ref_harness.REF_SRC, "conf",
                                                                         f"qk_regtr_full_{tag}.yaml")))
        levels = sum("strided" in b or "pool" in b for b in cfg.architecture)
        cfg.architecture = list(cfg.architecture) + ["nearest_upsample", "unary"] * levels
        for reduce in (True, False):
            m = backbone(ns, cfg, reduce)
            k = f"book|{tag}|{int(reduce)}|"
            fx[k + "skips"] = np.asarray(m.encoder.encoder_skips, np.int32)
            fx[k + "skip_dims"] = np.asarray(m.encoder.encoder_skip_dims, np.int32)
            fx[k + "concats"] = np.asarray(m.decoder.decoder_concats, np.int32)
            fx[k + "reprs"] = np.array([repr(b) for b in m.decoder.decoder_blocks])
            fx[k + "keys"] = np.array(list(m.decoder.state_dict().keys()))
            fx[k + "dims"] = np.asarray([[b.in_dim, b.out_dim] for b in m.decoder.decoder_blocks
                                         if hasattr(b, "in_dim")], np.int32)
    return fx


def main():
    if len(sys.argv) > 1:
        ref_harness.REF_SRC = sys.argv[1]
    ns = ref_harness.load()
    fx = {"seed": np.int32(dc.SEED), "row_step": np.int32(dc.ROW_STEP)}
    fx.update(bookkeeping(ns))

    # ---- big: end to end from points, outputs row-sampled ---------------------------------------------------------
    for cloud_seed in range(16):
        got = run(ns, "big", cloud_seed)
        if got is not None:
            break
        print("big: cloud seed", cloud_seed, "has a tied nearest coarse point")
    else:
        raise RuntimeError("no cloud seed with unique nearest coarse points")
    cfg, meta, model, x, skips = got
    with torch.no_grad():
        _, x_all = model.decoder(x, list(skips), meta)
    fx["big|cloud_seed"] = np.int32(cloud_seed)
    fx["big|rows"] = np.asarray([p.shape[0] for p in meta["points"]], np.int32)
    for l in range(len(meta["points"])):
        fx[f"big|lens{l}"] = meta["stack_lengths"][l].numpy().astype(np.int32)
    for l in range(len(meta["points"]) - 1):
        fx[f"big|up0_{l}"] = meta["upsamples"][l][:, 0].numpy().astype(np.int32)
    for j, y in enumerate(x_all):
        fx[f"big|x_all{j}|rows"] = y[dc.sample_rows(y.shape[0])].numpy()
        fx[f"big|x_all{j}|max"] = np.float64(y.abs().max())
    fx["big|enc_out|stats"] = np.array([x.mean(), x.abs().mean(), x.abs().max()], np.float64)
    for name, p in model.decoder.state_dict().items():
        fx[f"weight|{name}|norm"] = np.float64(p.double().norm())
        fx[f"weight|{name}|sum"] = np.float64(p.double().sum())
    fx["state_dict_keys"] = np.array(list(model.decoder.state_dict().keys()))
    print("big: rows per level", fx["big|rows"], "cloud seed", cloud_seed)

    # ---- small: everything whole, gradients ---------------------------------------------------------------------------
    for cloud_seed in range(16):
        got = run(ns, "small", cloud_seed)
        if got is not None:
            break
    else:
        raise RuntimeError("no cloud seed with unique nearest coarse points (small)")
    cfg, meta, model, x, skips = got
    fx["small|cloud_seed"] = np.int32(cloud_seed)
    for l in range(len(meta["points"])):
        fx[f"small|points{l}"] = meta["points"][l].numpy()
        fx[f"small|lens{l}"] = meta["stack_lengths"][l].numpy().astype(np.int32)
    for l in range(len(meta["points"]) - 1):
        fx[f"small|upsamples{l}"] = meta["upsamples"][l].numpy().astype(np.int32)
    x = x.detach().clone().requires_grad_(True)
    skips = [s.detach().clone().requires_grad_(True) for s in skips]
    fx["small|enc_out"] = x.detach().numpy()
    for l, s in enumerate(skips):
        fx[f"small|skip{l}"] = s.detach().numpy()
    model.train()      # InstanceNorm1d without running statistics: same arithmetic as eval
    _, x_all = model.decoder(x, list(skips), meta)
    loss = 0
    for j, y in enumerate(x_all):
        fx[f"small|x_all{j}"] = y.detach().numpy()
        loss = loss + (y * synthetic.rand(y.shape, dc.G_SEED + j)).sum()
    model.zero_grad(set_to_none=True)
    loss.backward()
    fx["small|grad|enc_out"] = x.grad.numpy()
    for l, s in enumerate(skips):
        fx[f"small|grad|skip{l}"] = s.grad.numpy()
    for name, p in model.decoder.named_parameters():
        g = p.grad.detach().reshape(-1).numpy()
        fx[f"small|grad|{name}|samples"] = g[grad_sample_indices(name, g.size, k=dc.W_SAMPLES)]
        fx[f"small|grad|{name}|norm"] = np.float64(np.linalg.norm(g.astype(np.float64)))
    print("small: rows per level", [p.shape[0] for p in meta["points"]], "cloud seed", cloud_seed)

    # ---- small, use_batch_norm: False (learnable bias instead of the norm) ---------------------------------------------
    cfg_b = ref_config(ns, use_batch_norm=False)
    model_b = backbone(ns, cfg_b).eval()
    with torch.no_grad():
        _, x_all_b = model_b.decoder(x.detach(), [s.detach() for s in skips], meta)
    for j, y in enumerate(x_all_b):
        fx[f"small|bias|x_all{j}"] = y.numpy()
    fx["bias|state_dict_keys"] = np.array(list(model_b.decoder.state_dict().keys()))

    np.savez_compressed(OUT, **fx)
    size = os.path.getsize(OUT)
    print(os.path.basename(OUT), size // 1024, "KB")
    assert size < 1 << 20, "the fixture must stay under 1 MiB: raise ROW_STEP"


if __name__ == "__main__":
    main()
