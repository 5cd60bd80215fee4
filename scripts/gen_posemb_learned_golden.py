"""TEST INFRASTRUCTURE ONLY -- writes the learned positional embedding fixtures by running the reference
(models/transformer/position_embedding.py:53-72 PositionEmbeddingLearned and models/qk_regtr_full.py with
pos_emb_type: learned, loaded through oracle.ref_harness).  Run from the repo root in the dev container:

    python scripts/gen_posemb_learned_golden.py

tests/golden/posemb_learned_ops.npz         op-level cases in float64: the module's ten parameters at torch's default
                                            init (seeded), per case the coordinates, the factor every parameter is
                                            multiplied by (the product rounded to float32 is what both sides use), the
                                            reference module's output; for the first case also an upstream gradient
                                            and the parameter gradients (whole tensors up to 4 096 entries, else norm,
                                            sum and pinned entries, as the grad_*_b2.npz fixtures do)
tests/golden/regtr_3dmatch_learned_b2.npz   the reference forward on the 3DMatch B = 2 golden pairs with the learned
                                            embedding, in the layout of regtr_3dmatch_b2.npz minus the pyramid and
                                            encoder-stage arrays (they do not depend on the embedding and are pinned by
                                            regtr_3dmatch_b2.npz), plus the state_dict() key list and shapes
tests/golden/grad_3dmatch_learned_b2.npz    a training step's losses and parameter gradients, layout of grad_3dmatch_b2.npz
                                            (whole tensors up to 1 024 entries instead of 4 096, so that the file with
                                            its ten extra tensors stays within that one's size)
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import ref_harness  # noqa: E402
from oracle.gen_golden import grad_sample_indices, loss_inputs, pairs_for  # noqa: E402
from superpoints_registration_amd import synthetic  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
PARAM_NAMES = [f"mlp.{i}.{leaf}" for i in (0, 2, 4, 6, 8) for leaf in ("weight", "bias")]

# name -> (tokens, coordinate magnitude, parameter factor)
OPS_CASES = {
    "default": (65, 1.0, 1.0),
    "kitti": (17, 80.0, 1.0),
    "w30": (9, 1.0, 30.0),
    "tiny": (1, 1e-3, 1e-3),
}
GRAD_CASE = "default"


def scaled_params(base, factor):
    """float32(base * factor) as float64: the parameters both the reference module and the kernel are handed."""
    return [torch.from_numpy((np.asarray(b, np.float64) * factor).astype(np.float32)).double() for b in base]


def gen_ops():
    ns = ref_harness.load()
    torch.manual_seed(0)
    module = ns["posemb"].PositionEmbeddingLearned(3, 256)
    base = [module.state_dict()[n].detach().double().numpy() for n in PARAM_NAMES]
    module = module.double()
    fx = {"names": np.array(list(OPS_CASES)), "param_names": np.array(PARAM_NAMES), "grad_case": np.array(GRAD_CASE)}
    for n, b in zip(PARAM_NAMES, base):
        fx[f"param|{n}"] = b
    for ci, (name, (T, mag, factor)) in enumerate(OPS_CASES.items()):
        xyz = (synthetic.rand((T, 3), 300 + ci).double() * mag).float().double()
        params = scaled_params(base, factor)
        module.load_state_dict(dict(zip(PARAM_NAMES, params)), strict=True)
        module.zero_grad(set_to_none=True)
        out = module(xyz)
        fx[f"{name}|xyz"], fx[f"{name}|factor"], fx[f"{name}|out"] = xyz.numpy(), np.float64(factor), out.detach().numpy()
        if name == GRAD_CASE:
            g = torch.Generator().manual_seed(77)
            dpe = torch.randint(-8, 9, (T, 256), generator=g).double() / 8.0      # eighths: exact, small on disk
            out.backward(dpe)
            fx[f"{name}|dpe"] = dpe.numpy()
            for n, p in module.named_parameters():
                gr = p.grad.detach().reshape(-1).numpy()
                fx[f"{name}|grad|{n}|norm"] = np.float64(np.linalg.norm(gr))
                fx[f"{name}|grad|{n}|sum"] = np.float64(gr.sum())
                fx[f"{name}|grad|{n}|samples"] = gr[grad_sample_indices(n, gr.size, k=256)]
                if gr.size <= 4096:
                    fx[f"{name}|grad|{n}|full"] = gr.copy()
        print(name, "T", T, "max |out|", float(out.detach().abs().max()))
    path = os.path.join(OUT, "posemb_learned_ops.npz")
    np.savez_compressed(path, **fx)
    print(os.path.basename(path), os.path.getsize(path) // 1024, "KB")


def learned_model():
    """The reference RegTR (3DMatch config) with pos_emb_type: learned; CPU Preprocessor as in ref_harness.make_model."""
    ns = ref_harness.load_regtr()
    cfg = ref_harness._EasyDict(ns["misc"].load_config(os.path.join(ref_harness.REF_SRC, "conf",
                                                                     "qk_regtr_full_3dmatch.yaml")))
    cfg.pos_emb_type = "learned"
    np.random.seed(0)
    torch.manual_seed(0)
    model = ns["regtr"].RegTR(cfg)
    model.preprocessor = ns["kpconv"].Preprocessor(cfg)
    return model, cfg


def golden_batch(B, with_loss):
    pairs, sizes = pairs_for("3dmatch", B)
    batch = {"src_xyz": [torch.from_numpy(p[0][:n]) for p, (n, m) in zip(pairs, sizes)],
             "tgt_xyz": [torch.from_numpy(p[1][:m]) for p, (n, m) in zip(pairs, sizes)]}
    if with_loss:
        pose, src_ov, tgt_ov = loss_inputs("3dmatch", B)
        batch.update(pose=torch.from_numpy(pose), src_overlap=[torch.from_numpy(o) for o in src_ov],
                     tgt_overlap=[torch.from_numpy(o) for o in tgt_ov])
    else:
        batch["pose"] = torch.eye(4)[None, :3].repeat(B, 1, 1)
    return batch, sizes


MATCH_MARGIN = 1e-4     # the features are gated at 1e-4 of their scale


def match_margin(out, B):
    """Smallest relative gap between a match's dual-softmax value and its runner-up (float64, from the reference's own
    features): how far the reference's arg-max is from a tie."""
    worst = np.inf
    for b in range(B):
        fs, ft = out["src_feat"][b][0].double(), out["tgt_feat"][b][0].double()
        c = fs @ ft.t() / fs.shape[1] ** 0.5
        a = torch.softmax(c, 0) * torch.softmax(c, 1)
        top = torch.topk(a, 2, dim=0 if a.shape[0] > a.shape[1] else 1).values
        top = top.t() if a.shape[0] > a.shape[1] else top
        worst = min(worst, float(((top[:, 0] - top[:, 1]) / top[:, 0]).min()))
    return worst


def gen_regtr(B=2):
    """oracle.gen_golden.gen_regtr with the learned embedding, without the pyramid / encoder-stage arrays.  With 77
    matches per pair the 99 % arg-max gate tolerates no flip, so the weights' seed is the first one at which the
    reference itself decides every match by a relative margin of at least MATCH_MARGIN (seed 0 leaves one match tied
    to 1e-5: the reference's own float32 arg-max then differs from the float64 arg-max of its own features)."""
    model, cfg = learned_model()
    sd = model.state_dict()
    keys = list(sd.keys())
    shapes = np.full((len(keys), 4), -1, np.int64)
    for i, k in enumerate(keys):
        shapes[i, :sd[k].dim()] = list(sd[k].shape)
    model.eval()
    for seed in range(16):
        synthetic.fill_parameters(model, seed=seed)
        batch, sizes = golden_batch(B, with_loss=False)
        with torch.no_grad():
            out = model(batch)
        margin = match_margin(out, B)
        print("seed", seed, "match margin", margin)
        if margin >= MATCH_MARGIN:
            break
    else:
        raise RuntimeError("no seed with decided matches")
    fx = {"B": np.int32(B), "seed": np.int32(seed), "match_margin": np.float64(margin), "sizes": np.asarray(sizes, np.int32),
          "state_dict_keys": np.array(keys), "state_dict_shapes": shapes, "pose": out["pose"].numpy()}
    for b in range(B):
        fx[f"src_feat{b}"] = out["src_feat"][b][0].numpy()
        fx[f"tgt_feat{b}"] = out["tgt_feat"][b][0].numpy()
        fx[f"src_overlap{b}"] = out["src_overlap"][b][0, :, 0].numpy()
        fx[f"tgt_overlap{b}"] = out["tgt_overlap"][b][0, :, 0].numpy()
        fx[f"val{b}"] = out["overlap_prob_list"][b].numpy()
        fx[f"ind{b}"] = out["ind_list"][b].numpy().astype(np.int32)
    path = os.path.join(OUT, f"regtr_3dmatch_learned_b{B}.npz")
    np.savez_compressed(path, **fx)
    print(os.path.basename(path), os.path.getsize(path) // 1024, "KB", "pose", out["pose"][0, :, 3].numpy())


def gen_grad(B=2):
    """oracle.gen_golden.gen_grad with the learned embedding, on the weights of the forward fixture."""
    seed = int(np.load(os.path.join(OUT, f"regtr_3dmatch_learned_b{B}.npz"))["seed"])
    model, cfg = learned_model()
    synthetic.fill_parameters(model, seed=seed)
    model.train()
    batch, _ = golden_batch(B, with_loss=True)
    out = model(batch)
    losses = model.compute_loss(out, batch)
    fx = {"B": np.int32(B), "seed": np.int32(seed)}
    for k, v in losses.items():
        fx[f"loss_{k}"] = np.float64(float(v))
    for tag, loss in (("fo", 0.1 * losses["feature"] + losses["overlap"]), ("total", losses["total"])):
        model.zero_grad(set_to_none=True)
        loss.backward(retain_graph=True)
        for name, p in model.named_parameters():
            if p.grad is None:
                fx[f"{tag}|{name}|none"] = np.int32(1)
                continue
            g = p.grad.detach().double().reshape(-1).numpy()
            fx[f"{tag}|{name}|norm"] = np.float64(np.linalg.norm(g))
            fx[f"{tag}|{name}|sum"] = np.float64(g.sum())
            fx[f"{tag}|{name}|samples"] = g[grad_sample_indices(name, g.size)].astype(np.float32)
            if g.size <= 1024:     # grad_3dmatch_b2.npz keeps whole tensors up to 4 096: the ten new tensors fit its size this way
                fx[f"{tag}|{name}|full"] = g.astype(np.float32)
    path = os.path.join(OUT, f"grad_3dmatch_learned_b{B}.npz")
    np.savez_compressed(path, **fx)
    print(os.path.basename(path), os.path.getsize(path) // 1024, "KB", {k: float(v) for k, v in losses.items()})


if __name__ == "__main__":
    what = sys.argv[1:] or ["ops", "regtr", "grad"]
    if "ops" in what:
        gen_ops()
    if "regtr" in what:
        gen_regtr()
    if "grad" in what:
        gen_grad()
