"""TEST INFRASTRUCTURE ONLY -- writes the circle feature loss fixtures by running the reference
(models/losses/feature_loss.py:160-243 CircleLossFull and models/qk_regtr_full.py with
feature_loss_type: circle, loaded through oracle.ref_harness).  Run from the repo root in the dev
container:

    python scripts/gen_circle_loss_golden.py

tests/golden/circle_ops.npz             op-level cases: inputs, the reference's per-pair losses and the
                                        input gradients of sum(pair losses) / B, all in float64
tests/golden/circle_grad_3dmatch_b2.npz a 3DMatch B = 2 training step with feature_loss_type: circle --
                                        losses and per-parameter gradients in the grad_*_b2.npz layout
tests/golden/circle_state_dict_3dmatch.npz
                                        the reference circle model's state_dict() key list

Keypoints of the op cases sit on a lattice of spacing H (the pose is a lattice symmetry), so every
squared distance is an integer multiple of H^2 and keeps a margin of >= 5e-4 from r_p and r_n:
direct differences and torch.cdist then classify every entry the same way.
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
H = 0.047                      # lattice spacing: (0.2 / H)^2 = 18.1, (0.4 / H)^2 = 72.4
R_P, R_N = 0.2, 0.4
POSE = np.array([[0.0, -1.0, 0.0, 3 * H], [1.0, 0.0, 0.0, -2 * H], [0.0, 0.0, 1.0, H]])   # 90 deg about z

# name -> (src lengths, tgt lengths, D, feature kind, feature scale)
CASES = {
    "ln": ((48, 40), (36, 56), 256, "ln", 1.0),            # LayerNorm-scale: fd ~ 22, logits in the thousands
    "small": ((60, 44), (52, 64), 32, "near", 0.35),       # fd in [0, 3]: pos below 0.1, active negs, zero weights
    "ragged": ((1, 50, 33), (37, 23, 64), 32, "near", 0.35),   # B = 3, N != M, a 1-row cloud (its col_sel is empty)
    "tiny": ((40,), (30,), 32, "near", 1e-3),
    "huge": ((40,), (30,), 32, "near", 1e3),
    "nosel": ((20, 30), (25, 18), 32, "near", 0.35),       # pair 0 has no positive at all -> NaN
}


def se3(pose, x):
    return x @ pose[:3, :3].T + pose[:3, 3]


def case_inputs(name, seed):
    src_lens, tgt_lens, D, kind, scale = CASES[name]
    rng = np.random.default_rng(seed)
    fs, ft, xs, xt = [], [], [], []
    for b, (n, m) in enumerate(zip(src_lens, tgt_lens)):
        K = 12
        ps = rng.integers(0, K, size=(n, 3)).astype(np.float64)
        if name == "nosel" and b == 0:
            pt = rng.integers(0, K, size=(m, 3)).astype(np.float64) + 40.0    # every target far away
        else:
            pt = rng.integers(0, K, size=(m, 3)).astype(np.float64)
        a = rng.standard_normal((n, D))
        t = rng.standard_normal((m, D))
        if kind == "ln":
            a = (a - a.mean(1, keepdims=True)) / a.std(1, keepdims=True)
            t = (t - t.mean(1, keepdims=True)) / t.std(1, keepdims=True)
        else:
            a, t = a * 0.3, t * 0.3
        # a third of the targets sit on a (transformed) source point with a near-copy of its feature
        xa = np.rint(se3(POSE, ps * H) / H)                                 # source points after pose_gt (lattice units)
        if not (name == "nosel" and b == 0):
            k = m // 3
            pick = rng.integers(0, n, size=k)
            pt[:k] = xa[pick]
            t[:k] = a[pick] + 0.02 * rng.standard_normal((k, D))
        fs.append((a * scale).astype(np.float32))
        ft.append((t * scale).astype(np.float32))
        xs.append((ps * H).astype(np.float32))
        xt.append((pt * H).astype(np.float32))
    return fs, ft, xs, xt


def radius_margin(xs, xt):
    m = np.inf
    for s, t in zip(xs, xt):
        cd = np.linalg.norm(se3(POSE, s.astype(np.float64))[:, None] - t.astype(np.float64)[None], axis=-1)
        m = min(m, np.abs(cd - R_P).min(), np.abs(cd - R_N).min())
    return m


def gen_ops():
    ns = ref_harness.load()
    FL = __import__("models.losses.feature_loss", fromlist=["CircleLossFull"])
    crit = FL.CircleLossFull(dist_type="euclidean", r_p=R_P, r_n=R_N)
    pose = torch.from_numpy(POSE)
    fx = {"names": np.array(list(CASES)), "pose": POSE.astype(np.float32), "r_p": np.float64(R_P),
          "r_n": np.float64(R_N)}
    del ns
    for ci, name in enumerate(CASES):
        fs, ft, xs, xt = case_inputs(name, 100 + ci)
        assert radius_margin(xs, xt) >= 5e-4, name
        B = len(fs)
        a = [torch.from_numpy(f).double().requires_grad_(True) for f in fs]
        t = [torch.from_numpy(f).double().requires_grad_(True) for f in ft]
        xa = [se3(pose.double(), torch.from_numpy(x).double()) for x in xs]
        xb = [torch.from_numpy(x).double() for x in xt]
        pair = torch.stack([crit([a[b]], [t[b]], [xa[b]], [xb[b]]) for b in range(B)])   # forward of one pair = its loss
        loss = crit(a, t, xa, xb)                                                           # sum over pairs / B
        # gradients of the finite pairs' sum / B (a NaN pair's loss still has finite row- or column-gradients)
        pair.sum().div(B).backward() if torch.isfinite(pair).all() else \
            pair[torch.isfinite(pair)].sum().div(B).backward()
        for b in range(B):
            fx[f"{name}|src_feat{b}"], fx[f"{name}|tgt_feat{b}"] = fs[b], ft[b]
            fx[f"{name}|src_kp{b}"], fx[f"{name}|tgt_kp{b}"] = xs[b], xt[b]
            fx[f"{name}|d_src{b}"] = a[b].grad.numpy()
            fx[f"{name}|d_tgt{b}"] = t[b].grad.numpy()
        fx[f"{name}|B"] = np.int32(B)
        fx[f"{name}|pair"] = pair.detach().numpy()
        fx[f"{name}|loss"] = np.float64(loss.detach())
        print(name, "pair losses", pair.detach().numpy())
    path = os.path.join(OUT, "circle_ops.npz")
    np.savez_compressed(path, **fx)
    print(os.path.basename(path), os.path.getsize(path) // 1024, "KB")


def circle_model():
    """The reference RegTR (3DMatch config) with feature_loss_type: circle; CPU Preprocessor as in
    ref_harness.make_model."""
    ns = ref_harness.load_regtr()
    cfg = ref_harness._EasyDict(ns["misc"].load_config(os.path.join(ref_harness.REF_SRC, "conf",
                                                                     "qk_regtr_full_3dmatch.yaml")))
    cfg.feature_loss_type = "circle"
    np.random.seed(0)
    torch.manual_seed(0)
    model = ns["regtr"].RegTR(cfg)
    model.preprocessor = ns["kpconv"].Preprocessor(cfg)
    return model, cfg


def gen_grad(B=2):
    """oracle.gen_golden.gen_grad with the circle feature loss."""
    model, cfg = circle_model()
    np.savez_compressed(os.path.join(OUT, "circle_state_dict_3dmatch.npz"),
                        keys=np.array(list(model.state_dict().keys())))
    synthetic.fill_parameters(model, seed=0)
    model.train()
    pairs, sizes = pairs_for("3dmatch", B)
    src = [p[0][:n] for p, (n, m) in zip(pairs, sizes)]
    tgt = [p[1][:m] for p, (n, m) in zip(pairs, sizes)]
    pose, src_ov, tgt_ov = loss_inputs("3dmatch", B)
    batch = {"src_xyz": [torch.from_numpy(s) for s in src], "tgt_xyz": [torch.from_numpy(t) for t in tgt],
             "pose": torch.from_numpy(pose),
             "src_overlap": [torch.from_numpy(o) for o in src_ov],
             "tgt_overlap": [torch.from_numpy(o) for o in tgt_ov]}
    out = model(batch)
    losses = model.compute_loss(out, batch)
    # how close the coarse keypoints come to the radii (direct differences vs torch.cdist)
    marg = np.inf
    for b in range(B):
        xa = se3(pose[b].astype(np.float64), out["src_kp"][b].detach().double().numpy())
        cd = np.linalg.norm(xa[:, None] - out["tgt_kp"][b].detach().double().numpy()[None], axis=-1)
        marg = min(marg, np.abs(cd - cfg.r_p).min(), np.abs(cd - cfg.r_n).min())
    fx = {"B": np.int32(B), "seed": np.int32(0), "radius_margin": np.float64(marg)}
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
            if g.size <= 4096:
                fx[f"{tag}|{name}|full"] = g.astype(np.float32)
    path = os.path.join(OUT, f"circle_grad_3dmatch_b{B}.npz")
    np.savez_compressed(path, **fx)
    print(os.path.basename(path), os.path.getsize(path) // 1024, "KB", {k: float(v) for k, v in losses.items()},
          "radius margin", marg)


if __name__ == "__main__":
    what = sys.argv[1:] or ["ops", "grad"]
    if "ops" in what:
        gen_ops()
    if "grad" in what:
        gen_grad()
