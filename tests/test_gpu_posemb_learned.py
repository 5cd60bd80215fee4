"""GPU: the learned positional embedding (pos_emb_type 'learned') -- the fused MLP kernel spr_posemb_mlp and its
backward against float64 torch on the CPU and the reference module's own results
(tests/golden/posemb_learned_ops.npz), the gradient LayerNormFn now hands to `pos`, and the whole model against the
reference forward / training step with the learned embedding (regtr_3dmatch_learned_b2.npz,
grad_3dmatch_learned_b2.npz; scripts/gen_posemb_learned_golden.py).

Criterion of the operator tests (tests/test_gpu_range.py): err <= max(1e-5 max|ref|, 4 err32) against float64 --
1e-5 = five layers at the 2e-6 one linear is held to there, err32 = the error of a plain float32 torch evaluation of
the same MLP on the CPU (amplification through the later layers)."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle.gen_golden import grad_sample_indices, loss_inputs, pairs_for
from superpoints_registration_amd import get_config, ops, synthetic
from superpoints_registration_amd.regtr import RegTR

pytestmark = pytest.mark.gpu

TILE = 64                                   # tokens per workgroup of the forward kernel (csrc/posemb_mlp.hip)
T_SET = (0, 1, TILE - 1, TILE, TILE + 1, 200)
TOL = 1e-5
TAU = 1e-4                                  # 10 x TOL: tokens with a pre-activation this close to zero carry no gradient


@pytest.fixture(scope="module")
def gold():
    return load_golden("posemb_learned_ops.npz")


def _params(gold, factor=1.0):
    """The reference module's default-init parameters times `factor`, rounded to float32 (what the fixtures used)."""
    return [torch.from_numpy((gold[f"param|{n}"] * factor).astype(np.float32)) for n in gold["param_names"]]


def _mlp(xyz, params, pre=None):
    """The MLP in the dtype of its arguments; pre (a list) receives the four pre-activations."""
    h = xyz
    for l in range(5):
        h = h @ params[2 * l].t() + params[2 * l + 1]
        if l < 4:
            if pre is not None:
                pre.append(h.detach())
            h = torch.relu(h)
    return h


def _xyz(T, mag, seed):
    return synthetic.rand((T, 3), seed) * mag


def _check(got, ref64, ref32, what):
    assert torch.isfinite(got).all(), what
    scale = float(ref64.abs().max()) if ref64.numel() else 0.0
    err = float((got.double() - ref64).abs().max()) if ref64.numel() else 0.0
    err32 = float((ref32.double() - ref64).abs().max()) if ref64.numel() else 0.0
    print(f"{what}: err {err:.3e}  fp32 {err32:.3e}  scale {scale:.3e}")
    assert err <= max(TOL * scale, 4 * err32), f"{what}: {err:.3e} (fp32 {err32:.3e}, scale {scale:.3e})"


# ---- 1. forward ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [1e-3, 1.0, 30.0])
def test_forward_against_float64(device, gold, factor):
    params = _params(gold, factor)
    dparams = [p.to(device) for p in params]
    p64 = [p.double() for p in params]
    for T in T_SET:
        for mi, mag in enumerate((1e-3, 1.0, 80.0, 1e3)):
            xyz = _xyz(T, mag, 500 + 10 * T + mi)
            got = ops.posemb_mlp(xyz.to(device), dparams)
            assert got.shape == (T, 256) and got.dtype == torch.float32
            _check(got.cpu(), _mlp(xyz.double(), p64), _mlp(xyz, params), f"T {T} |xyz| {mag:g} weights x{factor:g}")


def test_forward_against_the_reference_module(device, gold):
    for name in gold["names"]:
        params = _params(gold, float(gold[f"{name}|factor"]))
        xyz = torch.from_numpy(gold[f"{name}|xyz"]).float()
        got = ops.posemb_mlp(xyz.to(device), [p.to(device) for p in params])
        _check(got.cpu(), torch.from_numpy(gold[f"{name}|out"]), _mlp(xyz, params), f"golden case {name}")


def test_forward_with_a_dead_layer_is_the_last_bias(device, gold):
    params = _params(gold)
    params[7] = torch.full((256,), -1e3)                  # mlp.6.bias: every unit of layer 4 is dead
    xyz = _xyz(TILE + 1, 1.0, 7)
    got = ops.posemb_mlp(xyz.to(device), [p.to(device) for p in params]).cpu()
    assert torch.equal(got, params[9].expand(TILE + 1, 256))


def test_forward_rejects_what_the_kernel_is_not_built_for(device, gold):
    params = [p.to(device) for p in _params(gold)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.posemb_mlp(torch.zeros(4, 3), params)
    with pytest.raises(ValueError):
        ops.posemb_mlp(torch.zeros(4, 3, device=device), params[:8])
    bad = list(params)
    bad[8], bad[9] = torch.zeros(128, 256, device=device), torch.zeros(128, device=device)   # d_model 128
    with pytest.raises(ValueError):
        ops.posemb_mlp(torch.zeros(4, 3, device=device), bad)
    from superpoints_registration_amd import _lib
    import ctypes
    ptrs = (ctypes.c_void_p * 10)(*[p.data_ptr() for p in params])
    out = torch.empty(4, 128, device=device)
    rc = _lib.lib().spr_posemb_mlp(ops._ptr(torch.zeros(4, 3, device=device)), ptrs, 4, 128, ops._ptr(out), None)
    assert rc != 0 and b"d_model" in _lib.lib().spr_last_error()


# ---- 2. backward ---------------------------------------------------------------------------------------
# chosen on the CPU so that the float64 oracle alone zeroes at most 20 % of the rows (0, 8, 5, 6, 9 % with these)
BWD_SEEDS = {1: 1, TILE - 1: 6, TILE: 3, TILE + 1: 1, 200: 6}


def bwd_case(gold, T, seed, zero_rows=False):
    """Inputs of a backward case and the float64 oracle's verdict on them: xyz, params, dpe with the rows of every
    token zeroed that has a unit within TAU max|pre-activation of its layer| of zero (no ReLU mask can then decide
    anything), and the zeroed share."""
    params = _params(gold)
    xyz = _xyz(T, 1.0, 900 + 7 * T + seed)
    dpe = synthetic.rand((T, 256), 950 + T + seed)
    pre = []
    _mlp(xyz.double(), [p.double() for p in params], pre)
    near = torch.zeros(T, dtype=torch.bool)
    for z in pre:
        near |= (z.abs() < TAU * float(z.abs().max())).any(dim=1)
    dpe[near] = 0.0
    if zero_rows:
        dpe[::3] = 0.0
    return xyz, params, dpe, float(near.float().mean())


def _autograd(xyz, params, dpe, dtype):
    leaves = [p.detach().clone().to(dtype).requires_grad_(True) for p in params]
    _mlp(xyz.to(dtype), leaves).backward(dpe.to(dtype))
    return [p.grad for p in leaves]


def _ours(device, xyz, params, dpe):
    leaves = [p.detach().clone().to(device).requires_grad_(True) for p in params]
    ops.posemb_mlp(xyz.to(device), leaves).backward(dpe.to(device))
    return [p.grad for p in leaves]


@pytest.mark.parametrize("T", [t for t in T_SET if t > 0])
def test_backward_against_float64_autograd(device, gold, T):
    xyz, params, dpe, share = bwd_case(gold, T, BWD_SEEDS[T])
    assert share <= 0.2, share
    got = _ours(device, xyz, params, dpe)
    ref64, ref32 = _autograd(xyz, params, dpe, torch.float64), _autograd(xyz, params, dpe, torch.float32)
    for n, g, r64, r32 in zip(gold["param_names"], got, ref64, ref32):
        assert g.shape == r64.shape
        _check(g.cpu(), r64, r32, f"T {T} d {n} (zeroed rows {share:.2f})")


def test_backward_with_whole_zero_rows_and_twice_the_same_bits(device, gold):
    xyz, params, dpe, share = bwd_case(gold, 200, BWD_SEEDS[200], zero_rows=True)
    assert share <= 0.2
    a, b = _ours(device, xyz, params, dpe), _ours(device, xyz, params, dpe)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    ref64, ref32 = _autograd(xyz, params, dpe, torch.float64), _autograd(xyz, params, dpe, torch.float32)
    for n, g, r64, r32 in zip(gold["param_names"], a, ref64, ref32):
        _check(g.cpu(), r64, r32, f"zero rows d {n}")
    zero = _ours(device, xyz, params, torch.zeros_like(dpe))
    assert all(not g.any() for g in zero)


def test_backward_against_the_reference_module(device, gold):
    name = str(gold["grad_case"])
    params = _params(gold, float(gold[f"{name}|factor"]))
    xyz = torch.from_numpy(gold[f"{name}|xyz"]).float()
    dpe = torch.from_numpy(gold[f"{name}|dpe"]).float()
    got = _ours(device, xyz, params, dpe)
    ref32 = _autograd(xyz, params, dpe, torch.float32)
    for n, g, r32 in zip(gold["param_names"], got, ref32):
        g, r32 = g.cpu().reshape(-1), r32.reshape(-1)
        if f"{name}|grad|{n}|full" in gold:
            ref = torch.from_numpy(gold[f"{name}|grad|{n}|full"])
        else:
            idx = torch.from_numpy(grad_sample_indices(str(n), g.numel(), k=256))
            g, r32, ref = g[idx], r32[idx], torch.from_numpy(gold[f"{name}|grad|{n}|samples"])
        _check(g, ref, r32, f"golden d {n}")


# ---- 3. LayerNormFn hands pos its gradient --------------------------------------------------------------
def test_layernorm_passes_the_gradient_of_pos(device):
    x, g, b, p = synthetic.rand((65, 256), 5, -3, 5), synthetic.rand((256,), 6, 0.5, 1.5), synthetic.rand((256,), 7), \
        synthetic.rand((65, 256), 8)
    g1, g2 = synthetic.rand((65, 256), 9).to(device), synthetic.rand((65, 256), 10).to(device)

    def run(pos_grad):
        dx, dg, db = (t.clone().to(device).requires_grad_(True) for t in (x, g, b))
        dp = p.clone().to(device).requires_grad_(pos_grad)
        n, npos = ops.layernorm(dx, dg, db, 1e-5, pos=dp)
        (n * g1).sum().add((npos * g2).sum()).backward()
        return dx.grad, dg.grad, db.grad, dp.grad

    with_pos, without = run(True), run(False)
    assert torch.equal(with_pos[3], g2)                    # out_pos = LN(x) + pos: d pos = d out_pos, bit for bit
    assert without[3] is None
    for a, c in zip(with_pos[:3], without[:3]):
        assert torch.equal(a, c)


# ---- 4. end to end against the reference -------------------------------------------------------------------
def _batch(device, B, with_loss):
    pairs, sizes = pairs_for("3dmatch", B)
    batch = {"src_xyz": [torch.from_numpy(p[0][:n]).to(device) for p, (n, m) in zip(pairs, sizes)],
             "tgt_xyz": [torch.from_numpy(p[1][:m]).to(device) for p, (n, m) in zip(pairs, sizes)]}
    if with_loss:
        pose, src_ov, tgt_ov = loss_inputs("3dmatch", B)
        batch.update(pose=torch.from_numpy(pose).to(device), src_overlap=[torch.from_numpy(o).to(device) for o in src_ov],
                     tgt_overlap=[torch.from_numpy(o).to(device) for o in tgt_ov])
    return batch


def _model(device, seed, train=False):
    model = RegTR(get_config("3dmatch", pos_emb_type="learned"))
    synthetic.fill_parameters(model, seed=seed)
    model = model.to(device)
    return model.train() if train else model.eval()


def test_learned_model_matches_the_reference_forward(device):
    """The gates of test_gpu_regtr.py::test_regtr_matches_reference on the reference forward with the learned embedding."""
    g = load_golden("regtr_3dmatch_learned_b2.npz")
    B = int(g["B"])
    assert float(g["match_margin"]) >= 1e-4        # the fixture's own matches are decided (no tie at the features' gate)
    out = _model(device, int(g["seed"]))(_batch(device, B, False))
    assert out["pose"].shape == (B, 3, 4)
    for b in range(B):
        sf, tf = out["src_feat"][b][0].cpu().numpy(), out["tgt_feat"][b][0].cpu().numpy()
        scale = max(np.abs(g[f"src_feat{b}"]).max(), 1.0)
        print(f"pair {b}: feat {np.abs(sf - g[f'src_feat{b}']).max() / scale:.2e} {np.abs(tf - g[f'tgt_feat{b}']).max() / scale:.2e}")
        assert np.abs(sf - g[f"src_feat{b}"]).max() <= 1e-4 * scale
        assert np.abs(tf - g[f"tgt_feat{b}"]).max() <= 1e-4 * scale
        assert np.abs(out["src_overlap"][b][0, :, 0].cpu().numpy() - g[f"src_overlap{b}"]).max() < 1e-4
        assert (out["ind_list"][b].cpu().numpy() == g[f"ind{b}"]).mean() >= 0.99
        assert np.allclose(out["overlap_prob_list"][b].cpu().numpy(), g[f"val{b}"], rtol=5e-3, atol=1e-7)
        err = np.linalg.norm(out["pose"][b].cpu().numpy() - g["pose"][b])
        assert err < 1e-4, f"pose error {err:.2e}"


@pytest.mark.parametrize("which", ["fo", "total"])
def test_learned_model_gradients_match_the_reference(device, which):
    """A training step against the reference's own backward with the learned embedding, tolerances of
    test_gpu_backward.py::test_parameter_gradients_match_the_reference: outside the KPConv encoder -- the ten
    pos_embed.mlp.* tensors included, like feat_proj -- norm and pinned entries within 1e-4; encoder tensors norm 5e-4 and
    RMS 2e-2; the Sinkhorn scalars within the 1e-3 window against the reference (their float64 anchor needs the CPU
    oracle, which has no learned embedding)."""
    g = load_golden("grad_3dmatch_learned_b2.npz")
    model = _model(device, int(g["seed"]), train=True)
    batch = _batch(device, int(g["B"]), True)
    losses = model.compute_loss(model(batch), batch)
    loss = losses["total"] if which == "total" else 0.1 * losses["feature"] + losses["overlap"]
    model.zero_grad(set_to_none=True)
    loss.backward()
    for k in ("feature", "T", "overlap", "total"):
        assert abs(float(losses[k].detach()) - float(g[f"loss_{k}"])) <= 5e-5 * max(1.0, abs(float(g[f"loss_{k}"])))
    n_pos, report = 0, []
    for name, p in model.named_parameters():
        if f"{which}|{name}|none" in g:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, f"{name}: the reference has no gradient here"
            continue
        if not p.requires_grad:
            continue
        assert p.grad is not None, f"{name}: no gradient"
        gr = p.grad.detach().double().reshape(-1).cpu().numpy()
        ref_norm = float(g[f"{which}|{name}|norm"])
        if f"{which}|{name}|full" in g:
            ref_e, got_e = g[f"{which}|{name}|full"].astype(np.float64), gr
        else:
            ref_e = g[f"{which}|{name}|samples"].astype(np.float64)
            got_e = gr[grad_sample_indices(name, gr.size)]
        scale = max(np.abs(ref_e).max(), ref_norm / math.sqrt(gr.size), 1e-30)
        err = np.abs(got_e - ref_e).max() / scale
        rms = np.sqrt(np.mean((got_e - ref_e) ** 2)) / max(np.sqrt(np.mean(ref_e ** 2)), 1e-30)
        nerr = abs(np.linalg.norm(gr) - ref_norm) / max(ref_norm, 1e-30)
        report.append((err, name))
        if name in ("alpha", "beta"):
            assert nerr <= 1e-3, f"{which} {name}: deviates by {nerr:.2e}"
        elif name.startswith("kpf_encoder."):
            assert nerr <= 5e-4, f"{which} {name}: norm deviates by {nerr:.2e}"
            assert rms <= 2e-2, f"{which} {name}: RMS deviation {rms:.2e}"
        else:
            n_pos += name.startswith("pos_embed.mlp.")
            assert nerr <= 1e-4, f"{which} {name}: norm deviates by {nerr:.2e}"
            assert err <= 1e-4, f"{which} {name}: entries deviate by {err:.2e}"
    print(f"{which}: worst " + ", ".join(f"{n} {e:.1e}" for e, n in sorted(report, reverse=True)[:3]) + "; pos_embed: " +
          ", ".join(f"{n.split('mlp.')[1]} {e:.1e}" for e, n in report if n.startswith("pos_embed.")))
    assert n_pos == 10


# ---- 5. encode once, register pairs ------------------------------------------------------------------------
def test_register_equals_the_joint_forward_with_the_learned_embedding(device):
    from test_gpu_encode_once import _assert_rounding_level, _clouds
    pairs = [(0, 1), (2, 3), (0, 3)]
    clouds = _clouds(device)
    model = _model(device, 0)
    reg = model.register(model.encode(clouds), pairs)
    fwd = model({"src_xyz": [clouds[i] for i, _ in pairs], "tgt_xyz": [clouds[j] for _, j in pairs]})
    assert reg["pose"].shape == fwd["pose"].shape == (len(pairs), 3, 4)
    for b, pr in enumerate(pairs):
        _assert_rounding_level(reg, b, fwd, b, f"learned embedding, pair {pr}")
