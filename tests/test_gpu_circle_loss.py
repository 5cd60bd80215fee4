"""Circle feature loss on the MI355X (csrc/circle_loss.hip, ops.circle_loss, autograd.CircleLossFn,
RegTR.compute_loss with feature_loss_type: circle) against the float64 restatement of
test_circle_loss_host.py and against fixtures produced by the reference
(scripts/gen_circle_loss_golden.py)."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle.gen_golden import grad_sample_indices, loss_inputs, pairs_for
from superpoints_registration_amd import get_config, ops, synthetic
from superpoints_registration_amd.regtr import RegTR
from test_circle_loss_host import circle_reference, op_case

pytestmark = pytest.mark.gpu

H = 0.047        # keypoint lattice: squared distances are integer multiples of H^2, >= 5e-4 from both radii
R_P, R_N = 0.2, 0.4
POSE = torch.tensor([[0.0, -1.0, 0.0, 3 * H], [1.0, 0.0, 0.0, -2 * H], [0.0, 0.0, 1.0, H]])   # a lattice symmetry


def make_case(src_lens, tgt_lens, d, scale, seed, ln=False, far=(), extent=12):
    """Lists of src / tgt features and keypoints.  A third of every target cloud sits on transformed
    source points with near-copies of their features (fd < 0.1 positives); pairs in `far` have no
    positive at all."""
    rng = np.random.default_rng(seed)
    fs, ft, xs, xt = [], [], [], []
    R, t = POSE[:, :3].double().numpy(), POSE[:, 3].double().numpy()
    for b, (n, m) in enumerate(zip(src_lens, tgt_lens)):
        ps = rng.integers(0, extent, size=(n, 3)).astype(np.float64)
        pt = rng.integers(0, extent, size=(m, 3)).astype(np.float64) + (60.0 if b in far else 0.0)
        a, f = rng.standard_normal((n, d)), rng.standard_normal((m, d))
        if ln:
            a = (a - a.mean(1, keepdims=True)) / a.std(1, keepdims=True)
            f = (f - f.mean(1, keepdims=True)) / f.std(1, keepdims=True)
        else:
            a, f = a * 0.3, f * 0.3
        if b not in far:
            k = m // 3
            pick = rng.integers(0, n, size=k)
            pt[:k] = np.rint((ps[pick] * H @ R.T + t) / H)
            f[:k] = a[pick] + 0.02 * rng.standard_normal((k, d))
        fs.append(torch.from_numpy((a * scale).astype(np.float32)))
        ft.append(torch.from_numpy((f * scale).astype(np.float32)))
        xs.append(torch.from_numpy((ps * H).astype(np.float32)))
        xt.append(torch.from_numpy((pt * H).astype(np.float32)))
    return fs, ft, xs, xt


def run(device, fs, ft, xs, xt, grad=False, pose=POSE):
    B = len(fs)
    a = [f.to(device).requires_grad_(grad) for f in fs]
    b = [f.to(device).requires_grad_(grad) for f in ft]
    poses = pose.expand(B, 3, 4).contiguous().to(device)
    out = ops.circle_loss(a, b, [x.to(device) for x in xs], poses, [x.to(device) for x in xt], R_P, R_N)
    if not grad:
        return out, None, None
    ok = torch.isfinite(out.detach())
    out[ok].sum().div(B).backward()
    return out, [x.grad for x in a], [x.grad for x in b]


def reference(fs, ft, xs, xt, grad=False):
    a = [f.double().requires_grad_(grad) for f in fs]
    b = [f.double().requires_grad_(grad) for f in ft]
    pair = circle_reference(a, b, xs, POSE.double(), xt, R_P, R_N)
    if not grad:
        return pair.detach(), None, None
    ok = torch.isfinite(pair.detach())
    pair[ok].sum().div(len(fs)).backward()
    return pair.detach(), [x.grad for x in a], [x.grad for x in b]


def assert_pairs_close(got, ref, tol, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), (what, got, ref)
    ok = ~torch.isnan(ref)
    rel = ((got[ok] - ref[ok]).abs() / ref[ok].abs()).max() if ok.any() else torch.tensor(0.0)
    assert float(rel) <= tol, f"{what}: rel {float(rel):.2e}\n{got}\n{ref}"


def grad_rel(got, ref):
    got = torch.cat([g.detach().double().cpu().reshape(-1) for g in got])
    ref = torch.cat([g.detach().double().cpu().reshape(-1) for g in ref])
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


REGIMES = {
    # LayerNorm-scale features: fd ~ 22, active positive logits ~ 5 000; several tiles each way
    "layernorm": dict(src_lens=(150, 97), tgt_lens=(130, 200), d=256, scale=1.0, ln=True),
    # fd spans 0 .. 3: positives below 0.1, active negatives and zero-weight entries all occur
    "fd0to3": dict(src_lens=(140, 70), tgt_lens=(90, 129), d=32, scale=0.35),
    # ragged B = 3, N != M, a 1-row cloud (no column of that pair has both a pos and a neg: NaN)
    "ragged": dict(src_lens=(1, 65, 190), tgt_lens=(77, 64, 66), d=64, scale=0.35),
    "scale1e-3": dict(src_lens=(80,), tgt_lens=(70,), d=32, scale=1e-3),
    "scale1e-1": dict(src_lens=(80,), tgt_lens=(70,), d=32, scale=1e-1),
    "scale1e1": dict(src_lens=(80,), tgt_lens=(70,), d=32, scale=1e1),
    "scale1e3": dict(src_lens=(80,), tgt_lens=(70,), d=32, scale=1e3),
    "empty_row_sel": dict(src_lens=(40, 70), tgt_lens=(50, 30), d=32, scale=0.35, far=(0,)),
}


@pytest.mark.parametrize("regime", list(REGIMES))
def test_forward_matches_float64(device, regime):
    fs, ft, xs, xt = make_case(seed=sorted(REGIMES).index(regime) + 1, **REGIMES[regime])
    got, _, _ = run(device, fs, ft, xs, xt)
    ref, _, _ = reference(fs, ft, xs, xt)
    assert_pairs_close(got, ref, 1e-5, regime)
    if regime == "empty_row_sel":
        assert torch.isnan(got[0]) and torch.isfinite(got[1])
    else:
        assert torch.isfinite(ref[1 if regime == "ragged" else 0])


@pytest.mark.parametrize("regime", ["layernorm", "fd0to3", "ragged", "scale1e-1", "empty_row_sel"])
def test_input_gradients_match_float64(device, regime):
    fs, ft, xs, xt = make_case(seed=sorted(REGIMES).index(regime) + 1, **REGIMES[regime])
    _, ga, gb = run(device, fs, ft, xs, xt, grad=True)
    _, ra, rb = reference(fs, ft, xs, xt, grad=True)
    err = grad_rel(ga + gb, ra + rb)
    assert err <= 5e-5, f"{regime}: {err:.2e}"


def test_batched_equals_per_pair(device):
    fs, ft, xs, xt = make_case(seed=7, **REGIMES["ragged"])
    batched, ga, gb = run(device, fs, ft, xs, xt, grad=True)
    for b in range(len(fs)):
        one, oa, ob = run(device, fs[b:b + 1], ft[b:b + 1], xs[b:b + 1], xt[b:b + 1], grad=True)
        assert torch.equal(one.detach()[0], batched.detach()[b]) or (torch.isnan(one[0]) and torch.isnan(batched[b]))
        # gradients: the batched call scales each pair by 1 / B
        assert torch.equal(oa[0] / len(fs), ga[b]) or grad_rel([oa[0] / len(fs)], [ga[b]]) <= 1e-6, b
        assert torch.equal(ob[0] / len(fs), gb[b]) or grad_rel([ob[0] / len(fs)], [gb[b]]) <= 1e-6, b


def test_two_calls_are_bitwise_equal(device):
    fs, ft, xs, xt = make_case(seed=9, **REGIMES["layernorm"])
    o1, a1, b1 = run(device, fs, ft, xs, xt, grad=True)
    o2, a2, b2 = run(device, fs, ft, xs, xt, grad=True)
    assert torch.equal(o1, o2)
    for x, y in zip(a1 + b1, a2 + b2):
        assert torch.equal(x, y)


def test_refuses_cpu_tensors():
    fs, ft, xs, xt = make_case(seed=3, src_lens=(8,), tgt_lens=(9,), d=32, scale=1.0)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.circle_loss(fs, ft, xs, POSE[None], xt, R_P, R_N)


def test_matches_the_reference_op_fixture(device):
    g = load_golden("circle_ops.npz")
    pose = torch.from_numpy(g["pose"])
    for name in g["names"]:
        fs, ft, xs, xt = op_case(g, name)
        out, ga, gb = run(device, fs, ft, xs, xt, grad=True, pose=pose)
        assert_pairs_close(out, torch.from_numpy(g[f"{name}|pair"]), 1e-5, name)
        B = len(fs)
        ref = [torch.from_numpy(g[f"{name}|d_src{b}"]) for b in range(B)] + \
              [torch.from_numpy(g[f"{name}|d_tgt{b}"]) for b in range(B)]
        err = grad_rel(ga + gb, ref)
        assert err <= 5e-5, f"{name}: {err:.2e}"


def _circle_cfg():
    cfg = get_config("3dmatch")
    cfg.feature_loss_type = "circle"
    return cfg


def _batch(device):
    T = torch.from_numpy
    pairs, sizes = pairs_for("3dmatch", 2)
    pose, src_ov, tgt_ov = loss_inputs("3dmatch", 2)
    return {"src_xyz": [T(p[0][:n]).to(device) for p, (n, m) in zip(pairs, sizes)],
            "tgt_xyz": [T(p[1][:m]).to(device) for p, (n, m) in zip(pairs, sizes)],
            "pose": T(pose).to(device),
            "src_overlap": [T(o).to(device) for o in src_ov], "tgt_overlap": [T(o).to(device) for o in tgt_ov]}


@pytest.mark.parametrize("which", ["fo", "total"])
def test_training_step_gradients_match_the_reference(device, which):
    """Fixture (b): the reference's 3DMatch B = 2 step with feature_loss_type: circle.  Per-tensor criteria of
    test_gpu_backward.test_parameter_gradients_match_the_reference; alpha / beta (Sinkhorn scalars) get that
    test's 1e-3 norm window against the reference (its float64 anchor exists for InfoNCE only)."""
    g = load_golden("circle_grad_3dmatch_b2.npz")
    model = RegTR(_circle_cfg())
    synthetic.fill_parameters(model, seed=int(g["seed"]))
    model = model.to(device).train()
    batch = _batch(device)
    out = model(batch)
    losses = model.compute_loss(out, batch)
    for k in ("feature", "T", "overlap", "total"):
        ref = float(g[f"loss_{k}"])
        assert abs(float(losses[k].detach()) - ref) <= 5e-5 * max(1.0, abs(ref)), (k, float(losses[k]), ref)
    loss = losses["total"] if which == "total" else 0.1 * losses["feature"] + losses["overlap"]
    model.zero_grad(set_to_none=True)
    loss.backward()
    n_checked, n_enc, enc_loose, report = 0, 0, 0, []
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
        n_checked += 1
        if name in ("alpha", "beta"):
            assert nerr <= 1e-3, f"{which} {name}: deviates by {nerr:.2e}"
        elif name.startswith("kpf_encoder."):
            n_enc += 1
            enc_loose += err > 1e-4
            assert nerr <= 5e-4, f"{which} {name}: norm deviates by {nerr:.2e}"
            assert rms <= 2e-2, f"{which} {name}: RMS deviation {rms:.2e}"
        else:
            assert nerr <= 1e-4, f"{which} {name}: norm deviates by {nerr:.2e}"
            assert err <= 1e-4, f"{which} {name}: entries deviate by {err:.2e}"
        report.append((err, name))
    report.sort(reverse=True)
    print(f"circle/{which}: {n_checked} tensors; encoder above 1e-4 entrywise: {enc_loose}/{n_enc}; worst: " +
          ", ".join(f"{n} {e:.1e}" for e, n in report[:3]))
    assert n_checked >= 100


def test_trainer_step_with_the_circle_config(device):
    from superpoints_registration_amd.training import Trainer
    cfg = _circle_cfg()
    model = RegTR(cfg)
    synthetic.fill_parameters(model, seed=0)
    model = model.to(device)
    tr = Trainer(cfg).setup(model)
    losses = tr.train_step(model, dict(_batch(device)))
    for k in ("feature", "T", "overlap", "total"):
        assert math.isfinite(float(losses[k])), (k, losses[k])
    assert float(losses["feature"]) > 0
