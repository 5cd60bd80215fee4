"""GPU: deformable / modulated KPConv (csrc/kpconv_deform.hip, superpoints_registration_amd/deformable) against the
float64 restatement of tests/deform_cases.py and the reference's own results (tests/golden/kpconv_deform.npz).

Bounds: forward <= 1e-5 of the output's scale, dx / dW / d offset_features <= 2e-5 -- what tests/test_gpu_ops.py and
tests/test_gpu_backward.py hold KPConv to.  The two gradients that pass through a second backward stage (the offset
convolution's dW and d offset_bias) are held to 2e-5 in exact f32; in the two split-fp16 settings their bound is twice
the largest value MEASURED on the backward cases below (SECOND_STAGE_BOUND; never above 1e-4).  Measured, relative to
the gradient's largest entry, against the float64 restatement:
    offset conv dW   5.38e-07 (nq130 k70 64-256 int64 unsorted, plain); the other five runs 2.07e-07 .. 4.92e-07
    d offset_bias    3.99e-07 (same case); the others 1.97e-07 .. 2.89e-07
(identical in the default and the split-fp16 setting), so SECOND_STAGE_BOUND = 2 x 5.38e-07.  Exact f32 gives up to
7.67e-07 / 3.80e-07 on the same cases, under its own 2e-5.
Every case asserts the input conditions of deform_cases (range gap, distance floor, row sums, in-range share) before it
compares anything; no row is excluded."""
import numpy as np
import pytest
import torch

import deform_cases as dc
import kpconv_modes_cases as kc
from conftest import load_golden
from superpoints_registration_amd import deformable, get_config, ops, overlap, synthetic
from superpoints_registration_amd.kpconv import KPFEncoder, Preprocessor, plan_pyramid
from superpoints_registration_amd.regtr import RegTR
from test_gpu_backward import _rel
from test_gpu_kpconv_modes import arithmetic  # noqa: F401  (the fixture: default / split-fp16 / exact-f32)

pytestmark = pytest.mark.gpu
T = torch.from_numpy
MOD = [False, True]
mod_id = lambda m: "modulated" if m else "plain"
SECOND_STAGE_BOUND = 2 * 5.38e-07
_cache = {}


def case_of(name, modulated):
    """(case, float64 out, aux, go, grads), computed once and left unchanged."""
    key = (name, bool(modulated))
    if key not in _cache:
        case = dc.make_case(name, modulated)
        go = synthetic.rand((case["q"].shape[0], case["w"].shape[2]), 77)
        out, aux, grads = dc.ref64(case, go)
        dc.check_conditions(case, aux)
        _cache[key] = (case, out, aux, go, grads)
    return _cache[key]


def on_device(case, device, put=lambda t: t):
    return {k: (put(v.clone().to(device)) if isinstance(v, torch.Tensor) else v) for k, v in case.items()}


def scale_err(got, ref):
    return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def run_kernel(d, of, impl=0, want_min_d2=False):
    return deformable.kpconv_deform(d["q"], d["s"], d["idx"], d["x"], d["w"], d["kp"], d["extent"], of, d["modulated"],
                                    impl=impl, want_min_d2=want_min_d2)


def run_chain(d, impl=0):
    """The module's forward from its parts: rigid offset convolution (own kernel points) + bias -> kpconv_deform."""
    of = ops.kpconv(d["q"], d["s"], d["idx"], d["x"], d["off_w"], d["off_kp"], d["extent"]) + d["off_b"]
    return run_kernel(d, of, impl), of


def test_cases_hold_what_they_are_meant_to():
    for name in dc.CASES:
        for modulated in MOD:
            case, _, aux, _, _ = case_of(name, modulated)
            idx, ns = case["idx"].long(), case["s"].shape[0]
            if idx.shape[0] > 2:
                assert bool((idx[0] == ns).all()) and bool((idx == ns).any())
                assert bool((aux["valid"] & ~aux["in_range"]).any()) and bool(aux["in_range"].any())
    wide, _, aux, _, _ = case_of("nq130 k70 64-256 int64 unsorted", True)
    assert wide["idx"].dtype == torch.int64 and int(aux["in_range"][:, 64:].sum()) > 20
    assert case_of("strided nq37 ns130 k33 32-64", False)[0]["s"].shape[0] == 130


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
@pytest.mark.parametrize("name", list(dc.CASES))
def test_forward_matches_float64(device, name, modulated):
    case, ref, aux, _, _ = case_of(name, modulated)
    d = on_device(case, device)
    of = aux["offset_features"].float().to(device)           # the kernel under test alone: the float64 offsets, rounded
    if "strided" in name:                                    # a column slice of a wider matrix: nbr_stride > kmax
        wide = torch.full((d["idx"].shape[0], d["idx"].shape[1] + 3), -7, dtype=d["idx"].dtype, device=device)
        wide[:, :d["idx"].shape[1]] = d["idx"]
        d["idx"] = wide[:, :case["idx"].shape[1]]
    with torch.no_grad():
        out, min_d2 = run_kernel(d, of, want_min_d2=True)
        again = run_kernel(d, of)
        simple, min_d2_simple = run_kernel(d, of, impl=1, want_min_d2=True)
        _, cnt = deformable.weighted_features(d["q"], d["s"], d["idx"], d["x"], d["kp"], d["extent"], of)
    err, err_s = scale_err(out, ref), scale_err(simple, ref)
    e_min = float(((min_d2.double().cpu() - aux["min_d2"]).abs() / aux["min_d2"]).max())
    print(f"{name} {mod_id(modulated)}: {err:.2e} of the output's scale (simple kernel {err_s:.2e}), min_d2 {e_min:.2e}")
    assert err <= 1e-5 and err_s <= 1e-5
    assert torch.equal(out, again), "two runs differ"
    assert e_min <= 1e-5 and torch.equal(min_d2, min_d2_simple)
    assert torch.equal(cnt.cpu().long(), aux["count"]), "the in-range counts differ from the float64 counts"
    if case["idx"].shape[0] > 2:                             # row 0 is all shadow
        assert float(out[0].abs().max()) == 0.0 and float(simple[0].abs().max()) == 0.0
        far = (dc.FAR - case["q"][0].double()).unsqueeze(0) - aux["deformed_KP"][0]
        assert float(((min_d2[0].double().cpu() - (far ** 2).sum(1)).abs() / (far ** 2).sum(1)).max()) <= 1e-5


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
@pytest.mark.parametrize("name", list(dc.CASES))
def test_the_chain_matches_float64(device, name, modulated):
    """Offset convolution (float32, on the device) + bias -> kpconv_deform, as the module runs it; deformed_KP of the
    module's formula."""
    case, ref, aux, _, _ = case_of(name, modulated)
    d = on_device(case, device)
    with torch.no_grad():
        out, of = run_chain(d)
        simple, _ = run_chain(d, impl=1)
    K = d["kp"].shape[0]
    D = of[:, :3 * K].view(-1, K, 3) * d["extent"] + d["kp"]
    e_d = float((D.double().cpu() - aux["deformed_KP"]).abs().max() / aux["deformed_KP"].abs().max())
    print(f"{name} {mod_id(modulated)}: chain {scale_err(out, ref):.2e} (simple {scale_err(simple, ref):.2e}), "
          f"offsets {scale_err(of, aux['offset_features']):.2e}, deformed_KP {e_d:.2e}")
    assert scale_err(out, ref) <= 1e-5 and scale_err(simple, ref) <= 1e-5 and e_d <= 1e-5


@pytest.mark.parametrize("name", list(dc.CASES))
def test_zero_offsets_collapse_to_the_rigid_kernels(device, name):
    """Zero offset weights and bias, no modulation: D = kp.  On the rows whose valid neighbours are ALL in range (the
    float64 in_range of the restatement) the count is the rigid one and the result agrees with ops.kpconv to 1e-5 of its
    scale; on the other rows (a neighbour beyond every kernel point's extent is cut from the count) it equals the
    restatement."""
    case = dict(dc.make_case(name, False))
    case["off_w"], case["off_b"] = torch.zeros_like(case["off_w"]), torch.zeros_like(case["off_b"])
    ref, aux = dc.ref64(case)
    c = dc.conditions(case, aux)
    assert c["gap"] >= dc.GAP_MIN and c["row_sum"] >= dc.SUM_MIN
    d = on_device(case, device)
    with torch.no_grad():
        out, of = run_chain(d)
        rigid = ops.kpconv(d["q"], d["s"], d["idx"], d["x"], d["w"], d["kp"], d["extent"])
    assert float(of.abs().max()) == 0.0
    rows = (aux["in_range"] == aux["valid"]).all(1)          # every valid neighbour in range (all-shadow rows too)
    scale = float(rigid.abs().max())
    e_rigid = float((out[rows.to(device)] - rigid[rows.to(device)]).abs().max()) / max(scale, 1e-30)
    print(f"{name}: {int(rows.sum())} of {rows.numel()} rows fully in range; vs ops.kpconv {e_rigid:.2e}, "
          f"vs float64 {scale_err(out, ref):.2e}")
    if case["q"].shape[0] > 2:
        assert 0 < int(rows.sum()) < rows.numel()
    assert e_rigid <= 1e-5
    assert scale_err(out, ref) <= 1e-5


def _chain_grads(case, go, device, put=lambda t: t):
    d = on_device(case, device, put)
    leaves = {k: d[k].requires_grad_(True) for k in ("x", "w", "off_w", "off_b")}
    of = ops.kpconv(d["q"], d["s"], d["idx"], leaves["x"], leaves["off_w"], d["off_kp"], d["extent"]) + leaves["off_b"]
    of.retain_grad()
    out = run_kernel(dict(d, **leaves), of)
    out.backward(put(go.clone().to(device)))
    return out.detach(), dict(dx=leaves["x"].grad, dw=leaves["w"].grad, d_off_w=leaves["off_w"].grad,
                              d_off_b=leaves["off_b"].grad, d_of=of.grad)


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
@pytest.mark.parametrize("name", dc.BACKWARD_CASES)
def test_backward_matches_float64_autograd(device, arithmetic, name, modulated):
    case, _, _, go, ref = case_of(name, modulated)
    _, g = _chain_grads(case, go, device)
    _, g2 = _chain_grads(case, go, device)
    errs = {k: _rel(g[k], ref[k]) for k in ref}
    print(f"{name} {mod_id(modulated)} {arithmetic}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k in ("dx", "dw", "d_of"):
        assert errs[k] <= 2e-5, (k, errs[k])
    second = 2e-5 if arithmetic == (0, 0) else SECOND_STAGE_BOUND
    assert second <= 1e-4
    for k in ("d_off_w", "d_off_b"):
        assert errs[k] <= second, (k, errs[k])
    for k in g:
        assert torch.equal(g[k], g2[k]), f"two runs differ in {k}"


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
@pytest.mark.parametrize("name", ["nq37 k5 64-64", "simple 48-40"])
def test_the_module_runs_the_chain(device, name, modulated):
    """KPConvDeformable with a case's parameters, forward and backward in the default arithmetic: the chain's bounds, and
    the attributes the reference's module holds after a forward.  64 input channels: the offset convolution runs on
    zero-padded weights; 48: at its own width."""
    case, ref, aux, go, gref = case_of(name, modulated)
    d = on_device(case, device)
    K, cin, cout = case["w"].shape
    m = deformable.KPConvDeformable(K, 3, cin, cout, case["extent"], 0.1, modulated=modulated).to(device)
    with torch.no_grad():
        for p, v in ((m.weights, d["w"]), (m.kernel_points, d["kp"]), (m.offset_conv.weights, d["off_w"]),
                     (m.offset_conv.kernel_points, d["off_kp"]), (m.offset_bias, d["off_b"])):
            p.copy_(v)
        plain = m(d["q"], d["s"], d["idx"], d["x"])
        cached = m(d["q"], d["s"], d["idx"], d["x"])           # the cached padded copy
    assert torch.equal(plain, cached) and not m.offset_features.requires_grad
    x = d["x"].clone().requires_grad_(True)
    out = m(d["q"], d["s"], d["idx"], x)
    out.backward(go.to(device))
    errs = dict(out=scale_err(out, ref), plain=scale_err(plain, ref), dx=_rel(x.grad, gref["dx"]),
                dw=_rel(m.weights.grad, gref["dw"]), d_off_w=_rel(m.offset_conv.weights.grad, gref["d_off_w"]),
                d_off_b=_rel(m.offset_bias.grad, gref["d_off_b"]))
    print(f"module {name} {mod_id(modulated)}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["out"] <= 1e-5 and errs["plain"] <= 1e-5 and errs["dx"] <= 2e-5 and errs["dw"] <= 2e-5
    assert errs["d_off_w"] <= SECOND_STAGE_BOUND and errs["d_off_b"] <= SECOND_STAGE_BOUND
    assert m.kernel_points.grad is None and m.offset_conv.kernel_points.grad is None
    assert scale_err(m.offset_features, aux["offset_features"]) <= 1e-5
    assert scale_err(m.deformed_KP, aux["deformed_KP"]) <= 1e-5
    assert float(((m.min_d2.double().cpu() - aux["min_d2"]).abs() / aux["min_d2"]).max()) <= 1e-5
    assert not m.min_d2.requires_grad


# ---- the reference's own results -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
def test_forward_and_backward_match_the_reference(device, modulated):
    """tests/golden/kpconv_deform.npz: the reference's KPConv(deformable=True) in float32 on the CPU, with its own draws of
    both convolutions' kernel points."""
    g = load_golden("kpconv_deform.npz")
    case = dc.golden_case(modulated, kp=T(g["kp"]), off_kp=T(g["off_kp"]))
    dc.check_conditions(case)
    out, grads = _chain_grads(case, kc.golden_go(), device)
    tag = "mod|" if modulated else "plain|"
    errs = dict(out=scale_err(out, T(g[tag + "out"]).double()), dx=scale_err(grads["dx"], T(g[tag + "dx"]).double()),
                d_off_b=scale_err(grads["d_off_b"], T(g[tag + "d_off_b"]).double()))
    for name in ("dw", "d_off_w"):
        flat = grads[name].reshape(-1).double().cpu()
        errs[name] = float((flat[::dc.GOLDEN_DW_STEP] - T(g[tag + name + "|samples"]).double()).abs().max() / flat.abs().max())
        norm = float(g[tag + name + "|norm"])
        assert abs(float(flat.norm()) - norm) <= 2e-5 * norm, name
    print(f"{mod_id(modulated)}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["out"] <= 1e-5
    for k in ("dx", "dw", "d_off_w", "d_off_b"):
        assert errs[k] <= 2e-5, (k, errs[k])


# ---- encoder end to end --------------------------------------------------------------------------------------------------
def _encoder_config(name):
    arch, modulated = dc.ENCODER_ARCHS[name]
    return get_config('3dmatch', deformable_kpconv=True, architecture=list(arch), modulated=modulated)


def _fixture_pyramid(g, name, device):
    pyr = str(g[f"{name}|pyramid"])
    n_levels = sum(1 for k in g if k.startswith(f"{pyr}|points"))
    meta = {k: [] for k in ("points", "neighbors", "pools", "stack_lengths")}
    for l in range(n_levels):
        meta["points"].append(T(g[f"{pyr}|points{l}"]).to(device))
        meta["stack_lengths"].append(T(g[f"{pyr}|lens{l}"]).to(device))
        for kind in ("neighbors", "pools"):
            meta[kind].append(T(g[f"{pyr}|{kind}{l}"].astype(np.int64)).to(device))
    return meta


@pytest.mark.parametrize("name", list(dc.ENCODER_ARCHS))
def test_encoder_features_match_the_reference(device, name):
    """KPFEncoder with deformable blocks on the reference Preprocessor's pyramid (tests/golden/deform_encoder.npz) against
    the reference KPFEncoder's features; the bound of tests/test_gpu_regtr.py::test_encoder_features_match_reference."""
    g = load_golden("deform_encoder.npz")
    cfg = _encoder_config(name)
    enc = KPFEncoder(cfg, cfg.d_embed)
    synthetic.fill_parameters(enc, seed=int(g["seed"]))
    n_deform = sum(isinstance(m, deformable.KPConvDeformable) for m in enc.modules())
    assert n_deform == sum('deformable' in b for b in cfg.architecture) > 0
    enc = enc.to(device).eval()
    meta = _fixture_pyramid(g, name, device)
    with torch.no_grad():
        feats, _ = enc(torch.ones((meta["points"][0].shape[0], 1), dtype=torch.float32, device=device), meta)
    ref = T(g[f"{name}|feats"]).double()
    err = float((feats.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"encoder {name}: {err:.2e} of max |features|")
    assert feats.shape == ref.shape and err <= 2e-5
    for m in enc.modules():
        if isinstance(m, deformable.KPConvDeformable):
            nq = m.offset_features.shape[0]
            assert m.offset_features.shape == (nq, m.offset_dim) and m.deformed_KP.shape == (nq, m.K, 3)
            assert m.min_d2.shape == (nq, m.K) and bool(torch.isfinite(m.min_d2).all())


@pytest.mark.parametrize("name", ["last", "quirk"])
def test_preprocessor_rows_hold_the_reference_counts(device, name):
    """Our Preprocessor on the fixture's two clouds: the reference's points at every level and its per-row neighbour
    counts in every conv and pool matrix (counts do not depend on the order inside a row).  'quirk': the level whose only
    deformable conv block is its last keeps the normal conv radius, the deformable strided block widens its pools."""
    g = load_golden("deform_encoder.npz")
    cfg = _encoder_config(name)
    meta = Preprocessor(cfg)([T(g["src"]).to(device), T(g["tgt"]).to(device)])
    ref = _fixture_pyramid(g, name, "cpu")
    assert len(meta["points"]) == len(ref["points"])
    for l, pts in enumerate(ref["points"]):
        assert torch.equal(meta["stack_lengths"][l].cpu().long(), ref["stack_lengths"][l].long())
        assert float((meta["points"][l].cpu() - pts).abs().max()) <= 1e-6
        for kind, n_sup in (("neighbors", pts.shape[0]), ("pools", pts.shape[0])):
            want = ref[kind][l]
            if want.shape[0] == 0:
                assert meta[kind][l].shape[0] == 0
                continue
            got = meta[kind][l].cpu()
            assert torch.equal((got < n_sup).sum(1), (want < n_sup).sum(1)), (name, kind, l)
    _, levels, _ = plan_pyramid(cfg)
    if name == "quirk":
        assert levels[2].conv_radius == levels[2].radius and levels[1].pool_radius == 2 * levels[1].radius
    else:
        assert levels[2].conv_radius == 2 * levels[2].radius


# ---- training ------------------------------------------------------------------------------------------------------------
def _pair(device, seed, n=2048, **kw):
    src, tgt, pose = synthetic.make_pair(n, seed=seed, **dict(dict(extent=0.6, jitter=0.002), **kw))
    return T(src).to(device), T(tgt).to(device), T(pose).to(device)


def test_one_training_step_with_modulated_deformable_blocks(device):
    from superpoints_registration_amd.training import Trainer
    cfg = _encoder_config("last modulated")
    model = RegTR(cfg)
    synthetic.fill_parameters(model, seed=0)
    model = model.to(device)
    src, tgt, pose = _pair(device, 5)
    batch = {"src_xyz": [src], "tgt_xyz": [tgt], "pose": pose.unsqueeze(0)}
    overlap.label_batch(batch, cfg.overlap_radius)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    losses = Trainer(cfg).setup(model).train_step(model, batch)
    for k in ("feature", "T", "overlap", "total"):
        assert np.isfinite(float(losses[k])), (k, float(losses[k]))
    moved = [n for n, p in model.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert any(n.endswith("KPConv.offset_conv.weights") for n in moved) and any(n.endswith("KPConv.offset_bias") for n in moved)
    assert any(n.endswith("KPConv.weights") for n in moved) and len(moved) > len(before) // 2


# ---- regression guard ----------------------------------------------------------------------------------------------------
GUARD_PAIRS = {"3dmatch": lambda d: _pair(d, 3), "kitti": lambda d: _pair(d, 3, n=6000, extent=20.0, jitter=0.02),
               "modelnet": lambda d: tuple(T(a).to(d) for a in synthetic.make_sphere_pair(1024, seed=3))}


@pytest.mark.parametrize("tag", list(GUARD_PAIRS))
def test_the_shipped_configs_never_enter_deformable(device, monkeypatch, tag):
    """Inference and a training forward / backward with every function of the subpackage that launches or builds
    something replaced by a sentinel."""
    def sentinel(*a, **k):
        raise AssertionError("the deformable subpackage entered by a shipped config")
    for fn in ("kpconv_deform", "kpconv_deform_raw", "weighted_features", "bwd_dx", "bwd_offsets"):
        monkeypatch.setattr(deformable, fn, sentinel)
    monkeypatch.setattr(deformable.KPConvDeformFn, "forward", staticmethod(sentinel))
    monkeypatch.setattr(deformable.KPConvDeformable, "__init__", sentinel)
    monkeypatch.setattr(deformable.KPConvDeformable, "forward", sentinel)
    cfg = get_config(tag)
    assert not cfg.deformable_kpconv
    model = RegTR(cfg)
    synthetic.fill_parameters(model, seed=0)
    model = model.to(device).eval()
    src, tgt, pose = GUARD_PAIRS[tag](device)
    with torch.no_grad():
        out = model({"src_xyz": [src], "tgt_xyz": [tgt]})
    assert bool(torch.isfinite(out["pose"]).all())
    model.train()
    batch = {"src_xyz": [src], "tgt_xyz": [tgt], "pose": pose.unsqueeze(0)}
    overlap.label_batch(batch, cfg.overlap_radius)
    losses = model.compute_loss(model(batch), batch)
    losses["total"].backward()
    assert np.isfinite(float(losses["total"].detach()))
