"""GPU: KPConv in the six rigid modes (csrc/kpconv_modes.hip, superpoints_registration_amd/kpconv_modes.py) against
the float64 restatement of tests/kpconv_modes_cases.py and the reference's own results (tests/golden/kpconv_modes.npz).

Bounds: forward <= 1e-5 of the output's scale, gradients <= 2e-5 -- what tests/test_gpu_ops.py and
tests/test_gpu_backward.py hold KPConv to.  Every case asserts the input conditions of kpconv_modes_cases (arg-min
gap, row sums clear of 0) before it compares anything; no row is excluded."""
import numpy as np
import pytest
import torch

import kpconv_modes_cases as kc
from conftest import load_golden
from oracle import torch_oracle as O
from superpoints_registration_amd import _lib, get_config, kpconv_blocks, kpconv_modes, ops, overlap, stem, synthetic
from superpoints_registration_amd.regtr import RegTR
from test_gpu_backward import _rel
from test_gpu_workspace import _one_byte_short, run_three

pytestmark = pytest.mark.gpu
T = torch.from_numpy

# name -> make_case arguments.  Tile kernel: cin, cout multiples of 32, cout <= 256, 15 kernel points; both channel
# chunks (32: cin 32; 64: cin 64, 128 = two chunks), every n-tile count per wave (cout 32 / 64 / 128 / 256), tile tails
# (nq 1, 37, 130 = more than one workgroup), one staging pass and two (kmax 70, shuffled so that the second holds real
# neighbours).  Everything else: the one-thread-per-element kernel.
CASES = {
    "tile nq1 k1 32-32": dict(seed=21, nq=1, kmax=1, cin=32, cout=32),
    "tile nq37 k5 64-64": dict(seed=22, nq=37, kmax=5, cin=64, cout=64),
    "tile nq130 k33 128-128": dict(seed=23, nq=130, kmax=33, cin=128, cout=128),
    "tile nq130 k70 64-256 int64 unsorted": dict(seed=24, nq=130, kmax=70, cin=64, cout=256, radius=0.35, shuffle=True,
                                                 index_dtype=torch.int64),
    "tile strided nq37 ns130 k33 32-64": dict(seed=25, nq=37, ns=130, kmax=33, cin=32, cout=64, radius=0.3),
    "simple cin1 1-32": dict(seed=26, nq=37, kmax=5, cin=1, cout=32),
    "simple 48-40": dict(seed=27, nq=37, kmax=5, cin=48, cout=40),
    "simple 7 kernel points 32-32": dict(seed=28, nq=37, kmax=33, cin=32, cout=32, n_kp=7, radius=0.3),
}
BACKWARD_CASES = ("tile nq37 k5 64-64", "simple 48-40", "tile nq130 k70 64-256 int64 unsorted")
_cache = {}


def case_of(name):
    if name not in _cache:
        case = kc.make_case(**CASES[name])
        kc.check_conditions(case)
        _cache[name] = dict(case=case, ref={})
    return _cache[name]["case"]


def ref_of(name, mode):
    case = case_of(name)
    refs = _cache[name]["ref"]
    if mode not in refs:
        go = synthetic.rand((case["q"].shape[0], case["w"].shape[2]), 77)
        refs[mode] = (go,) + kc.ref64(case, mode[0], mode[1], go)
    return refs[mode]


def on_device(case, device, put=lambda t: t):
    return {k: (put(v.clone().to(device)) if isinstance(v, torch.Tensor) else v) for k, v in case.items()}


def run_forward(d, mode, impl=0):
    return kpconv_modes.kpconv(d["q"], d["s"], d["idx"], d["x"], d["w"], d["kp"], d["extent"], mode[0], mode[1], impl=impl)


def scale_err(got, ref):
    return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def test_cases_hold_what_they_are_meant_to():
    """Shadow entries, an all-shadow row and a row whose neighbours all have a negative feature sum in the cases with
    more than two queries; real neighbours behind column 64 in the wide case; the strided case's slice."""
    for name in CASES:
        case = case_of(name)
        idx, ns, x = case["idx"].long(), case["s"].shape[0], case["x"]
        if idx.shape[0] > 2:
            assert bool((idx[0] == ns).all()) and bool((idx == ns).any())
            last = idx[-1][idx[-1] < ns]
            assert last.numel() > 0 and bool((x[last].double().sum(1) < 0).all())
    wide = case_of("tile nq130 k70 64-256 int64 unsorted")["idx"]
    assert wide.dtype == torch.int64 and int((wide[:, 64:] < 130).sum()) > 20
    assert case_of("tile strided nq37 ns130 k33 32-64")["s"].shape[0] == 130


@pytest.mark.parametrize("mode", kc.MODES, ids=lambda m: "-".join(m))
@pytest.mark.parametrize("name", list(CASES))
def test_forward_matches_float64(device, name, mode):
    case = case_of(name)
    _, ref, _, _ = ref_of(name, mode)
    d = on_device(case, device)
    if "strided" in name:                         # a column slice of a wider matrix: nbr_stride > kmax
        wide = torch.full((d["idx"].shape[0], d["idx"].shape[1] + 3), -7, dtype=d["idx"].dtype, device=device)
        wide[:, :d["idx"].shape[1]] = d["idx"]
        d["idx"] = wide[:, :case["idx"].shape[1]]
    with torch.no_grad():
        out = run_forward(d, mode)
        again = run_forward(d, mode)
        simple = run_forward(d, mode, impl=1)
    err = scale_err(out, ref)
    print(f"{name} {mode}: {err:.2e} of the output's scale (simple kernel {scale_err(simple, ref):.2e})")
    assert err <= 1e-5
    assert scale_err(simple, ref) <= 1e-5
    assert torch.equal(out, again), "two runs differ"
    if case["idx"].shape[0] > 2:                  # row 0 is all shadow
        assert float(out[0].abs().max()) == 0.0


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("tile")])
def test_linear_sum_agrees_with_the_shipped_kernels(device, name):
    """The cross-check of the new tile kernel against spr_kpconv_fwd (ring / tile kernels), same 1e-5."""
    d = on_device(case_of(name), device)
    with torch.no_grad():
        new = run_forward(d, ('linear', 'sum'))
        shipped = ops.kpconv(d["q"], d["s"], d["idx"], d["x"], d["w"], d["kp"], d["extent"])
    err = float((new - shipped).abs().max() / shipped.abs().max()) if float(shipped.abs().max()) > 0 else \
        float((new - shipped).abs().max())
    print(f"{name}: new vs shipped {err:.2e}")
    assert err <= 1e-5


def _golden(device):
    g = load_golden("kpconv_modes.npz")
    case = dict(kc.golden_case(), kp=T(g["kp"]))
    kc.check_conditions(case)
    return g, on_device(case, device)


@pytest.mark.parametrize("mode", kc.NEW_MODES, ids=lambda m: "-".join(m))
def test_forward_and_backward_match_the_reference(device, mode):
    g, d = _golden(device)
    x, w = d["x"].requires_grad_(True), d["w"].requires_grad_(True)
    out = kpconv_modes.kpconv(d["q"], d["s"], d["idx"], x, w, d["kp"], d["extent"], mode[0], mode[1])
    out.backward(kc.golden_go().to(device))
    tag = f"{mode[0]}|{mode[1]}|"
    errs = (scale_err(out, T(g[tag + "out"]).double()), scale_err(x.grad, T(g[tag + "dx"]).double()))
    dw = w.grad.reshape(-1).double().cpu()
    e_dw = float((dw[::kc.GOLDEN_DW_STEP] - T(g[tag + "dw|samples"]).double()).abs().max() / dw.abs().max())
    print(f"{mode}: out {errs[0]:.2e}, dx {errs[1]:.2e}, dW {e_dw:.2e}")
    assert errs[0] <= 1e-5 and errs[1] <= 2e-5 and e_dw <= 2e-5
    assert abs(float(dw.norm()) - float(g[tag + "dw|norm"])) <= 2e-5 * float(g[tag + "dw|norm"])


@pytest.fixture(params=[(4, 1), (1, 1), (0, 0)], ids=["default", "split-fp16", "exact-f32"])
def arithmetic(request):
    """The three settings tests/test_gpu_backward.py runs its operators in, as (attention mode, GEMM mode).  The KPConv
    backward follows the GEMM switch (split-fp16 products or exact-f32 spr_bgemm); the attention switch is set with it
    so that each setting is the library state its name stands for."""
    attn, gemm = request.param
    ops.set_attn_mode(attn)
    ops.set_gemm_mode(gemm)
    yield request.param
    ops.set_attn_mode(ops.DEFAULT_ATTN_MODE)
    ops.set_gemm_mode(1)


@pytest.mark.parametrize("mode", kc.MODES, ids=lambda m: "-".join(m))
@pytest.mark.parametrize("name", BACKWARD_CASES)
def test_backward_matches_float64_autograd(device, arithmetic, name, mode):
    case = case_of(name)
    go, _, dx_ref, dw_ref = ref_of(name, mode)

    def grads():
        d = on_device(case, device)
        x, w = d["x"].requires_grad_(True), d["w"].requires_grad_(True)
        run_forward(dict(d, x=x, w=w), mode).backward(go.to(device))
        return x.grad, w.grad
    dx, dw = grads()
    dx2, dw2 = grads()
    print(f"{name} {mode}: dx {_rel(dx, dx_ref):.2e}, dW {_rel(dw, dw_ref):.2e}")
    assert _rel(dx, dx_ref) <= 2e-5
    assert _rel(dw, dw_ref) <= 2e-5
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2), "two runs differ"


# ---- bounds --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [('gaussian', 'sum'), ('linear', 'closest'), ('constant', 'sum')], ids=lambda m: "-".join(m))
@pytest.mark.parametrize("name", ["tile nq130 k70 64-256 int64 unsorted", "tile strided nq37 ns130 k33 32-64", "simple 48-40",
                                  "simple cin1 1-32"])
def test_forward_and_backward_inside_guarded_tensors(device, monkeypatch, name, mode):
    """spr_kpconv_modes_fwd, _weighted_features and _bwd_dx with exactly the workspace they ask for, poisoned, and
    every input, output and host-side scratch tensor between guard bands (tests/test_gpu_workspace.py::run_three).
    Fresh weight tensors per run: the planes are built inside the arena."""
    case = case_of(name)
    go, ref, dx_ref, dw_ref = ref_of(name, mode)

    def f(put):
        d = on_device(case, device, put)
        x, w = d["x"].requires_grad_(True), d["w"].requires_grad_(True)
        out = run_forward(dict(d, x=x, w=w), mode)
        out.backward(put(go.clone().to(device)))
        with torch.no_grad():
            plain = run_forward(on_device(case, device, put), mode)
        return out.detach(), plain, x.grad, w.grad
    out, plain, dx, dw = run_three(monkeypatch, f, f"kpconv_modes {name} {mode}", placed=True)
    assert torch.equal(out, plain)
    assert scale_err(out, ref) <= 1e-5 and _rel(dx, dx_ref) <= 2e-5 and _rel(dw, dw_ref) <= 2e-5


def test_one_byte_short_is_refused(device, monkeypatch):
    """Each of the three entry points that carve a workspace, handed its size query minus one byte: the operator's own
    status (RuntimeError naming the workspace), nothing written, guards intact (test_gpu_workspace.py::_one_byte_short)."""
    infl, agg = kpconv_modes.mode_codes('gaussian', 'closest')
    for name in ("tile nq37 k5 64-64", "simple 48-40"):
        d = on_device(case_of(name), device)
        cin = d["x"].shape[1]
        dwf = synthetic.rand((d["q"].shape[0], d["kp"].shape[0] * cin), 5).to(device)
        _one_byte_short(monkeypatch, f"kpconv_modes forward {name}",
                        lambda: None, lambda _: kpconv_modes.kpconv_raw(d["q"], d["s"], d["idx"], d["x"], d["w"].clone(),
                                                                        d["kp"], d["extent"], infl, agg))
        _one_byte_short(monkeypatch, f"kpconv_modes weighted features {name}",
                        lambda: None, lambda _: kpconv_modes.weighted_features(d["q"], d["s"], d["idx"], d["x"], d["kp"],
                                                                               d["extent"], infl, agg))
        _one_byte_short(monkeypatch, f"kpconv_modes bwd_dx {name}",
                        lambda: None, lambda _: kpconv_modes.bwd_dx(d["q"], d["s"], d["idx"], cin, d["kp"], d["extent"],
                                                                    infl, agg, dwf))


def test_unknown_mode_is_refused_with_the_operators_status(device):
    d = on_device(case_of("tile nq37 k5 64-64"), device)
    with pytest.raises(RuntimeError, match="influence"):
        kpconv_modes.kpconv_raw(d["q"], d["s"], d["idx"], d["x"], d["w"], d["kp"], d["extent"], 3, 0)
    with pytest.raises(RuntimeError, match="aggregation"):
        kpconv_modes.weighted_features(d["q"], d["s"], d["idx"], d["x"], d["kp"], d["extent"], 0, 2)


# ---- encoder end to end ----------------------------------------------------------------------------------------------------
def _pair(device, seed):
    src, tgt, pose = synthetic.make_pair(2048, seed=seed, extent=0.6, jitter=0.002)
    return T(src).to(device), T(tgt).to(device), T(pose).to(device)


@pytest.mark.parametrize("mode", [('gaussian', 'sum'), ('linear', 'closest')], ids=lambda m: "-".join(m))
def test_encoder_features_match_the_oracle(device, monkeypatch, mode):
    """KPFEncoder inference in a non-default mode against oracle.torch_oracle.encoder (float64) with its kpconv replaced
    by the restatement, on OUR pyramid; the bound of tests/test_gpu_regtr.py::test_encoder_features_match_reference.
    The first block does not take the stem route (the stem kernel is linear / sum), the others run through
    kpconv_modes, never ops.kpconv."""
    cfg = get_config('3dmatch', KP_influence=mode[0], aggregation_mode=mode[1])
    model = RegTR(cfg)
    synthetic.fill_parameters(model, seed=4)
    sd = {k: (v.detach().clone().double() if v.is_floating_point() else v.clone()) for k, v in model.state_dict().items()}
    model = model.to(device).eval()
    src, tgt, _ = _pair(device, 3)
    calls = {"modes": 0}
    real = kpconv_modes.kpconv

    def counted(*a, **k):
        calls["modes"] += 1
        return real(*a, **k)
    monkeypatch.setattr(kpconv_modes, "kpconv", counted)
    monkeypatch.setattr(ops, "kpconv", lambda *a, **k: pytest.fail("ops.kpconv in a non-default mode"))
    monkeypatch.setattr(stem, "kpconv_stem", lambda *a, **k: pytest.fail("the stem route in a non-default mode"))
    with torch.no_grad():
        meta = model.preprocessor([src, tgt])
        feats0 = torch.ones((meta['points'][0].shape[0], 1), dtype=torch.float32, device=device)
        first = model.kpf_encoder.encoder_blocks[0]
        assert isinstance(first, kpconv_blocks.SimpleBlock)
        assert stem.stem_route(feats0, first.KPConv.weights, first.use_bn), "the default mode would take the stem here"
        assert not first.stem_route(feats0)
        feats, _ = model.kpf_encoder(feats0, meta)
    n_conv = sum(isinstance(m, kpconv_blocks.KPConv) for m in model.kpf_encoder.modules())
    assert calls["modes"] == n_conv > 0
    cpu = {k: [t.cpu() for t in meta[k]] for k in ('points', 'neighbors', 'pools', 'stack_lengths')}
    cpu['points'] = [p.double() for p in cpu['points']]
    monkeypatch.setattr(O, "kpconv", lambda q, s, idx, x, w, kp, ext: kc.kpconv_ref(q, s, idx, x, w, kp, ext, *mode))
    ref, _ = O.encoder(cfg, sd, cpu)
    err = float((feats.double().cpu() - ref).abs().max() / ref.abs().max())
    print(f"encoder {mode}: {err:.2e} of max |features|")
    assert feats.shape == ref.shape and err <= 2e-5


def test_one_training_step_in_gaussian_closest(device):
    from superpoints_registration_amd.training import Trainer
    cfg = get_config('3dmatch', KP_influence='gaussian', aggregation_mode='closest')
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
    assert any("KPConv.weights" in n for n in moved) and len(moved) > len(before) // 2


# ---- regression guard --------------------------------------------------------------------------------------------------------
def test_the_default_config_never_enters_kpconv_modes(device, monkeypatch):
    """With the shipped configs KPConv.forward runs ops.kpconv (and the stem), as before: inference and a training
    forward / backward, with every function of kpconv_modes that launches something replaced by a sentinel."""
    def sentinel(*a, **k):
        raise AssertionError("kpconv_modes entered in the default mode")
    for fn in ("kpconv", "kpconv_raw", "weighted_features", "bwd_dx"):
        monkeypatch.setattr(kpconv_modes, fn, sentinel)
    monkeypatch.setattr(kpconv_modes.KPConvModesFn, "forward", staticmethod(sentinel))
    cfg = get_config('3dmatch')
    model = RegTR(cfg)
    synthetic.fill_parameters(model, seed=0)
    model = model.to(device).eval()
    src, tgt, pose = _pair(device, 3)
    with torch.no_grad():
        out = model({"src_xyz": [src], "tgt_xyz": [tgt]})
    assert bool(torch.isfinite(out["pose"]).all())
    model.train()
    batch = {"src_xyz": [src], "tgt_xyz": [tgt], "pose": pose.unsqueeze(0)}
    overlap.label_batch(batch, cfg.overlap_radius)
    losses = model.compute_loss(model(batch), batch)
    losses["total"].backward()
    assert np.isfinite(float(losses["total"].detach()))
