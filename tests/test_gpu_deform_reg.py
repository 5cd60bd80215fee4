"""GPU: the regulariser of deformable KPConv (csrc/deform_reg.hip, superpoints_registration_amd/deform_reg) against the
float64 restatement of tests/deform_reg_cases.py -- the operator on all eight cases of tests/deform_cases.py, modulated
off and on; through KPConvDeformable; and end to end through RegTR.compute_loss and its backward.

Bounds: fit and rep each within 1e-5 relative of float64 and d offset_features within 1e-5 of the float64 gradient's
largest magnitude -- the figure tests/test_gpu_deform.py holds min_d2 and deformed_KP to; the offset parameters'
gradients through the module within 2e-5 in exact f32 and within SECOND_STAGE_BOUND in the default arithmetic.
Every comparison of a gradient asserts the argmin-gap condition of deform_reg_cases first; no row is excluded."""
import numpy as np
import pytest
import torch

import deform_cases as dc
import deform_reg_cases as rc
from superpoints_registration_amd import _lib, deform_reg, deformable, get_config, ops, overlap, synthetic
from superpoints_registration_amd.regtr import RegTR
from test_gpu_backward import _rel
from test_gpu_deform import on_device, run_kernel

pytestmark = pytest.mark.gpu
T = torch.from_numpy
MOD, mod_id = rc.MOD, rc.mod_id
R = rc.R_DEFAULT
# Measured on MI355X, default arithmetic (split-fp16 products in the offset convolution's backward), the largest of the
# four module cases below: d offset_conv.weights 2.862e-07 and d offset_bias 2.654e-07 of the float64 gradient's
# largest entry (exact f32: 3.293e-07 and 2.654e-07).  The bound is twice the larger default figure, as
# SECOND_STAGE_BOUND of tests/test_gpu_deform.py is set.
SECOND_STAGE_BOUND = 2 * 2.862e-07


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def run_op(d, of, repulse=R):
    """(value, fit, rep, d_of) of one launch with the gradient, through the autograd Function."""
    of = of.detach().clone().requires_grad_(True)
    value, fit, rep = deform_reg.deform_reg(d["q"], d["s"], d["idx"], of, d["kp"], d["extent"], repulse)
    assert value.requires_grad and not fit.requires_grad and not rep.requires_grad
    value.backward()
    return value.detach(), fit, rep, of.grad


# ---- the operator --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
@pytest.mark.parametrize("name", list(dc.CASES))
def test_value_and_gradient_match_float64(device, name, modulated):
    case, ref = rc.case_of(name, modulated)                 # asserts the argmin gap
    d = on_device(case, device)
    of = ref["offset_features"].float().to(device)
    K, nq = case["kp"].shape[0], case["q"].shape[0]
    if "strided" in name:                                   # a column slice of a wider matrix: nbr_stride > kmax
        wide = torch.full((nq, d["idx"].shape[1] + 3), -7, dtype=d["idx"].dtype, device=device)
        wide[:, :d["idx"].shape[1]] = d["idx"]
        d["idx"] = wide[:, :case["idx"].shape[1]]
    value, fit, rep, d_of = run_op(d, of)
    e_fit = abs(float(fit) - float(ref["fit"])) / float(ref["fit"])
    e_rep = abs(float(rep) - float(ref["rep"])) / float(ref["rep"])
    e_grad = _rel(d_of, ref["d_of"])
    print(f"{name} {mod_id(modulated)}: fit {float(fit):.6f} ({e_fit:.2e}), rep {float(rep):.6f} ({e_rep:.2e}), "
          f"d_of {e_grad:.2e} of {float(ref['d_of'].abs().max()):.3e}")
    assert e_fit <= 1e-5 and e_rep <= 1e-5
    assert abs(float(value) - float(ref["value"])) <= 1e-5 * float(ref["value"])
    assert d_of.shape == of.shape and e_grad <= 1e-5
    assert float(d_of[:, 3 * K:].abs().max() if modulated else 0.0) == 0.0             # modulation logits: exactly 0
    # two runs: the same bits
    again = run_op(d, of)
    for a, b in zip((value, fit, rep, d_of), again):
        assert torch.equal(bits(a), bits(b)), "two runs differ"
    # a gradient scaled on the way in scales d_of (0.5: exactly)
    half = of.detach().clone().requires_grad_(True)
    (0.5 * deform_reg.deform_reg(d["q"], d["s"], d["idx"], half, d["kp"], d["extent"], R)[0]).backward()
    assert torch.equal(bits(half.grad), bits(0.5 * d_of))
    if nq > 2:
        # row 0 is all shadow: no fit term, and its gradient is exactly the repulsive term's -- the row's gradient when
        # EVERY row is all shadow (the same 1 / (nq K), the same offsets)
        assert bool((d["idx"][0] == case["s"].shape[0]).all())
        _, fit0, rep0, d_rep = run_op(dict(d, idx=torch.full_like(d["idx"], case["s"].shape[0])), of)
        assert float(fit0) == 0.0 and torch.equal(bits(rep0), bits(rep))
        assert torch.equal(bits(d_of[0]), bits(d_rep[0])) and float(d_rep[0].abs().max()) > 0.0
        assert not torch.equal(bits(d_of[1]), bits(d_rep[1]))


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
@pytest.mark.parametrize("name", ["nq37 k5 64-64", "nq130 k70 64-256 int64 unsorted"])
def test_the_minimum_is_the_modules_min_d2_on_rows_with_a_real_neighbour(device, name, modulated):
    """The module's min_d2 keeps the far-point contract (a shadow entry is (1e6, 1e6, 1e6)); on rows that hold a real
    neighbour it is this operator's minimum: the fit it implies and the operator's fit are both within 1e-5 of float64."""
    case, ref = rc.case_of(name, modulated)
    d = on_device(case, device)
    of = ref["offset_features"].float().to(device)
    with torch.no_grad():
        _, min_d2 = run_kernel(d, of, want_min_d2=True)
        _, fit, _ = deform_reg.deform_reg(d["q"], d["s"], d["idx"], of, d["kp"], d["extent"], R)
    real = ((case["idx"].long() >= 0) & (case["idx"].long() < case["s"].shape[0])).any(1)
    assert 0 < int(real.sum()) < real.numel() and bool((min_d2[~real.to(device)] > 1e11).all())
    e_elem = float(((min_d2.double().cpu()[real] - ref["m"][real]).abs() / ref["m"][real]).max())
    implied = float(min_d2.double().cpu()[real].sum()) / case["extent"] ** 2 / ref["m"].numel()
    e_implied = abs(implied - float(ref["fit"])) / float(ref["fit"])
    e_fit = abs(float(fit) - float(ref["fit"])) / float(ref["fit"])
    print(f"{name} {mod_id(modulated)}: min_d2 {e_elem:.2e} per element, implied fit {e_implied:.2e}, fit {e_fit:.2e}")
    assert e_elem <= 1e-5 and e_implied <= 1e-5 and e_fit <= 1e-5


def test_coincident_kernel_points(device):
    """Hand-built offsets put kernel points 1 and 2 of query 1 on one spot (deform_reg_cases.coincident_case): value and
    gradient are finite, the pair counts R^2 twice, and it contributes nothing to the gradient (upstream's sqrt yields
    NaN there)."""
    case, of, ref = rc.coincident_case()                    # asserts the argmin gap
    d = on_device(case, device)
    K, nq = case["kp"].shape[0], case["q"].shape[0]
    D = d["kp"] + d["extent"] * of.to(device)[:, :3 * K].view(-1, K, 3)
    assert torch.equal(D[1, 1], D[1, 2])
    value, fit, rep, d_of = run_op(d, of.to(device))
    assert bool(torch.isfinite(value)) and bool(torch.isfinite(d_of).all())
    e_rep, e_grad = abs(float(rep) - float(ref["rep"])) / float(ref["rep"]), _rel(d_of, ref["d_of"])
    print(f"coincident: rep {float(rep):.6f} ({e_rep:.2e}), fit {abs(float(fit) - float(ref['fit'])) / float(ref['fit']):.2e}, "
          f"d_of {e_grad:.2e}")
    assert e_rep <= 1e-5 and abs(float(fit) - float(ref["fit"])) <= 1e-5 * float(ref["fit"]) and e_grad <= 1e-5
    # The pair alone: row 1 by itself with R at half the smallest OTHER distance of the row, so that no other pair is
    # inside R.  The value is then the pair's R^2, twice, and the gradient is the fit term's alone: bit for bit the
    # gradient at R = 0, where nothing repels.
    L = (D / d["extent"])[1].double().cpu()
    dist = (L.unsqueeze(1) - L.unsqueeze(0)).norm(dim=2)
    small = 0.5 * float(dist[dist > 0].min())
    one = {k: (v[1:2] if k in ("q", "idx") else v) for k, v in d.items()}
    _, _, rep_row, d_row = run_op(one, of[1:2].to(device), repulse=small)
    assert abs(float(rep_row) * K - 2 * small * small) <= 1e-5 * 2 * small * small
    _, _, rep_none, d_none = run_op(one, of[1:2].to(device), repulse=0.0)
    assert float(rep_none) == 0.0 and float(d_none.abs().max()) > 0.0 and torch.equal(bits(d_row), bits(d_none))


def test_an_exact_tie_takes_the_lowest_column(device):
    """k* is the LOWEST column that attains the minimum.  One kernel point at two queries that both sit midway between
    two support points (exactly: +-0.03125 on the x axis), whose rows list the two points in opposite orders: equal
    values, opposite gradients, each pointing away from its row's first entry."""
    s = torch.tensor([[0.03125, 0.0, 0.0], [-0.03125, 0.0, 0.0]], device=device)
    q, kp = torch.zeros((2, 3), device=device), torch.zeros((1, 3), device=device)
    idx = torch.tensor([[0, 1, 2], [1, 0, 2]], dtype=torch.int32, device=device)       # column 2: a shadow
    e = 0.125
    value, fit, rep, d_of = run_op(dict(q=q, s=s, idx=idx, kp=kp, extent=e), torch.zeros((2, 3), device=device))
    assert float(rep) == 0.0 and float(fit) == 0.03125 ** 2 / e ** 2 and float(value) == 2 * float(fit)
    want = 4 * 0.03125 / e / 2                              # 4 (D - y*) / e / (nq K), D = 0
    assert d_of.cpu().tolist() == [[-want, 0.0, 0.0], [want, 0.0, 0.0]]


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
@pytest.mark.parametrize("name", ["nq37 k5 64-64", "nq130 k70 64-256 int64 unsorted"])
def test_without_a_gradient_the_same_numbers_and_no_gradient_buffer(device, monkeypatch, name, modulated):
    case, ref = rc.case_of(name, modulated)
    d = on_device(case, device)
    of = ref["offset_features"].float().to(device)
    value, fit, rep, _ = run_op(d, of)
    real, calls = _lib.lib(), []

    class Spy:
        def __getattr__(self, fn):
            if fn != "spr_deform_reg":
                return getattr(real, fn)
            return lambda *a: calls.append(a) or real.spr_deform_reg(*a)
    monkeypatch.setattr(_lib, "lib", lambda: Spy())
    allocated = []
    empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: allocated.append(a[0]) or empty(*a, **k))
    with torch.no_grad():
        got = deform_reg.deform_reg(d["q"], d["s"], d["idx"], of.clone().requires_grad_(True), d["kp"], d["extent"], R)
    plain = deform_reg.deform_reg(d["q"], d["s"], d["idx"], of, d["kp"], d["extent"], R)    # nothing asks for a gradient
    for v, f, r in (got, plain):
        assert not v.requires_grad
        assert torch.equal(bits(v), bits(value)) and torch.equal(bits(f), bits(fit)) and torch.equal(bits(r), bits(rep))
    assert len(calls) == 2 and all(a[15] is None for a in calls)                         # d_offset_features: NULL
    assert all(tuple(s) == (3,) for s in allocated if isinstance(s, (tuple, list, torch.Size))) and len(allocated) >= 2


# ---- through the module --------------------------------------------------------------------------------------------------
def _module(case, d, device, modulated):
    K, cin, cout = case["w"].shape
    m = deformable.KPConvDeformable(K, 3, cin, cout, case["extent"], 0.1, modulated=modulated).to(device)
    with torch.no_grad():
        for p, v in ((m.weights, d["w"]), (m.kernel_points, d["kp"]), (m.offset_conv.weights, d["off_w"]),
                     (m.offset_conv.kernel_points, d["off_kp"]), (m.offset_bias, d["off_b"])):
            p.copy_(v)
    return m


@pytest.fixture(params=[(4, 1), (0, 0)], ids=["default", "exact-f32"])
def arithmetic(request):
    """(attention mode, GEMM mode), as tests/test_gpu_kpconv_modes.py sets them."""
    attn, gemm = request.param
    ops.set_attn_mode(attn)
    ops.set_gemm_mode(gemm)
    yield request.param
    ops.set_attn_mode(ops.DEFAULT_ATTN_MODE)
    ops.set_gemm_mode(1)


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
@pytest.mark.parametrize("name", ["nq37 k5 64-64", "simple 48-40"])
def test_through_the_module(device, arithmetic, name, modulated):
    """KPConvDeformable with its flag set: forward, regulariser, backward().  The offset convolution's weights and the
    offset bias against float64 autograd through the restated offset convolution.  The block's own weights receive
    nothing.  Its input does, through the offset convolution that produced the offsets and through nothing else (as in
    KPConv's own training, where the regulariser is a function of the offset features): that gradient is held to the
    float64 one as well.
    Exact f32: within 2e-5.  Default arithmetic: measured on MI355X at most 2.862e-07 (d offset_conv.weights, `simple
    48-40` plain) and 2.654e-07 (d offset_bias, `nq37 k5 64-64` plain) of the float64 gradient's largest entry; the
    assertion is twice the larger figure (SECOND_STAGE_BOUND), itself required to be <= 1e-4."""
    case, ref = rc.chain_of(name, modulated)                # asserts the argmin gap
    d = on_device(case, device)
    m = _module(case, d, device, modulated)
    x = d["x"].clone().requires_grad_(True)
    m(d["q"], d["s"], d["idx"], x)
    assert m.reg_inputs is None and deform_reg.p2p_fitting_regularizer(m, 1.0, R) is None    # flag off: nothing kept
    m.keep_reg_inputs = True
    m(d["q"], d["s"], d["idx"], x)
    reg = deform_reg.p2p_fitting_regularizer(m, 1.0, R)
    terms = deform_reg.regularizer_terms(m, 1.0, R)
    assert reg.requires_grad and torch.equal(bits(reg), bits(terms[0]))
    assert abs(float(reg.detach()) - float(ref["value"])) <= 1e-5 * float(ref["value"])
    assert abs(float(terms[1]) - float(ref["fit"])) <= 1e-5 * float(ref["fit"])
    assert abs(float(terms[2]) - float(ref["rep"])) <= 1e-5 * float(ref["rep"])
    reg.backward()
    errs = dict(d_off_w=_rel(m.offset_conv.weights.grad, ref["d_off_w"]), d_off_b=_rel(m.offset_bias.grad, ref["d_off_b"]),
                dx=_rel(x.grad, ref["dx"]))
    print(f"module {name} {mod_id(modulated)} {arithmetic}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    bound = 2e-5 if arithmetic == (0, 0) else SECOND_STAGE_BOUND
    assert bound <= 1e-4
    assert errs["d_off_w"] <= bound and errs["d_off_b"] <= bound
    assert errs["dx"] <= 2e-5
    assert m.weights.grad is None and m.kernel_points.grad is None and m.offset_conv.kernel_points.grad is None
    # twice the power: twice the gradient
    first = None
    for power in (1.0, 2.0):
        m.zero_grad(set_to_none=True)
        m(d["q"], d["s"], d["idx"], x)
        deform_reg.p2p_fitting_regularizer(m, power, R).backward()
        first = m.offset_bias.grad.clone() if first is None else first
    assert torch.equal(bits(m.offset_bias.grad), bits(2.0 * first))


# ---- end to end ----------------------------------------------------------------------------------------------------------
KEYS = {"overlap", "feature", "T", "total"}
NEW = {"deform_reg", "deform_fit", "deform_rep"}
_runs = {}


def _config(name, **kw):
    arch, modulated = dc.ENCODER_ARCHS[name]
    return get_config('3dmatch', deformable_kpconv=True, architecture=list(arch), modulated=modulated, **kw)


def _batch(device, form="lists"):
    src, tgt, pose = synthetic.make_pair(110, seed=31, extent=0.24, jitter=0.002)       # deform_cases.encoder_clouds()
    s, t = dc.encoder_clouds()
    assert np.array_equal(s, np.ascontiguousarray(src, np.float32))
    s, t, pose = T(s).to(device), T(t).to(device), T(np.ascontiguousarray(pose, np.float32)).to(device).unsqueeze(0)
    lists = {"src_xyz": [s], "tgt_xyz": [t], "pose": pose}
    overlap.label_batch(lists, get_config('3dmatch').overlap_radius)
    if form == "lists":
        return lists
    return {"clouds": [s, t], "pairs": [(0, 1)], "pose": pose, "src_overlap": lists["src_overlap"],
            "tgt_overlap": lists["tgt_overlap"]}


def _step(name, device, form="lists", grad=True, **kw):
    """One model (parameters from the seed), forward, compute_loss and, with grad, backward: losses, parameter
    gradients and the op-level values of its deformable blocks.  Computed once per key."""
    key = (name, form, grad, tuple(sorted(kw.items())))
    if key not in _runs:
        cfg = _config(name, **kw)
        model = RegTR(cfg)
        synthetic.fill_parameters(model, seed=0)
        model = model.to(device).train()
        batch = _batch(device, form)
        with torch.enable_grad() if grad else torch.no_grad():
            pred = model(batch)
            losses = model.compute_loss(pred, batch)
            values = []
            for m in model.modules():
                if isinstance(m, deformable.KPConvDeformable) and m.reg_inputs is not None:
                    with torch.no_grad():
                        values.append(deform_reg.deform_reg(*m.reg_inputs, m.offset_features, m.kernel_points,
                                                            m.KP_extent, cfg.repulse_extent))
            if grad:
                losses["total"].backward()
        grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}
        torch.cuda.synchronize()
        _runs[key] = dict(losses={k: v.detach().clone() for k, v in losses.items()}, grads=grads, values=values,
                          requires_grad={k: v.requires_grad for k, v in losses.items()})
    return _runs[key]


def _downstream(n):
    """Parameters outside the deformable blocks and upstream of none of them, in ENCODER_ARCHS 'last' (blocks 6 and 7 of
    nine are deformable): the encoder's last block, the token projection, the position embedding, the cross-encoder, the
    overlap head, the feature criteria and the matching scalars.  Blocks 0 to 5 feed the deformable blocks' offset
    convolutions, so the regulariser reaches them."""
    return not any(n.startswith(f"kpf_encoder.encoder_blocks.{i}.") for i in range(8))


@pytest.mark.parametrize("name", ["last", "last modulated"])
def test_compute_loss_adds_the_term_and_backward_reaches_the_offsets(device, name):
    on, off = _step(name, device, deform_fitting_power=1.0), _step(name, device, deform_fitting_power=0.0)
    L = on["losses"]
    assert set(L) == KEYS | NEW and set(off["losses"]) == KEYS
    assert on["requires_grad"]["deform_reg"] and not on["requires_grad"]["deform_fit"] and not on["requires_grad"]["deform_rep"]
    for k in KEYS - {"total"}:
        assert torch.equal(bits(L[k]), bits(off["losses"][k])), k
    old = L["T"] + 0.1 * L["feature"] + L["overlap"]
    assert torch.equal(bits(old), bits(off["losses"]["total"])) and torch.equal(bits(L["total"]), bits(old + L["deform_reg"]))
    assert len(on["values"]) == 2 and not off["values"]
    assert torch.equal(bits(L["deform_reg"]), bits(on["values"][0][0] + on["values"][1][0]))
    assert torch.equal(bits(L["deform_fit"]), bits(on["values"][0][1] + on["values"][1][1]))
    assert torch.equal(bits(L["deform_rep"]), bits(on["values"][0][2] + on["values"][1][2]))
    assert float(L["deform_reg"]) > 0 and np.isfinite(float(L["total"]))
    print(f"{name}: " + ", ".join(f"{k} {float(v):.5f}" for k, v in L.items()))
    offsets = [n for n in on["grads"] if n.endswith(("offset_conv.weights", "offset_bias"))]
    assert len(offsets) == 4
    for n in offsets:
        assert not torch.equal(bits(on["grads"][n]), bits(off["grads"][n])), n
        assert bool(torch.isfinite(on["grads"][n]).all())
    same = [n for n in on["grads"] if _downstream(n)]
    assert len(same) > 100 and any(n.startswith("kpf_encoder.encoder_blocks.8.") for n in same)
    assert any(n.startswith("transformer_encoder.") for n in same) and "overlap_predictor.weight" in same
    for n in same:
        a, b = on["grads"][n], off["grads"][n]
        assert (a is None) == (b is None), n
        if a is not None:
            assert torch.equal(bits(a), bits(b)), n
    upstream = [n for n in on["grads"] if any(n.startswith(f"kpf_encoder.encoder_blocks.{i}.") for i in range(6))
                and on["grads"][n] is not None and not torch.equal(bits(on["grads"][n]), bits(off["grads"][n]))]
    assert upstream, "the regulariser reaches the blocks that feed the offset convolutions"


@pytest.mark.parametrize("name", ["last", "last modulated"])
def test_power_zero_is_todays_model(device, name):
    zero, untouched = _step(name, device, deform_fitting_power=0.0), _step(name, device)
    assert set(zero["losses"]) == set(untouched["losses"]) == KEYS
    for k in KEYS:
        assert torch.equal(bits(zero["losses"][k]), bits(untouched["losses"][k])), k
    assert set(zero["grads"]) == set(untouched["grads"])
    for n, a in zero["grads"].items():
        b = untouched["grads"][n]
        assert (a is None) == (b is None), n
        if a is not None:
            assert torch.equal(bits(a), bits(b)), n


@pytest.mark.parametrize("name", ["last", "last modulated"])
def test_under_no_grad_and_on_a_cloud_batch_the_same_values(device, name):
    train = _step(name, device, deform_fitting_power=1.0)
    quiet = _step(name, device, grad=False, deform_fitting_power=1.0)
    shared = _step(name, device, form="clouds", deform_fitting_power=1.0)
    assert set(quiet["losses"]) == set(shared["losses"]) == KEYS | NEW
    assert not any(quiet["requires_grad"].values())
    for k in sorted(NEW):
        print(f"{name} {k}: training {float(train['losses'][k]):.7f}, no_grad {float(quiet['losses'][k]):.7f}, "
              f"clouds / pairs {float(shared['losses'][k]):.7f}")
    for k in NEW:
        # the cloud batch encodes the same two clouds in the same order on the same kernels: the pair-list bits
        assert torch.equal(bits(shared["losses"][k]), bits(train["losses"][k])), k
        # Under no_grad the encoder runs its inference kernels (fused block tails, cached padded offset weights), whose
        # features agree with the training route's to float32 rounding, not in every bit: the operator itself returns
        # the same bits with and without a gradient (test_without_a_gradient_...), the offsets it is handed differ in
        # the last place.  Held to what tests/test_gpu_shared_clouds.py holds one batch's losses on two routes to.
        x, y = float(quiet["losses"][k]), float(train["losses"][k])
        assert abs(x - y) <= 5e-5 * max(1.0, abs(y)), (k, x, y)
    for n in shared["grads"]:
        if n.endswith(("offset_conv.weights", "offset_bias")):
            assert shared["grads"][n] is not None and bool(torch.isfinite(shared["grads"][n]).all())
