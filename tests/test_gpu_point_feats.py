"""GPU: per-point input features, from the small-Cin KPConv kernel (k_kpconv_few<C>, 2 <= C <= 8: spr_kpconv_fwd's
route for a first block fed colour / intensity / height) up to RegTR's batch keys.

  kernel   against forward_cases.kpconv_f64 at 1e-5 of the output scale (tests/test_gpu_stem.py::_check's bound and
           rule) over the widths, query counts around the 16-query wave and the 64-query workgroup, row widths around
           the record batches and the 64-column staged chunk, sorted / unsorted / strided / int64 rows, 1, 15 and 16
           kernel points; the count rule; KITTI-like offsets; magnitudes 1e-12 .. 1e+12 per column (per output column);
           routes within 2e-6 of scale (test_gpu_forward_range.py::test_kpconv_routes_agree's rule); batch invariance;
  backward dW / dX with the bound and helper of tests/test_gpu_backward_range.py::_kp_check;
  encoder  with input features against the reference's own KPFEncoder (tests/golden/point_feats.npz), forward at
           test_gpu_regtr.py::test_encoder_features_match_reference's bound, parameter gradients at
           test_gpu_backward.py::test_parameter_gradients_match_the_reference's encoder bounds;
  model    forward == encode + register == clouds-and-pairs bit for bit, features change the result, in_feats_dim = 1
           with explicit ones is the default forward, one augmented training step, the KITTI intensity pair.

Every features case keeps point_feats_cases.check_conditions (asserted on the CPU in tests/test_point_feats_host.py and
again here per case), so the neighbour count is the same in float32 and float64."""
import math

import numpy as np
import pytest
import torch

import forward_cases as fc
import point_feats_cases as pc
from conftest import load_golden
from superpoints_registration_amd import get_config, kitti, ops, stem, synthetic
from superpoints_registration_amd.regtr import RegTR
from superpoints_registration_amd.training import Trainer
from test_gpu_backward_range import _kp_check as bwd_check, _kp_cloud as bwd_cloud

pytestmark = pytest.mark.gpu
T = torch.from_numpy
LIST_KEYS = ("src_feat", "tgt_feat", "src_kp", "tgt_kp", "src_corr", "tgt_corr", "src_overlap", "tgt_overlap",
             "overlap_prob_list", "ind_list")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _run(device, q, s, nb, x, w, kp, ext, srt, impl=0, pad=0, int64=False):
    """pad > 0: the rows are a column slice of a wider matrix whose further columns hold VALID indices the kernel must
    not read (nbr_stride = kmax + pad)."""
    nq, kmax = nb.shape
    dt = np.int64 if int64 else np.int32
    if pad:
        wide = np.concatenate([nb, fc.rng_of(811, nq, kmax).integers(0, s.shape[0], (nq, pad))], 1).astype(dt)
        nbt = T(wide).to(device)[:, :kmax]
        assert nbt.stride(0) == kmax + pad
    else:
        nbt = T(nb.astype(dt)).to(device)
    return ops.kpconv_raw(T(q).to(device), T(s).to(device), nbt, T(x).to(device), T(w).to(device), T(kp).to(device), ext,
                          rows_sorted=srt, impl=impl)


def _close(y, ref, what, per_column=False):
    """err <= 1e-5 * scale; per_column: against each output column's own scale."""
    y = y.detach().cpu()
    assert torch.isfinite(y).all(), what
    err = np.abs(y.double().numpy() - ref)
    if per_column:
        scale, err = np.abs(ref).max(0), err.max(0)
        assert np.all(scale > 0), what
        worst = float((err / scale).max())
        print(f"{what}: worst column err / scale {worst:.3e} (ratio {worst / 1e-5:.3f})")
        assert np.all(err <= 1e-5 * scale), f"{what}: a column is off by {worst:.3e} of its scale"
    else:
        scale, err = float(np.abs(ref).max()), float(err.max())
        print(f"{what}: err {err:.3e} scale {scale:.3e} ratio {err / max(1e-5 * scale, 1e-300):.3f}")
        assert scale > 0 and err <= 1e-5 * scale, f"{what}: {err:.3e} > 1e-5 * {scale:.3e}"


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,ns,kmax,c,cout,kind,srt,n_kp", pc.SHAPE_CASES)
def test_kernel_shapes(device, nq, ns, kmax, c, cout, kind, srt, n_kp):
    """One representative per class; each with contiguous int32, strided int32 and int64 rows, twice for the bits."""
    assert stem.few_shape_ok(c, cout, n_kp)
    q, s, nb, x, w, kp, ext = pc.kernel_case(nq, ns, kmax, c, cout, 1000 + nq, kind, rows_sorted=srt, n_kp=n_kp)
    pc.check_conditions(x)
    ref = fc.kpconv_f64(q, s, nb, x, w, kp, ext)
    what = f"few C={c} cout={cout} nq={nq} kmax={kmax} srt={srt} n_kp={n_kp}"
    y = _run(device, q, s, nb, x, w, kp, ext, srt)
    _close(y, ref, what)
    assert torch.equal(_bits(y), _bits(_run(device, q, s, nb, x, w, kp, ext, srt))), "two launches differ"
    assert torch.equal(_bits(y), _bits(_run(device, q, s, nb, x, w, kp, ext, srt, pad=3))), "strided rows differ"
    assert torch.equal(_bits(y), _bits(_run(device, q, s, nb, x, w, kp, ext, srt, int64=True))), "int64 rows differ"
    if nq > 3 and srt:
        assert np.all(nb[3] == ns) and torch.equal(y[3].cpu(), torch.zeros(cout)), "a row of only shadow entries is exactly zero"
    if srt:       # sorted rows read as unsorted ones (no early stop): the same sums in the same order
        assert torch.equal(_bits(y), _bits(_run(device, q, s, nb, x, w, kp, ext, False)))


@pytest.mark.parametrize("kind", pc.COUNT_KINDS)
@pytest.mark.parametrize("c", [2, 4, 8])
def test_count_rule(device, c, kind):
    """neighbor_num = valid neighbours whose feature sum is > 0, at least 1; a neighbour that is not counted still adds
    its features.  'negative': nothing counts, the divisor is 1 and the output the plain weighted sum; 'integer': rows
    with exact-zero and -1 sums, queries that see only those; 'signed': both kinds in every row.  The divisor read off
    the output (y = U / count, U the float64 un-normalised sum) equals the restatement's count."""
    nq, ns, kmax, cout, ext = 90, 160, 10, 64, 0.125
    q, s, nb, x, w, kp, _ = pc.kernel_case(nq, ns, kmax, c, cout, 1200 + c, kind, ext=ext, fill=0.8)
    pc.check_conditions(x)
    if kind == "integer":
        nb[5:25] = np.where(nb[5:25] < ns, nb[5:25] % (ns // 2), ns)      # queries 5..24 see only rows with sum <= 0
    cnt = pc.count_f64(nb, x)
    if kind == "negative":
        assert cnt.max() == 0
    elif kind == "integer":
        assert np.all(cnt[5:25] == 0) and cnt.max() > 1
    else:
        valid = (nb < ns).sum(1)
        assert np.any((cnt > 0) & (cnt < valid)) and cnt.max() > 1
    ref = fc.kpconv_f64(q, s, nb, x, w, kp, ext)
    y = _run(device, q, s, nb, x, w, kp, ext, True)
    _close(y, ref, f"few counts C={c} {kind}")
    assert torch.equal(y[3].cpu(), torch.zeros(cout))
    U = ref * np.maximum(cnt, 1)[:, None]
    yd = y.cpu().double().numpy()
    den = (yd * yd).sum(1)
    live = den > 0
    got = np.round((U * yd).sum(1)[live] / den[live])
    assert live.sum() >= nq - 2 and np.array_equal(got, np.maximum(cnt, 1)[live].astype(np.float64))
    if kind == "negative":                     # divisor 1: the output is still the weighted sum, not zero
        assert float(np.abs(yd).max()) > 0 and np.array_equal(np.maximum(cnt, 1), np.ones(nq, np.int64))


@pytest.mark.parametrize("offset,ext", [(1e2, 0.03), (1e3, 0.03), (1e2, 0.6), (1e3, 5.0)])
@pytest.mark.parametrize("c", [3, 8])
def test_offset_coordinates(device, c, offset, ext):
    """test_gpu_forward_range.py::test_kpconv_offset_coordinates' geometry: large absolute coordinates, small
    differences; sorted and unsorted rows."""
    for srt in (True, False):
        q, s, nb = fc.kp_cloud_case(300, 350, 20, offset, ext, 41, rows_sorted=srt)
        x, w, kp = pc.features(350, c, 1300 + c, "signed"), fc.kp_weights(c, 64, 43), fc.random_kernel_points(ext, 44)
        y = _run(device, q, s, nb, x, w, kp, ext, srt)
        _close(y, fc.kpconv_f64(q, s, nb, x, w, kp, ext), f"few C={c} offset {offset:g} ext {ext:g} srt={srt}")


@pytest.mark.parametrize("c", [2, 5, 8])
def test_magnitudes_per_column(device, c):
    """Feature columns at 1e-12 .. 1e+12, each its own; weights at 1e-12 .. 1e+12 per output column.  The result is
    float32, so every output column is held to 1e-5 of ITS scale in the float64 result."""
    q, s, nb = fc.kp_cloud_case(200, 260, 30, 1e2, 0.125, 71, rows_sorted=True)
    x, xm = pc.magnitude_features(260, c, 1400 + c)
    w, wm = pc.magnitude_weights(c, 40, 1410 + c)
    pc.check_conditions(x)
    assert xm.max() / xm.min() >= 1e23 and wm.max() / wm.min() >= 1e15
    kp = fc.random_kernel_points(0.125, 72)
    y = _run(device, q, s, nb, x, w, kp, 0.125, True)
    _close(y, fc.kpconv_f64(q, s, nb, x, w, kp, 0.125), f"few magnitudes C={c}", per_column=True)


@pytest.mark.parametrize("c,cout", [(2, 64), (4, 64), (8, 40)])
def test_routes_agree(device, c, cout):
    """impl 0 and 2 (the small-Cin kernel) and impl 1 (the generic kernel, what these shapes ran on before) within 2e-6
    of scale -- test_gpu_forward_range.py::test_kpconv_routes_agree's data and rule; 0 and 2 are the same launch."""
    ext = 0.0625
    q, s, nb = fc.kp_cloud_case(333, 400, 37, 1e3, ext, 59, rows_sorted=True)
    x, w, kp = pc.features(400, c, 1500 + c, "signed"), fc.kp_weights(c, cout, 61), fc.random_kernel_points(ext, 62)
    ys = {impl: _run(device, q, s, nb, x, w, kp, ext, True, impl=impl).cpu().double() for impl in (0, 1, 2)}
    scale = float(ys[1].abs().max())
    for a, b in ((0, 1), (0, 2), (1, 2)):
        d = float((ys[a] - ys[b]).abs().max())
        print(f"few {c}->{cout}: impl {a} vs {b}: {d / scale:.3e}")
        assert d <= 2e-6 * scale, f"kpconv {c}->{cout}: impl {a} vs {b}: {d / scale:.3e}"
    assert torch.equal(ys[0], ys[2])


@pytest.mark.parametrize("c", [2, 4, 8])
def test_batch_invariance(device, c):
    """A cloud alone and between two others (its queries then start inside a wave, with other wave mates and another
    stop): the same bits."""
    ext = 0.125
    parts = [pc.kernel_case(nq, ns, 24, c, 64, 1600 + i, "signed", ext=ext) for i, (nq, ns) in enumerate([(37, 50), (150, 170), (21, 40)])]
    w, kp = parts[1][4], parts[1][5]
    alone = _run(device, *parts[1][:4], w, kp, ext, True)
    tot = sum(p[1].shape[0] for p in parts)
    qs, ss, xs, nbs, off = [], [], [], [], 0
    for q, s, nb, x, *_ in parts:
        qs.append(q), ss.append(s), xs.append(x)
        nbs.append(np.where(nb < s.shape[0], nb + off, tot))
        off += s.shape[0]
    both = _run(device, np.concatenate(qs), np.concatenate(ss), np.concatenate(nbs), np.concatenate(xs), w, kp, ext, True)
    assert torch.equal(_bits(both[37:37 + 150]), _bits(alone))


# ---- 2. backward -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,mx,mg", [(2, 1.0, 1.0), (4, 1e3, 1e-8), (8, 1e-5, 1e15)])
def test_backward_dw_and_dx(device, c, mx, mg):
    """dW of a C -> 64 layer (the float64-accumulated product, as Cin = 1) and dX (the generic scatter route) against the
    float64 restatement: test_gpu_backward_range.py::test_kpconv_backward_pooling_neighbourhoods' geometry, bound and
    helper.  Features non-negative, so the count is the same at every scale."""
    q, s, nb, kp, ext = bwd_cloud(700)
    x = synthetic.rand((s.shape[0], c), 701, 0.0, 1.0) * mx
    x[::7] = 0.0
    w = synthetic.rand((15, c, 64), 702) * 0.1
    go = synthetic.rand((q.shape[0], 64), 703) * mg
    bwd_check(device, q, s, nb, kp, ext, x, w, go, f"few backward C={c} |x|~{mx:g} |dout|~{mg:g}")


def _order_dependent_rows(ns, c, seed):
    """test_gpu_backward_range.py::test_kpconv_backward_counts_like_the_forward's rows at width c: a quarter all zero,
    two quarters {1, -1, +-2^-30} at drawn positions (the float32 sum is 0 or +-2^-30 depending on where the small term
    meets the pair), a quarter random.  These rows are OUTSIDE point_feats_cases' condition on purpose: the kernel is
    compared with the routes that count by k_rowflag, not with float64."""
    g = torch.Generator().manual_seed(seed)
    x = synthetic.rand((ns, c), seed + 1)
    for r in range(ns):
        kind = r % 4
        if kind == 3:
            continue
        x[r] = 0.0
        if kind == 0:
            continue
        i, j, l = torch.randperm(c, generator=g)[:3].tolist()
        x[r, i], x[r, j] = 1.0, -1.0
        x[r, l] = 2.0 ** -30 if kind == 1 else -(2.0 ** -30)
    return x


@pytest.mark.parametrize("c", [3, 4, 5, 8])
def test_count_is_the_row_flags_in_forward_and_backward(device, c):
    """The record pass restates k_rowflag's summation order.  On rows whose sum has an order-dependent sign, the kernel
    (impl 0) agrees with the generic kernel (impl 1, which reads k_rowflag's flags) within the routes' 2e-6 -- one
    neighbour counted differently changes a row by 1 / count -- and the backward, which counts by k_rowflag, divides by
    the count the forward used (test_gpu_backward_range.py's helper reads that count off the forward's output)."""
    q, s, nb, kp, ext = bwd_cloud(710, kmax=70)
    x = _order_dependent_rows(s.shape[0], c, 711 + c)
    w = synthetic.rand((15, c, 64), 713) * 0.1
    args = (q.to(device), s.to(device), nb.to(torch.int32).to(device), x.to(device), w.to(device), kp.to(device), ext)
    ys = {impl: ops.kpconv_raw(*args, rows_sorted=True, impl=impl).cpu().double() for impl in (0, 1)}
    scale = float(ys[1].abs().max())
    d = float((ys[0] - ys[1]).abs().max())
    print(f"few count C={c}: impl 0 vs 1: {d / scale:.3e}")
    assert d <= 2e-6 * scale
    bwd_check(device, q, s, nb, kp, ext, x, w, synthetic.rand((q.shape[0], 64), 714), f"few count C={c}")


# ---- 3. the encoder against the reference ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_run(device):
    """The fixture's pair through RegTR's own entry (the batch keys), in training mode with the tape: the un-projected
    encoder output caught at the last block, then its backward for the fixture's cotangent.  Computed once."""
    g = load_golden("point_feats.npz")
    src, tgt, fs, ft = pc.golden_inputs()
    model = RegTR(get_config("3dmatch", in_feats_dim=pc.GOLDEN_C))
    synthetic.fill_parameters(model.kpf_encoder, seed=int(g["seed"]))
    model = model.to(device).train()
    caught = []
    hook = model.kpf_encoder.encoder_blocks[-1].register_forward_hook(lambda m, a, o: caught.append(o))
    batch = {"src_xyz": [T(src).to(device)], "tgt_xyz": [T(tgt).to(device)],
             "src_point_feats": [T(fs).to(device)], "tgt_point_feats": [T(ft).to(device)]}
    with torch.enable_grad():
        model(batch)
    hook.remove()
    assert len(caught) == 1
    feats_un = caught[0]
    model.zero_grad(set_to_none=True)
    feats_un.backward(pc.golden_cotangent(feats_un.shape).to(device))
    return g, model, feats_un.detach(), batch


def test_encoder_features_match_reference(golden_run):
    g, model, feats_un, batch = golden_run
    assert np.array_equal(model.kpf_encoder.encoder_blocks[0].KPConv.kernel_points.detach().cpu().numpy(), g["kernel_points0"])
    assert [int(v) for v in batch["kpconv_meta"]["_lens_host"][-1]] == [int(v) for v in g["lens"]]
    ref = g["feats_un"]
    assert feats_un.shape == ref.shape
    err = np.abs(feats_un.cpu().numpy() - ref).max() / np.abs(ref).max()
    print(f"encoder with input features: {err:.3e} of the scale")
    assert err <= 2e-5


def test_encoder_gradients_match_reference(golden_run):
    """The first block's dW whole, every other encoder tensor by norm and 64 pinned entries:
    | ||g|| - ||r|| | <= 5e-4 ||r|| and the RMS deviation of the entries <= 2e-2 of their RMS (the encoder bounds of
    test_gpu_backward.py::test_parameter_gradients_match_the_reference)."""
    g, model, _, _ = golden_run
    n, report = 0, []
    for name, p in model.kpf_encoder.named_parameters():
        if f"{name}|none" in g:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        if not p.requires_grad:
            continue
        assert p.grad is not None, name
        gr = p.grad.detach().double().reshape(-1).cpu().numpy()
        ref_norm = float(g[f"{name}|norm"])
        if f"{name}|full" in g:
            ref_e, got_e = g[f"{name}|full"].astype(np.float64), gr
            assert name == "encoder_blocks.0.KPConv.weights" and gr.size == 15 * pc.GOLDEN_C * 64
        else:
            ref_e, got_e = g[f"{name}|samples"].astype(np.float64), gr[pc.grad_sample_indices(name, gr.size)]
        rms = np.sqrt(np.mean((got_e - ref_e) ** 2)) / max(np.sqrt(np.mean(ref_e ** 2)), 1e-30)
        nerr = abs(np.linalg.norm(gr) - ref_norm) / max(ref_norm, 1e-30)
        report.append((max(rms, nerr), name, rms, nerr))
        assert nerr <= 5e-4, f"{name}: norm deviates by {nerr:.2e}"
        assert rms <= 2e-2, f"{name}: RMS deviation {rms:.2e}"
        n += 1
    report.sort(reverse=True)
    print(f"{n} encoder tensors; worst: " + ", ".join(f"{nm} rms {r:.1e} norm {e:.1e}" for _, nm, r, e in report[:3]))
    # every gradient the fixture holds was compared (the 3DMatch encoder: 8 blocks, 25 weight tensors)
    assert n == sum(1 for k in g if k.endswith("|norm")) >= 25
    assert any(nm == "encoder_blocks.0.KPConv.weights" for _, nm, _, _ in report)


# ---- 4. the model -------------------------------------------------------------------------------------------------------------
def _pairs(device, n=1100):
    made = [synthetic.make_pair(n + 90 * i, seed=40 + i, extent=0.45, jitter=0.002, trans=(0.03, -0.02, 0.01)) for i in range(2)]
    src = [T(np.ascontiguousarray(p[0][:n - 100 * i])).to(device) for i, p in enumerate(made)]
    tgt = [T(np.ascontiguousarray(p[1])).to(device) for p in made]
    pose = T(np.stack([p[2] for p in made])).to(device)
    return src, tgt, pose


def _assert_bitwise(a, b):
    assert torch.equal(_bits(a["pose"]), _bits(b["pose"]))
    for key in LIST_KEYS:
        assert len(a[key]) == len(b[key])
        for x, y in zip(a[key], b[key]):
            assert x.dtype == y.dtype and torch.equal(x, y), key


@pytest.fixture(scope="module")
def feat_model(device):
    model = RegTR(get_config("3dmatch", in_feats_dim=4))
    synthetic.fill_parameters(model, seed=0)
    model = model.to(device).eval()
    src, tgt, pose = _pairs(device)
    lens = [int(c.shape[0]) for c in src + tgt]
    feats = pc.model_feats(lens, 4, 1700, device)
    fwd = model({"src_xyz": src, "tgt_xyz": tgt, "src_point_feats": feats[:2], "tgt_point_feats": feats[2:]})
    return dict(model=model, src=src, tgt=tgt, pose=pose, feats=feats, fwd=fwd, lens=lens)


def test_forward_encode_register_and_cloud_batch_agree_bitwise(feat_model):
    m = feat_model
    model, src, tgt, feats = m["model"], m["src"], m["tgt"], m["feats"]
    enc = model.encode(src + tgt, point_feats=feats)
    _assert_bitwise(model.register(enc, [(0, 2), (1, 3)]), m["fwd"])
    shared = model({"clouds": src + tgt, "pairs": [(0, 2), (1, 3)], "cloud_point_feats": feats})
    _assert_bitwise(shared, m["fwd"])
    assert all(bool(torch.isfinite(p).all()) for p in m["fwd"]["pose"])
    with pytest.raises(ValueError, match="in_feats_dim = 4"):
        model.encode(src + tgt)
    with pytest.raises(ValueError, match=r"clouds\[1\]"):
        model.encode(src + tgt, point_feats=[feats[0], feats[1][:-1]] + feats[2:])
    with pytest.raises(ValueError, match="the target of pair 0"):
        model({"src_xyz": src, "tgt_xyz": tgt, "src_point_feats": feats[:2], "tgt_point_feats": [feats[2].cpu(), feats[3]]})


def test_features_change_the_result(feat_model):
    m = feat_model
    other = pc.model_feats(m["lens"], 4, 1800, m["src"][0].device)
    out = m["model"]({"src_xyz": m["src"], "tgt_xyz": m["tgt"], "src_point_feats": other[:2], "tgt_point_feats": other[2:]})
    for b in range(2):
        assert out["src_feat"][b].shape == m["fwd"]["src_feat"][b].shape
        assert not torch.equal(out["src_feat"][b], m["fwd"]["src_feat"][b])
        assert not torch.equal(out["tgt_feat"][b], m["fwd"]["tgt_feat"][b])
    assert not torch.equal(out["pose"], m["fwd"]["pose"])


def test_width_one_with_explicit_ones_is_the_default_forward(device):
    model = RegTR(get_config("3dmatch"))
    synthetic.fill_parameters(model, seed=0)
    model = model.to(device).eval()
    src, tgt, _ = _pairs(device)
    ones = [torch.ones((int(c.shape[0]), 1), dtype=torch.float32, device=device) for c in src + tgt]
    a = model({"src_xyz": src, "tgt_xyz": tgt})
    b = model({"src_xyz": src, "tgt_xyz": tgt, "src_point_feats": ones[:2], "tgt_point_feats": ones[2:]})
    _assert_bitwise(a, b)
    half = [0.5 * o for o in ones]                      # [n, 1] features are used as given
    c = model({"src_xyz": src, "tgt_xyz": tgt, "src_point_feats": half[:2], "tgt_point_feats": half[2:]})
    assert all(bool(torch.isfinite(x).all()) for x in c["src_feat"])


def test_training_step_with_augmentation_carries_the_features(device):
    """One Trainer.train_step(augment=True) on a batch with features: it runs, and the features the model received are
    the caller's gathered by the permutation the augmentation reports, sides exchanged where the pair swapped."""
    cfg = get_config("3dmatch", in_feats_dim=4)
    model = RegTR(cfg)
    synthetic.fill_parameters(model, seed=0)
    model = model.to(device)
    src, tgt, pose = _pairs(device, n=900)
    lens = [int(c.shape[0]) for c in src + tgt]
    feats = pc.model_feats(lens, 4, 1900, device)
    for f in feats:                                      # column 1 = the point's own row: the gather is visible
        f[:, 1] = torch.arange(f.shape[0], device=device, dtype=torch.float32) / f.shape[0]
    batch = {"src_xyz": src, "tgt_xyz": tgt, "pose": pose, "src_point_feats": feats[:2], "tgt_point_feats": feats[2:]}
    keys = sorted(batch)
    seen = []
    hook = model.register_forward_pre_hook(lambda m, args: seen.append(args[0]))
    tr = Trainer(cfg, augment=True, seed=23).setup(model)
    losses = tr.train_step(model, batch)
    hook.remove()
    assert all(bool(torch.isfinite(v).all()) for v in losses.values()), losses
    assert sorted(batch) == keys and batch["src_point_feats"][0] is feats[0]      # the caller's batch stays as it is
    aug = seen[0]
    _, swap, _ = ops.augment_draw(23, tr._pair_keys(2), cfg.perturb_pose)
    for b in range(2):
        for side, own, other in (("src", feats[b], feats[2 + b]), ("tgt", feats[2 + b], feats[b])):
            perm, got = aug[f"{side}_perm"][b], aug[f"{side}_point_feats"][b]
            origin = other if bool(swap[b]) else own
            assert got.shape[0] == aug[f"{side}_xyz"][b].shape[0] == perm.shape[0] == origin.shape[0]
            assert torch.equal(torch.sort(perm).values, torch.arange(origin.shape[0], device=device))
            assert not torch.equal(perm, torch.arange(origin.shape[0], device=device))
            assert torch.equal(got, origin[perm])


def test_kitti_pair_with_intensity_runs_end_to_end(device):
    """The README example: raw [n, 4] scans -> kitti.prepare_pairs(intensity=True) -> RegTR(in_feats_dim = 2)."""
    cfg = get_config("kitti", in_feats_dim=2)
    model = RegTR(cfg)
    synthetic.fill_parameters(model, seed=0)
    model = model.to(device).eval()
    rng = np.random.default_rng(3)
    src, tgt, pose = synthetic.make_lidar_pair(n=20000, seed=5)
    raw = [T(np.concatenate([c, rng.random((c.shape[0], 1)).astype(np.float32)], 1)).to(device) for c in (src, tgt)]
    batch = kitti.prepare_pairs([raw[0]], [raw[1]], cfg, pose=T(pose[None]).to(device), intensity=True)
    for side, scan in (("src", raw[0]), ("tgt", raw[1])):
        f, idx = batch[f"{side}_point_feats"][0], batch[f"{side}_index"][0]
        assert f.dtype == torch.float32 and f.shape == (batch[f"{side}_xyz"][0].shape[0], 2)
        assert torch.equal(f[:, 0], torch.ones_like(f[:, 0])) and torch.equal(f[:, 1], scan[idx, 3])
    out = model(batch)
    assert out["pose"].shape == (1, 3, 4) and bool(torch.isfinite(out["pose"]).all())
    plain = kitti.prepare_pairs([raw[0]], [raw[1]], cfg)
    assert "src_point_feats" not in plain and torch.equal(plain["src_xyz"][0], batch["src_xyz"][0])
