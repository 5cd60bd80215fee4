"""GPU: the KPConv decoder -- spr_upsample_unary (csrc/upsample_unary.hip) and its operator route against float64,
across magnitudes, batch-invariant, between poisoned guard bands; KPFDecoder against the reference's golden
(tests/golden/decoder_3dmatch.npz), end to end from points, and its gradients against float64 autograd."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import decoder_cases as dc
from conftest import load_golden
from oracle.gen_golden import grad_sample_indices
from superpoints_registration_amd import _lib, decoder, get_config, ops, synthetic
from superpoints_registration_amd.kpconv import KPFDecoder, KPFEncoder, Preprocessor
from tensor_arena import TensorArena
from workspace_arena import GUARD, Arena

pytestmark = pytest.mark.gpu
T = torch.from_numpy
F64 = torch.float64

TILE = 128                    # rows of a workgroup's tile in split-fp16 mode; the exact-f32 kernel's is TILE / 2
NS = sorted({1, 31, 32, 33, TILE // 2 - 1, TILE // 2 + 1, TILE - 1, TILE + 1, 2 * TILE + 3})
SHAPES = [(32, 32, 64), (64, 32, 64), (256, 128, 128)]
STRIDES = (1, 7, 40)
NCS = (1, 5, 300)
PATTERNS = ("one", "descending", "shadow", "all_shadow")


@pytest.fixture(autouse=True)
def _default_mode():
    yield
    ops.set_gemm_mode(1)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _indices(pattern, n, nc):
    i = np.arange(n)
    if pattern == "one":
        idx = np.full(n, nc - 1)
    elif pattern == "descending":                            # a descending walk with every coarse row used twice
        idx = (nc - 1 - (i // 2) % nc)
    elif pattern == "shadow":                                # a third shadow, some beyond it, some negative
        idx = (7 * i + 3) % nc
        idx = np.where(i % 3 == 0, nc, idx)
        idx = np.where(i % 11 == 4, nc + 5, idx)
        idx = np.where(i % 13 == 6, -1, idx)
    else:
        idx = np.full(n, nc)
    return idx.astype(np.int64)


def _matrix(idx, stride, device):
    """idx as column 0 of an int32 [n, stride] matrix whose other columns hold indices that must not be read."""
    m = np.full((len(idx), stride), 2 ** 30, np.int32)
    m[:, 0] = idx
    return T(m).to(device)


def _ref64(xc, xs, idx, w):
    ext = torch.cat([xc.double(), torch.zeros(1, xc.shape[1], dtype=F64)])
    ii = T(np.where((idx < 0) | (idx >= xc.shape[0]), xc.shape[0], idx))
    return torch.cat([ext[ii], xs.double()], 1) @ w.double().t()


def _ref32(xc, xs, idx, w):
    ext = torch.cat([xc, torch.zeros(1, xc.shape[1])])
    ii = T(np.where((idx < 0) | (idx >= xc.shape[0]), xc.shape[0], idx))
    return torch.cat([ext[ii], xs], 1) @ w.t()


def _check(got, ref, bound, what):
    err, scale = float((got.double().cpu() - ref).abs().max()), float(ref.abs().max())
    assert torch.isfinite(got).all(), what
    assert scale > 0 and err <= bound * scale, f"{what}: err {err:.3e} > {bound:g} * {scale:.3e}"


# ---- 1. the operator against float64 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kc,ks,n_out", SHAPES)
@pytest.mark.parametrize("route", ["fused", "operator"])
@pytest.mark.parametrize("mode", [1, 0])
def test_upsample_unary_against_float64(device, mode, route, kc, ks, n_out):
    """err <= 2e-6 * max(1, K // 256) * scale, K = kc + ks: the criterion of test_gpu_ops.py::test_linear_exact_f32 for
    the concatenated product.  Every n x index pattern x index row stride x coarse row count."""
    ops.set_gemm_mode(mode)
    bound = 2e-6 * max(1, (kc + ks) // 256)
    xc, xs = synthetic.rand((max(NCS), kc), 11, -3.0, 3.0), synthetic.rand((max(NS), ks), 12, -3.0, 3.0)
    w = synthetic.rand((n_out, kc + ks), 13, -0.2, 0.2)
    xc_d, xs_d, w_d = xc.to(device), xs.to(device), w.to(device)
    for n, nc, pattern, stride in itertools.product(NS, NCS, PATTERNS, STRIDES):
        idx = _indices(pattern, n, nc)
        y = decoder.upsample_unary(xc_d[:nc], xs_d[:n], _matrix(idx, stride, device), w_d, route=route)
        assert y.shape == (n, n_out) and y.dtype == torch.float32
        ref = xs[:n].double() @ w[:, kc:].double().t() if pattern == "all_shadow" else _ref64(xc[:nc], xs[:n], idx, w)
        _check(y, ref, bound, f"mode {mode} {route} n={n} nc={nc} {pattern} stride {stride}")


@pytest.mark.parametrize("route", ["fused", "operator"])
@pytest.mark.parametrize("mode", [1, 0])
def test_upsample_unary_widest_shape(device, mode, route):
    """(kc, ks, n_out) = (1024, 512, 512) at n = 33: 48 K slabs, four column tiles."""
    ops.set_gemm_mode(mode)
    kc, ks, n_out, n = 1024, 512, 512, 33
    xc, xs = synthetic.rand((300, kc), 21, -3.0, 3.0), synthetic.rand((n, ks), 22, -3.0, 3.0)
    w = synthetic.rand((n_out, kc + ks), 23, -0.2, 0.2)
    for nc, pattern, stride in itertools.product(NCS, PATTERNS, STRIDES):
        idx = _indices(pattern, n, nc)
        y = decoder.upsample_unary(xc[:nc].to(device), xs.to(device), _matrix(idx, stride, device), w.to(device),
                                   route=route)
        ref = xs.double() @ w[:, kc:].double().t() if pattern == "all_shadow" else _ref64(xc[:nc], xs, idx, w)
        _check(y, ref, 2e-6 * ((kc + ks) // 256), f"mode {mode} {route} nc={nc} {pattern} stride {stride}")


def test_one_dimensional_and_int64_indices(device):
    xc, xs, w = synthetic.rand((5, 64), 31), synthetic.rand((33, 32), 32), synthetic.rand((64, 96), 33)
    idx = _indices("shadow", 33, 5)
    want = decoder.upsample_unary(xc.to(device), xs.to(device), _matrix(idx, 7, device), w.to(device), route="fused")
    for form in (T(idx).to(device), T(idx.astype(np.int32)).to(device), T(idx).to(device)[:, None].expand(33, 3),
                 _matrix(idx, 7, device)[:, 0], T(idx.astype(np.int32)).to(device)[:, None].expand(33, 3)):
        for route in ("fused", "operator", None):
            y = decoder.upsample_unary(xc.to(device), xs.to(device), form, w.to(device), route=route)
            _check(y, _ref64(xc, xs, idx, w), 2e-6, f"{form.dtype} {tuple(form.shape)} {route}")
            if route != "operator":
                assert torch.equal(_bits(y), _bits(want))


# ---- 2. magnitudes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["fused", "operator"])
@pytest.mark.parametrize("mode", [1, 0])
def test_upsample_unary_across_magnitudes(device, mode, route):
    """xc and xs scaled independently by 1e-6, 1, 1e+6 at (64, 32, 64), n = 33: err <= max(2e-6 * scale, 4 * err32),
    err32 = the float32 torch evaluation of the same formula (test_gpu_forward_range._bounded).  The two sources share
    one scale in split-fp16 mode, so the smaller one keeps an absolute error of 2^-39 of the larger one's maximum."""
    ops.set_gemm_mode(mode)
    kc, ks, n_out, n, nc = 64, 32, 64, 33, 5
    xc0, xs0 = synthetic.rand((nc, kc), 41, -3.0, 3.0), synthetic.rand((n, ks), 42, -3.0, 3.0)
    w = synthetic.rand((n_out, kc + ks), 43, -0.2, 0.2)
    idx = _indices("shadow", n, nc)
    for a, b in itertools.product((1e-6, 1.0, 1e6), repeat=2):
        xc, xs = (xc0 * a).float(), (xs0 * b).float()
        y = decoder.upsample_unary(xc.to(device), xs.to(device), _matrix(idx, 7, device), w.to(device), route=route)
        ref = _ref64(xc, xs, idx, w)
        err32 = float((_ref32(xc, xs, idx, w).double() - ref).abs().max())
        err, scale = float((y.double().cpu() - ref).abs().max()), float(ref.abs().max())
        print(f"mode {mode} {route} xc*{a:g} xs*{b:g}: err {err:.3e} scale {scale:.3e} err32 {err32:.3e}")
        assert torch.isfinite(y).all() and err <= max(2e-6 * scale, 4 * err32), (a, b, err, scale, err32)


# ---- 3. batch invariance, n = 0 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kc,ks,n_out", [(64, 32, 64), (256, 128, 128)])
@pytest.mark.parametrize("mode", [1, 0])
def test_rows_do_not_depend_on_their_batch(device, mode, kc, ks, n_out):
    """The rows of one cloud computed alone (its own coarse rows, indices rebased) and as the middle of three clouds of
    other lengths (another tile position, other tile mates) carry the same bits.  In split-fp16 mode a row's bits also
    depend on the two power-of-two scales; the largest |xc| entry is placed in the middle cloud so that both calls
    measure the same range."""
    ops.set_gemm_mode(mode)
    fine, coarse = (70, 150, 45), (30, 60, 20)
    f0, c0 = np.concatenate([[0], np.cumsum(fine)]), np.concatenate([[0], np.cumsum(coarse)])
    xc, xs = synthetic.rand((sum(coarse), kc), 51, -3.0, 3.0), synthetic.rand((sum(fine), ks), 52, -3.0, 3.0)
    xc[c0[1] + 3, 5] = 64.0
    w = synthetic.rand((n_out, kc + ks), 53, -0.2, 0.2).to(device)
    rng = np.random.default_rng(5)
    idx = np.concatenate([c0[k] + rng.integers(0, coarse[k] + 1, fine[k]) for k in range(3)])
    idx = np.where(idx >= np.repeat(c0[1:], fine), sum(coarse), idx)            # a cloud's own shadow -> the batch's
    batch = decoder.upsample_unary(xc.to(device), xs.to(device), _matrix(idx, 7, device), w, route="fused")
    mid = idx[f0[1]:f0[2]]
    mid = np.where(mid >= sum(coarse), coarse[1], mid - c0[1])
    alone = decoder.upsample_unary(xc[c0[1]:c0[2]].to(device), xs[f0[1]:f0[2]].to(device), _matrix(mid, 1, device), w,
                                   route="fused")
    assert (mid == coarse[1]).any() and torch.equal(_bits(alone), _bits(batch[f0[1]:f0[2]]))


@pytest.mark.parametrize("route", ["fused", "operator", None])
@pytest.mark.parametrize("mode", [1, 0])
def test_no_rows(device, mode, route):
    ops.set_gemm_mode(mode)
    xc, w = synthetic.rand((5, 64), 61).to(device), synthetic.rand((64, 96), 62).to(device)
    y = decoder.upsample_unary(xc, torch.empty((0, 32), device=device), torch.empty((0, 7), dtype=torch.int32, device=device),
                               w, route=route)
    torch.cuda.synchronize()
    assert y.shape == (0, 64) and y.dtype == torch.float32
    # the entry point itself accepts n = 0 and launches nothing
    n_host = ctypes.c_int(-1)
    ws = torch.empty(_lib.lib().spr_upsample_unary_workspace_size(), dtype=torch.uint8, device=device)
    rc = _lib.lib().spr_upsample_unary(ops._ptr(xc), 5, 64, None, 0, 32, None, 1, ops._ptr(w), 64, None, None, 0, None, 0,
                                       None, 0, None, 0, ctypes.byref(n_host), ops._ptr(ws), ws.numel(), ops._stream(xc))
    torch.cuda.synchronize()
    assert rc == 0 and n_host.value == 0


# ---- 4. inside its tensors and its workspace ----------------------------------------------------------------------------
@pytest.mark.parametrize("kc,ks,n_out,n", [(64, 32, 64, 2 * TILE + 3), (256, 128, 128, TILE + 1), (32, 32, 96, 33)])
@pytest.mark.parametrize("mode", [1, 0])
def test_fused_call_inside_its_tensors_and_workspace(device, monkeypatch, mode, kc, ks, n_out, n):
    """The fused call with every device tensor between guard bands (both flavours of tensor_arena.TensorArena) and
    exactly the reported workspace between guard bands (workspace_arena.Arena, both poisons): bit-equal to production,
    no band touched, no input written."""
    ops.set_gemm_mode(mode)
    nc = 5
    xc, xs = synthetic.rand((nc, kc), 71, -3.0, 3.0).to(device), synthetic.rand((n, ks), 72, -3.0, 3.0).to(device)
    w = synthetic.rand((n_out, kc + ks), 73, -0.2, 0.2).to(device)
    idx = _indices("shadow", n, nc)

    def f(put):
        # the index matrix has one column: its last element is flush against the rear band
        ins = [put(t) for t in (xc, xs, _matrix(idx, 1, device), w.clone())]
        keep = [t.clone() for t in ins]
        y = decoder.upsample_unary(*ins, route="fused")
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(ins, keep)), "an input was written"
        r, rn = ops._get_range(y)
        assert (rn > 0) == (mode == 1)
        if rn:                                              # the published range bounds the result, tightly
            assert float(r[:rn].max()) == float(y.abs().max())
        return y
    production = f(lambda t: t)
    _check(production, _ref64(xc.cpu(), xs.cpu(), idx, w.cpu()), 2e-6 * max(1, (kc + ks) // 256), "production")
    for flavour, poison in ((1, 0xFF), (2, 0x00), (1, 0x00), (2, 0xFF)):
        tensors, arena = TensorArena(flavour, GUARD), Arena(poison)
        with monkeypatch.context() as m:
            tensors.install(m)
            m.setattr(ops, "_workspace", arena)
            guarded = f(tensors.put)
        tensors.verify()
        arena.verify()
        assert arena.calls == 1 and tensors.calls >= 6, (arena.calls, tensors.calls)
        assert torch.equal(_bits(production), _bits(guarded)), (flavour, poison)


def test_a_workspace_one_byte_short_is_refused(device):
    L = _lib.lib()
    need = L.spr_upsample_unary_workspace_size()
    assert need > 0
    xc, xs = synthetic.rand((5, 64), 81).to(device), synthetic.rand((33, 32), 82).to(device)
    w, idx = synthetic.rand((64, 96), 83).to(device), _matrix(_indices("one", 33, 5), 1, device)
    y = torch.full((33, 64), 7.0, device=device)
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    n_host = ctypes.c_int(-1)

    def call(ws_bytes, n=33):
        return L.spr_upsample_unary(ops._ptr(xc), 5, 64, ops._ptr(xs), n, 32, ops._ptr(idx), 1, ops._ptr(w), 64,
                                    ops._ptr(y), None, 0, None, 0, None, 0, None, 0, ctypes.byref(n_host), ops._ptr(ws),
                                    ws_bytes, ops._stream(xc))
    assert call(need - 1) == 2 and b"workspace" in L.spr_last_error()
    torch.cuda.synchronize()
    assert float(y.min()) == float(y.max()) == 7.0           # refused before any launch
    assert call(need) == 0
    torch.cuda.synchronize()
    _check(y, _ref64(xc.cpu(), xs.cpu(), _indices("one", 33, 5), w.cpu()), 2e-6, "exact workspace")
    # shapes without a kernel are refused with a status as well
    assert L.spr_upsample_unary_supported(48, 32, 64) == 0 and L.spr_upsample_unary_supported(64, 32, 16) == 0
    for kc, ks, n_out in ((256, 128, 128), (512, 256, 256), (1024, 512, 512), (256, 128, 256), (1024, 512, 1024)):
        assert L.spr_upsample_unary_supported(kc, ks, n_out) in (0, 1)


# ---- 5. the decoder against the reference ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return load_golden("decoder_3dmatch.npz")


def _backbone(gold, device, bias=False):
    cfg = dc.with_decoder(get_config("3dmatch"), use_batch_norm=not bias)
    enc = KPFEncoder(cfg, cfg.d_embed)
    dec = KPFDecoder(cfg, enc.encoder_skip_dims[-1], enc.encoder_skip_dims)
    model = dc.Backbone(enc, dec)
    synthetic.fill_parameters(model, seed=int(gold["seed"]))
    return cfg, model.to(device)


def _small_batch(gold, device):
    """The small case's pyramid as the decoder reads it, and its inputs."""
    batch = {"points": [T(gold[f"small|points{l}"]).to(device) for l in range(3)],
             "stack_lengths": [T(gold[f"small|lens{l}"]).to(device) for l in range(3)],
             "upsamples": [T(gold[f"small|upsamples{l}"].astype(np.int64)).to(device) for l in range(2)]
             + [torch.zeros((0, 1), dtype=torch.int64, device=device)]}
    return batch, T(gold["small|enc_out"]).to(device), [T(gold[f"small|skip{l}"]).to(device) for l in range(2)]


def _restated(gold, model, bias, dtype):
    dec = model.decoder
    w = [dec.decoder_blocks[j].mlp.weight.detach().cpu().to(dtype) for j in (1, 3)]
    b = [dec.decoder_blocks[j].batch_norm.bias.detach().cpu().to(dtype) for j in (1, 3)] if bias else None
    up0 = [T(gold[f"small|upsamples{l}"][:, 0].astype(np.int64)) for l in (0, 1)]
    lens = [gold[f"small|lens{l}"] for l in range(3)]
    return dc.restated_decoder(T(gold["small|enc_out"]).to(dtype), [T(gold[f"small|skip{l}"]).to(dtype) for l in (0, 1)],
                               up0, lens, w, b)


@pytest.mark.parametrize("bias", [False, True], ids=["norm", "bias"])
@pytest.mark.parametrize("route", ["fused", "operator"])
@pytest.mark.parametrize("mode", [1, 0])
def test_decoder_on_the_references_tensors(gold, device, monkeypatch, mode, route, bias):
    """Fed the reference's encoder output, skips and upsamples: every x_all entry within 1e-5 of the tensor's scale
    (the feature gate of SURVEY section 7, as test_gpu_ops.py::test_kpconv_vs_reference), or within 4 * err32 where a
    near-constant channel makes float32 itself worse (err32: the float32 restatement against the float64 one)."""
    ops.set_gemm_mode(mode)
    cfg, model = _backbone(gold, device, bias)
    other = KPFDecoder(cfg, 512, model.encoder.encoder_skip_dims)
    other.load_state_dict(model.decoder.state_dict(), strict=True)
    assert list(other.state_dict().keys()) == gold["bias|state_dict_keys" if bias else "state_dict_keys"].tolist()
    calls = []
    real = decoder.upsample_unary_fused
    monkeypatch.setattr(decoder, "supported", lambda *a: route == "fused")
    monkeypatch.setattr(decoder, "upsample_unary_fused", lambda *a: (calls.append(1), real(*a))[1])
    batch, x, skips = _small_batch(gold, device)
    with torch.no_grad():
        out, x_all = other.to(device)(x, list(skips), batch)
    assert len(calls) == (2 if route == "fused" else 0) and out is x_all[-1] and len(x_all) == 2
    r64, r32 = _restated(gold, model, bias, F64), _restated(gold, model, bias, torch.float32)
    for j, y in enumerate(x_all):
        ref = T(gold[f"small|bias|x_all{j}" if bias else f"small|x_all{j}"]).double()
        err32 = float((r32[j].double() - r64[j]).abs().max())
        err, scale = float((y.double().cpu() - ref).abs().max()), float(ref.abs().max())
        print(f"mode {mode} {route} bias {bias} x_all[{j}]: err {err:.3e} scale {scale:.3e} err32 {err32:.3e}")
        assert y.shape == ref.shape and err <= max(1e-5 * scale, 4 * err32), (j, err, scale, err32)


def test_decoder_end_to_end_from_points(gold, device):
    """This package's Preprocessor + KPFEncoder + KPFDecoder on the big case's clouds with the golden's weights.  The
    generator guarantees a unique nearest coarse point per row, so column 0 of both upsamples matrices must equal the
    reference's; the sampled x_all rows then lie within the gate of test_gpu_regtr.py's encoder check (2e-5 of the
    tensor's maximum).  The pyramid of the architecture with a decoder is bitwise the one without."""
    cfg, model = _backbone(gold, device)
    pts = [T(c).to(device) for c in dc.clouds("big", int(gold["big|cloud_seed"]))]
    with torch.no_grad():
        meta = Preprocessor(cfg)(pts)
        plain = Preprocessor(get_config("3dmatch"))(pts)
        assert [int(p.shape[0]) for p in meta["points"]] == gold["big|rows"].tolist()
        for key in ("points", "stack_lengths", "neighbors", "pools", "upsamples"):
            assert len(meta[key]) == len(plain[key]) == 3
            for a, b in zip(meta[key], plain[key]):
                assert a.dtype == b.dtype and torch.equal(a, b), key
        for l in (0, 1):
            assert torch.equal(meta["upsamples"][l][:, 0].cpu(), T(gold[f"big|up0_{l}"]).long()), l
        feats = torch.ones((meta["points"][0].shape[0], 1), device=device)
        x, skips = model.encoder(feats, meta)
        assert len(skips) == 2 and [s.shape[1] for s in skips] == [128, 256] and x.shape[1] == 512
        out, x_all = model.decoder(x, skips, meta)
    assert not skips and out is x_all[-1]
    for j, y in enumerate(x_all):
        ref = gold[f"big|x_all{j}|rows"]
        got = y.cpu().numpy()[dc.sample_rows(y.shape[0])]
        err, scale = np.abs(got - ref).max(), float(gold[f"big|x_all{j}|max"])
        print(f"x_all[{j}] {tuple(y.shape)}: err {err:.3e} scale {scale:.3e}")
        assert got.shape == ref.shape and err <= 2e-5 * scale, (j, err, scale)


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def test_decoder_gradients(gold, device):
    """sum(y * g) backward through the module (the operator route: every piece has a HIP backward) against float64
    autograd of the restated decoder: _rel <= max(2e-5, 2 x the reference's own float32 distance from float64)."""
    cfg, model = _backbone(gold, device)
    batch, x, skips = _small_batch(gold, device)
    x, skips = x.requires_grad_(True), [s.requires_grad_(True) for s in skips]
    model.train()
    _, x_all = model.decoder(x, list(skips), batch)
    assert all(y.requires_grad for y in x_all)
    loss = sum((y * synthetic.rand(y.shape, dc.G_SEED + j).to(device)).sum() for j, y in enumerate(x_all))
    model.zero_grad(set_to_none=True)
    loss.backward()
    # float64 restatement
    dec = model.decoder
    names = ["decoder_blocks.1.mlp.weight", "decoder_blocks.3.mlp.weight"]
    w64 = [dec.decoder_blocks[j].mlp.weight.detach().cpu().double().requires_grad_(True) for j in (1, 3)]
    x64 = T(gold["small|enc_out"]).double().requires_grad_(True)
    s64 = [T(gold[f"small|skip{l}"]).double().requires_grad_(True) for l in (0, 1)]
    up0 = [T(gold[f"small|upsamples{l}"][:, 0].astype(np.int64)) for l in (0, 1)]
    ya = dc.restated_decoder(x64, s64, up0, [gold[f"small|lens{l}"] for l in range(3)], w64)
    sum((y * synthetic.rand(y.shape, dc.G_SEED + j).double()).sum() for j, y in enumerate(ya)).backward()
    cases = [("enc_out", x.grad, x64.grad, T(gold["small|grad|enc_out"]))]
    cases += [(f"skip{l}", skips[l].grad, s64[l].grad, T(gold[f"small|grad|skip{l}"])) for l in (0, 1)]
    for name, p, p64 in zip(names, (dec.decoder_blocks[1].mlp.weight, dec.decoder_blocks[3].mlp.weight), w64):
        pick = T(grad_sample_indices(name, p64.numel(), k=dc.W_SAMPLES))
        cases.append((name, p.grad.reshape(-1).cpu()[pick], p64.grad.reshape(-1)[pick], T(gold[f"small|grad|{name}|samples"])))
    for name, got, ref64, ref32 in cases:
        ours, theirs = _rel(got, ref64), _rel(ref32, ref64)
        print(f"d {name}: ours {ours:.3e} from float64, the reference {theirs:.3e}")
        assert ours <= max(2e-5, 2 * theirs), (name, ours, theirs)
