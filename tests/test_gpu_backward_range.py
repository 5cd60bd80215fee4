"""GPU: the HIP backward across operand magnitudes, shape tails and dispatch paths.

test_gpu_backward.py checks every backward operator once, at unit magnitude and one shape per operator.  Here
each operator meets the shapes, magnitudes and alignments that select its other kernels, against float64 torch
on the CPU:
  * weight-gradient products (autograd._tn_product: split-fp16 MFMA, spr_bgemm and float64 paths), spr_bgemm's
    four tile kernels, the Linear backward (split / bgemm dX, both activation and both colsum kernels);
  * the 64-bit fixed-point scatter-adds (max-pool, row gather, KPConv dX) from 1e-30 to 1e20;
  * the KPConv backward on pooling-like neighbourhoods (queries != supports, several clouds, shadow padding,
    rows without a valid neighbour, two neighbour chunks, every cin form) and on rows whose feature sum is 0
    or has an order-dependent float32 sign;
  * InstanceNorm and LayerNorm backward on ragged clouds, every LayerNorm width, unaligned storage and rows with
    a large mean and a small spread.

Products are checked per ELEMENT (test_gpu_range._check_gemm): |err_ij| <= (2^-21 + sqrt(K) 2^-24) sum_k |a_ik b_kj|
plus a max-norm bound -- a max-norm criterion alone lets cancellation hide a wrong element.
"""
import math

import pytest
import torch

from superpoints_registration_amd import _lib, autograd, ops, synthetic

pytestmark = pytest.mark.gpu
F64 = torch.float64

MAGS = [(1e-5, 1e-5), (1e-5, 1e3), (1e-3, 2e-3), (1.0, 2e-4), (3.0, 0.2), (1e3, 1e-5), (1e3, 1e3), (6e4, 1.0)]


@pytest.fixture
def gemm_mode(request):
    ops.set_gemm_mode(request.param)
    yield request.param
    ops.set_gemm_mode(1)


def _coef(k):
    # forward error bound of an fp32 dot product of length k whose operands carry 2^-22 relative error
    return 2.0 ** -21 + math.sqrt(k) * 2.0 ** -24


def _check_prod(got, ref, mag, k, what, floor=None):
    """got ~ ref (float64) with mag = the same product of absolute values.  floor: an extra absolute allowance
    per element (the fixed-point scatter-adds' quantisation), same shape as ref or a scalar."""
    got = torch.as_tensor(got).detach().cpu().to(F64)
    assert torch.isfinite(got).all(), f"{what}: non-finite gradient"
    err = (got - ref).abs()
    allow = _coef(k) * mag + (0.0 if floor is None else floor)
    ratio = err / (allow + 1e-300)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    i = int(ratio.argmax()) if ratio.numel() else 0
    assert worst <= 1.0, (f"{what}: element {i} error {float(err.flatten()[i]):.3e} exceeds its bound "
                          f"{float(allow.flatten()[i]):.3e} ({worst:.2f}x; ref {float(ref.flatten()[i]):.3e})")
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    if floor is None:
        assert float(err.max()) <= 2e-6 * max(1, k // 256) * scale, \
            f"{what}: max err {float(err.max()):.3e} vs scale {scale:.3e}"


# ---- 1. weight-gradient products --------------------------------------------------------------------------- #
def _tn(L, R, f64=False):
    rows, nl = L.shape
    nr = R.shape[1]
    return autograd._tn_product(L, R, rows, nl, nr, f64=f64)


def _tn_ref(L, R):
    L64, R64 = L.to(F64), R.to(F64)
    return L64.t() @ R64, L64.abs().t() @ R64.abs()


TN_SHAPES = [(32, 32), (36, 100), (720, 24), (1920, 128), (256, 1024)]


@pytest.mark.parametrize("rows", [1, 15, 17, 255, 257, 4100])
@pytest.mark.parametrize("nl,nr", TN_SHAPES)
@pytest.mark.parametrize("gemm_mode", [1, 0], indirect=True, ids=["split", "f32"])
def test_tn_product_shapes(device, rows, nl, nr, gemm_mode):
    """One split-K part and many (_tn_chunk), tile tails (36 x 100), the KPConv shapes (720 x 24: bgemm;
    1920 x 128: split), a 4-tile output; split-fp16 (mode 1) and exact-f32 (mode 0) arithmetic."""
    L = synthetic.rand((rows, nl), 100 + rows)
    R = synthetic.rand((rows, nr), 200 + nl)
    got = _tn(L.to(device), R.to(device)).cpu()
    ref, mag = _tn_ref(L, R)
    _check_prod(got, ref, mag, rows, f"tn {rows}x{nl}x{nr} mode {gemm_mode}")


@pytest.mark.parametrize("nl,nr", [(32, 32), (36, 100), (720, 24), (1920, 128)])
def test_tn_product_long(device, nl, nr):
    """~20 000 rows: many split-K parts and the fixed-order reduction."""
    rows = 20011
    L = synthetic.rand((rows, nl), 301)
    R = synthetic.rand((rows, nr), 302)
    got = _tn(L.to(device), R.to(device)).cpu()
    ref, mag = _tn_ref(L, R)
    _check_prod(got, ref, mag, rows, f"tn {rows}x{nl}x{nr}")


@pytest.mark.parametrize("ml,mr", MAGS + [(1e-8, 1e3), (1e-9, 1e3), (1e-6, 30.0)])
@pytest.mark.parametrize("gemm_mode", [1, 0], indirect=True, ids=["split", "f32"])
def test_tn_product_every_magnitude(device, ml, mr, gemm_mode):
    """The forward's MAGS grid, plus the training pairing: output gradients 1e-9 .. 1e-6 against activations
    up to 1e3."""
    rows, nl, nr = 3001, 256, 96
    L = synthetic.rand((rows, nl), 311) * ml
    R = synthetic.rand((rows, nr), 312) * mr
    got = _tn(L.to(device), R.to(device)).cpu()
    ref, mag = _tn_ref(L, R)
    _check_prod(got, ref, mag, rows, f"tn |L|~{ml:g} |R|~{mr:g} mode {gemm_mode}")


@pytest.mark.parametrize("gemm_mode", [1, 0], indirect=True, ids=["split", "f32"])
def test_tn_product_mixed_magnitudes_and_cancelling_columns(device, gemm_mode):
    """Rows of L spanning 1e-9 .. 1e-5, columns of R spanning 1e3 .. 1e-1, and L's columns summing to zero over
    each of three segments (the InstanceNorm backward's output per cloud): sum L_ik R_kj is then mostly
    cancellation, which only the per-element bound sees."""
    rows, nl, nr = 5000, 64, 128
    L = synthetic.rand((rows, nl), 321) * torch.logspace(-5, -9, rows).unsqueeze(1)
    for a, b in ((0, 1), (1, 3000), (3000, 5000)):
        L[a:b] -= L[a:b].mean(0, keepdim=True)
    R = synthetic.rand((rows, nr), 322, 0.0, 1.0) * torch.logspace(3, -1, nr).unsqueeze(0)
    got = _tn(L.to(device), R.to(device)).cpu()
    ref, mag = _tn_ref(L, R)
    _check_prod(got, ref, mag, rows, f"tn mixed mode {gemm_mode}")


@pytest.mark.parametrize("rows,nl,nr,ml,mr", [(20011, 15, 64, 1.0, 1e-8), (20011, 15, 128, 1e3, 1e-6),
                                              (257, 15, 32, 1.0, 1.0), (4100, 720, 24, 1e-3, 1e3)])
def test_tn_product_f64_path(device, rows, nl, nr, ml, mr):
    """spr_tn_product_f64 (the first KPConv's dW): float64 accumulation, rounded once."""
    L = synthetic.rand((rows, nl), 331, 0.0, 1.0) * ml
    R = synthetic.rand((rows, nr), 332) * mr
    got = _tn(L.to(device), R.to(device), f64=True).cpu()
    ref, mag = _tn_ref(L, R)
    # float64 sums rounded once to float32: half an ulp of the result, far inside the fp32 product bound
    _check_prod(got, ref, mag, rows, f"tn f64 {rows}x{nl}x{nr}")
    # ... and tighter: float64 sums rounded once to float32, half an ulp of each result
    err = (got.to(F64) - ref).abs()
    assert bool((err <= 2.0 ** -24 * ref.abs() + 1e-12 * mag).all()), f"tn f64 {rows}x{nl}x{nr}: not rounded once"


@pytest.mark.parametrize("gemm_mode", [1, 0], indirect=True, ids=["split", "f32"])
def test_tn_product_is_bitwise_reproducible(device, gemm_mode):
    L = (synthetic.rand((20011, 256), 341) * 1e-7).to(device)
    R = (synthetic.rand((20011, 256), 342) * 1e2).to(device)
    a = _tn(L, R).clone()
    b = _tn(L, R).clone()
    assert torch.equal(a, b)


# ---- 2. spr_bgemm ------------------------------------------------------------------------------------------ #
def _bgemm_case(device, recs, sa, sb, sc, alpha, beta, seed):
    """Flat A, B, C buffers addressed by the descriptor records; float64 reference of the same addressing."""
    def extent(off_i, m_i, s):
        return max(r[off_i] + (r[m_i[0]] - 1) * s[0] + (r[m_i[1]] - 1) * s[1] for r in recs) + 1
    na = extent(0, (3, 5), sa)
    nb = extent(1, (5, 4), sb)
    nc = extent(2, (3, 4), sc)
    A = synthetic.rand((na,), seed)
    B = synthetic.rand((nb,), seed + 1)
    C0 = synthetic.rand((nc,), seed + 2)
    C = C0.clone().to(device)
    autograd.bgemm(A.to(device), B.to(device), C, recs, sa, sb, sc, alpha, beta)
    C = C.cpu()
    ref = C0.to(F64) * beta
    mag = C0.to(F64).abs() * abs(beta)
    touched = torch.zeros(nc, dtype=torch.bool)
    kmax = 1
    for (ao, bo, co, m, n, k) in recs:
        ia = ao + torch.arange(m)[:, None] * sa[0] + torch.arange(k)[None, :] * sa[1]
        ib = bo + torch.arange(k)[:, None] * sb[0] + torch.arange(n)[None, :] * sb[1]
        ic = co + torch.arange(m)[:, None] * sc[0] + torch.arange(n)[None, :] * sc[1]
        a64, b64 = A.to(F64)[ia], B.to(F64)[ib]
        ref[ic] = alpha * (a64 @ b64) + beta * C0.to(F64)[ic]
        mag[ic] = abs(alpha) * (a64.abs() @ b64.abs()) + abs(beta) * C0.to(F64)[ic].abs()
        touched[ic] = True
        kmax = max(kmax, k)
    # elements outside every output block are left exactly as they were
    assert torch.equal(C[~touched], C0[~touched])
    return C[touched], ref[touched], mag[touched], kmax


@pytest.mark.parametrize("case", ["t64", "t128", "t64x128", "t128x32"])
def test_bgemm_every_tile_kernel(device, case):
    """One case per tile kernel (64 x 64; 128 x 128 at >= 160 tile-batches; 64 x 128 below; 128 x 32 for n <= 32),
    each with m, n and k tails, transposed or strided operands, alpha / beta != (1, 0)."""
    if case == "t64":              # small: k_bgemm_f32; A transposed (column-major), C with a row pitch
        recs = [(0, 0, 0, 100, 50, 37)]
        sa, sb, sc, alpha, beta = (1, 100), (50, 1), (61, 1), 1.0, 0.5
    elif case == "t128":           # 8 x 5 tiles x 4 batches of different sizes = 160: k_bgemm_f32_t<128, 128>
        recs = [(0, 0, 0, 1000, 520, 70), (70, 70 * 600, 1000 * 600, 999, 517, 33),
                (140, 2 * 70 * 600, 2 * 1000 * 600, 129, 97, 17), (210, 3 * 70 * 600, 3 * 1000 * 600, 1000, 600, 70)]
        sa, sb, sc, alpha, beta = (300, 1), (600, 1), (600, 1), 0.75, 0.0
    elif case == "t64x128":        # 3 x 2 tiles, one batch: k_bgemm_f32_t<64, 128>; B transposed
        recs = [(0, 0, 0, 300, 200, 33)]
        sa, sb, sc, alpha, beta = (33, 1), (1, 33), (200, 1), 1.0, -1.0
    else:                          # n <= 32: k_bgemm_f32_t<128, 32>; B with a column stride, two batches
        recs = [(0, 0, 0, 500, 20, 45), (500 * 45, 3 * 20 * 45 + 5, 500 * 31, 257, 31, 45)]
        sa, sb, sc, alpha, beta = (45, 1), (3 * 31, 3), (31, 1), 1.0, 2.0
    got, ref, mag, k = _bgemm_case(device, recs, sa, sb, sc, alpha, beta, 400)
    _check_prod(got, ref, mag, k, f"bgemm {case}")


# ---- 3. Linear backward ------------------------------------------------------------------------------------ #
_ACTS = {ops.ACT_NONE: "none", ops.ACT_RELU: "relu", ops.ACT_SIGMOID: "sigmoid"}


def _linear_grads(device, m, k, n, act, mx, mw, seed, bias=True):
    x = synthetic.rand((m, k), seed) * mx
    w = synthetic.rand((n, k), seed + 1) * mw
    b = synthetic.rand((n,), seed + 2) * mx * mw
    go = synthetic.rand((m, n), seed + 3)
    lx, lw = x.clone().to(device).requires_grad_(True), w.clone().to(device).requires_grad_(True)
    lb = b.clone().to(device).requires_grad_(True) if bias else None
    y = ops.linear(lx, lw, lb, None, act)
    y.backward(go.to(device))
    yc = y.detach().cpu().to(F64)
    # g = dout * act'(y) from the kernel's own forward output: the reference differentiates the same branch
    if act == ops.ACT_RELU:
        d = (yc > 0).to(F64)
    elif act == ops.ACT_SIGMOID:
        d = yc * (1.0 - yc)
    else:
        d = torch.ones_like(yc)
    g = go.to(F64) * d
    gm = go.to(F64).abs() * d.abs()
    return (lx.grad.cpu(), lw.grad.cpu(), None if lb is None else lb.grad.cpu()), g, gm, x.to(F64), w.to(F64)


def _check_linear(grads, g, gm, x64, w64, what):
    dx, dw, db = grads
    m, n = g.shape
    k = x64.shape[1]
    # the activation step multiplies in fp32 (<= 3 roundings): absorbed into the operand error of _coef
    _check_prod(dx, g @ w64, gm @ w64.abs(), n, f"{what} dx")
    _check_prod(dw, g.t() @ x64, gm.t() @ x64.abs(), m, f"{what} dW")
    if db is not None:
        _check_prod(db, g.sum(0), gm.sum(0), m, f"{what} db")


@pytest.mark.parametrize("m,k,n", [(777, 256, 192), (257, 64, 96), (130, 48, 50), (300, 8, 64), (131, 40, 50),
                                   (515, 32, 1024), (64, 16, 3)])
@pytest.mark.parametrize("act", list(_ACTS), ids=list(_ACTS.values()))
def test_linear_backward_shapes(device, m, k, n, act):
    """dX on the split NT product (n % 32 == 0, k >= 16) and on spr_bgemm (n = 50, 3; k = 8); m n % 4 != 0
    (131 x 50, 64 x 3: k_act_bwd); bias widths dividing 1024 (k_colsum_flat) and not (50, 96, 3: k_colsum_parts)."""
    grads, g, gm, x64, w64 = _linear_grads(device, m, k, n, act, 1.5, 0.2, 500 + m)
    _check_linear(grads, g, gm, x64, w64, f"linear {m}x{k}x{n} act {_ACTS[act]}")


@pytest.mark.parametrize("mx,mw", MAGS)
@pytest.mark.parametrize("gemm_mode", [1, 0], indirect=True, ids=["split", "f32"])
def test_linear_backward_every_magnitude(device, mx, mw, gemm_mode):
    grads, g, gm, x64, w64 = _linear_grads(device, 515, 256, 768, ops.ACT_RELU, mx, mw, 520)
    _check_linear(grads, g, gm, x64, w64, f"linear |x|~{mx:g} |w|~{mw:g} mode {gemm_mode}")


@pytest.mark.parametrize("gemm_mode", [1, 0], indirect=True, ids=["split", "f32"])
def test_linear_backward_tiny_gradients(device, gemm_mode):
    """Training-size output gradients (1e-8) through a sigmoid, activations up to 1e3."""
    m, k, n = 700, 256, 256
    x = (synthetic.rand((m, k), 531) * torch.logspace(3, -1, m).unsqueeze(1))
    w = synthetic.rand((n, k), 532) * 0.05
    go = synthetic.rand((m, n), 533) * 1e-8
    lx, lw = x.clone().to(device).requires_grad_(True), w.clone().to(device).requires_grad_(True)
    y = ops.linear(lx, lw, None, None, ops.ACT_SIGMOID)
    y.backward(go.to(device))
    yc = y.detach().cpu().to(F64)
    d = yc * (1.0 - yc)
    g, gm = go.to(F64) * d, go.to(F64).abs() * d
    _check_linear((lx.grad.cpu(), lw.grad.cpu(), None), g, gm, x.to(F64), w.to(F64), f"linear tiny g mode {gemm_mode}")


def test_act_bwd_both_kernels(device):
    """spr_act_bwd directly: n % 4 == 0 on aligned storage (k_act_bwd4) and an odd length / offset view (k_act_bwd)."""
    L = _lib.lib()
    for n, off in ((4096, 0), (4095, 0), (4096, 1)):
        y = synthetic.rand((n + 1,), 540, 0.0, 1.0).to(device)[off:off + n]
        dy = (synthetic.rand((n + 1,), 541) * 1e-20).to(device)[off:off + n]
        for act in (ops.ACT_RELU, ops.ACT_SIGMOID):
            out = torch.empty(n + 1, dtype=torch.float32, device=device)[off:off + n]
            _lib.check(L.spr_act_bwd(ops._ptr(y), ops._ptr(dy), act, n, ops._ptr(out), ops._stream(y)), "spr_act_bwd")
            yc, dc = y.cpu().to(F64), dy.cpu().to(F64)
            ref = dc * (yc > 0) if act == ops.ACT_RELU else dc * yc * (1 - yc)
            # three fp32 roundings at most (1 - y, two products)
            assert float(((out.cpu().to(F64) - ref).abs() - 3 * 2.0 ** -24 * ref.abs()).max()) <= 0, (n, off, act)


# ---- 4. fixed-point scatter-adds --------------------------------------------------------------------------- #
def _fx_floor(counts, amax):
    """The scatter-adds sum contributions in 64-bit fixed point with the largest one near 2^40: each contribution
    is rounded to 2^-40 of (a power of two below 2 amax), plus the final rounding to fp32 (in _check_prod's
    per-element term)."""
    return counts.to(F64) * 2.0 ** -40 * 2.0 * amax


FX_MAGS = [1e-30, 1e-25, 1e-20, 1e-16, 1e-14, 1e-8, 1.0, 1e8, 1e15, 1e20]


@pytest.mark.parametrize("c", [64, 30])
@pytest.mark.parametrize("mag", FX_MAGS)
def test_maxpool_backward_every_magnitude(device, c, mag):
    """c % 4 == 0 (k_maxpool_bwd4) and not (spr_maxpool_bwd directly: k_maxpool_bwd); shadow indices; support row 0 is every query's
    maximum in the even channels, so it receives one contribution per query there (3000)."""
    ns, nq, k = 900, 3000, 9
    x = synthetic.rand((ns, c), 600)
    x[0, ::2] = 10.0
    g = torch.Generator().manual_seed(601)
    idx = torch.randint(0, ns + 1, (nq, k), generator=g)       # ns = the shadow row
    idx[:, 4] = 0
    idx[5] = ns                                                 # a query with only shadow neighbours
    go = synthetic.rand((nq, c), 602) * mag
    if c % 4 == 0:
        lx = x.clone().to(device).requires_grad_(True)
        ops.maxpool(lx, idx.to(torch.int32).to(device)).backward(go.to(device))
        got = lx.grad
    else:   # the forward gather takes c % 4 == 0 only: the backward's scalar kernel directly
        L = _lib.lib()
        dxd, dgo, didx = x.to(device), go.to(device), idx.to(torch.int32).to(device)
        got = torch.empty_like(dxd)
        ws = torch.empty(L.spr_scatter_workspace_bytes(ns, c), dtype=torch.uint8, device=device)
        _lib.check(L.spr_maxpool_bwd(ops._ptr(dxd), ns, c, ops._ptr(didx), nq, k, k, ops._ptr(dgo), ops._ptr(got),
                                     ops._ptr(ws), ws.numel(), ops._stream(dxd)), "spr_maxpool_bwd")
    cx = x.to(F64).requires_grad_(True)
    ext = torch.cat([cx, torch.zeros_like(cx[:1])])
    arg = ext[idx].argmax(1)                                    # [nq, c]: first maximum (ties: shadow-only rows)
    src = torch.gather(idx, 1, arg)                             # support row of every (query, channel)
    ref = torch.zeros(ns + 1, c, dtype=F64).scatter_add_(0, src, go.to(F64))[:ns]
    mag_ = torch.zeros(ns + 1, c, dtype=F64).scatter_add_(0, src, go.to(F64).abs())[:ns]
    cnt = torch.zeros(ns + 1, c, dtype=F64).scatter_add_(0, src, torch.ones(nq, c, dtype=F64))[:ns]
    assert float(cnt[0, ::2].min()) >= nq - 1
    _check_prod(got, ref, mag_, 1, f"maxpool c={c} |dy|~{mag:g}", floor=_fx_floor(cnt, float(go.abs().max())))


@pytest.mark.parametrize("mag", FX_MAGS)
def test_gather_rows_backward_every_magnitude(device, mag):
    """One source row receives 4000 contributions; indices equal to n_src (out of range) contribute nothing."""
    n_src, c = 500, 48
    g = torch.Generator().manual_seed(610)
    sel = torch.randint(0, n_src, (6000,), generator=g)
    sel[::3] = 7
    sel[1::500] = n_src
    go = synthetic.rand((6000, c), 611) * mag
    lx = torch.zeros((n_src, c), device=device, requires_grad=True)
    ops.gather_rows(lx, sel.to(torch.int32).to(device)).backward(go.to(device))
    keep = sel < n_src
    ref = torch.zeros(n_src, c, dtype=F64).index_add_(0, sel[keep], go.to(F64)[keep])
    mag_ = torch.zeros(n_src, c, dtype=F64).index_add_(0, sel[keep], go.to(F64)[keep].abs())
    cnt = torch.zeros(n_src, dtype=F64).index_add_(0, sel[keep], torch.ones(int(keep.sum()), dtype=F64))
    _check_prod(lx.grad, ref, mag_, 1, f"gather |dy|~{mag:g}", floor=_fx_floor(cnt[:, None], float(go.abs().max())))


def test_scatter_adds_mixed_magnitudes(device):
    """Rows of the incoming gradient spanning 1e-20 .. 1e4 in one tensor: the largest sets the fixed-point scale,
    the small rows keep 2^-40 of it as their absolute resolution (the floor below), nothing worse."""
    n_src, c = 300, 32
    g = torch.Generator().manual_seed(620)
    sel = torch.randint(0, n_src, (4000,), generator=g)
    go = synthetic.rand((4000, c), 621) * torch.logspace(4, -20, 4000).unsqueeze(1)
    lx = torch.zeros((n_src, c), device=device, requires_grad=True)
    ops.gather_rows(lx, sel.to(torch.int32).to(device)).backward(go.to(device))
    ref = torch.zeros(n_src, c, dtype=F64).index_add_(0, sel, go.to(F64))
    mag_ = torch.zeros(n_src, c, dtype=F64).index_add_(0, sel, go.to(F64).abs())
    cnt = torch.zeros(n_src, dtype=F64).index_add_(0, sel, torch.ones(4000, dtype=F64))
    _check_prod(lx.grad, ref, mag_, 1, "gather mixed", floor=_fx_floor(cnt[:, None], float(go.abs().max())))


# ---- 5. KPConv backward ------------------------------------------------------------------------------------ #
def _kp_cloud(seed, kmax=80):
    """Two clouds of supports (500 + 300 points in 0.3-boxes), 260 queries drawn apart from the supports (a pooling
    layer: nq < ns), neighbours within 0.11 of the query in its own cloud, nearest first, at most kmax, padded with
    the shadow index ns; four queries far from everything have no valid neighbour."""
    g = torch.Generator().manual_seed(seed)
    s = torch.cat([torch.rand((500, 3), generator=g) * 0.3, torch.rand((300, 3), generator=g) * 0.3 + 5.0])
    q = torch.cat([torch.rand((170, 3), generator=g) * 0.3, torch.rand((86, 3), generator=g) * 0.3 + 5.0,
                   torch.full((4, 3), -50.0)])
    scloud = torch.cat([torch.zeros(500), torch.ones(300)])
    qcloud = torch.cat([torch.zeros(170), torch.ones(86), torch.full((4,), 2.0)])
    d = torch.cdist(q.double(), s.double())
    d[qcloud[:, None] != scloud[None, :]] = float("inf")
    d[d > 0.11] = float("inf")
    dist, order = d.sort(1)
    nb = order[:, :kmax].clone()
    nb[~torch.isfinite(dist[:, :kmax])] = s.shape[0]
    kp = torch.cat([torch.zeros(1, 3), torch.randn((14, 3), generator=g) * 0.03])
    return q, s, nb, kp, 0.05


def _kp_unnorm(q, s, nb, x, w, kp, ext):
    """kpconv_blocks.py:309-406 in float64: the sum over kernel points BEFORE the division by the count."""
    s_ext = torch.cat((s, torch.full_like(s[:1], 1e6)), 0)
    diff = (s_ext[nb] - q.unsqueeze(1)).unsqueeze(2) - kp
    infl = torch.clamp(1 - torch.sqrt((diff ** 2).sum(3)) / ext, min=0.0).transpose(1, 2)
    nx = torch.cat((x, torch.zeros_like(x[:1])), 0)[nb]
    return torch.matmul(torch.matmul(infl, nx).permute(1, 0, 2), w).sum(0)


def _kp_check(device, q, s, nb, kp, ext, x, w, go, what):
    lx, lw = x.clone().to(device).requires_grad_(True), w.clone().to(device).requires_grad_(True)
    y = ops.kpconv(q.to(device), s.to(device), nb.to(torch.int32).to(device), lx, lw, kp.to(device), ext,
                   rows_sorted=True)
    y.backward(go.to(device))
    q64, s64, kp64 = q.to(F64), s.to(F64), kp.to(F64)
    # the count the forward divided by, read off its output: y = U / count with U the float64 un-normalised sum
    with torch.no_grad():
        U = _kp_unnorm(q64, s64, nb, x.to(F64), w.to(F64), kp64, ext)
        yc = y.detach().cpu().to(F64)
        den = (yc * yc).sum(1)
        cnt = torch.where(den > 0, ((U * yc).sum(1) / den.clamp_min(1e-300)).round(), torch.ones_like(den))
        assert float(cnt.min()) >= 1 and float(cnt.max()) <= nb.shape[1], what
    # the gradients of U / count for that count: dW is a product (per-element bound over the contraction
    # nq x kmax); dx is a fixed-point scatter-add of products (per-element bound + the 2^-40 quantisation floor)
    gsc = go.to(F64) / cnt[:, None]
    cx, cw = x.to(F64).requires_grad_(True), w.to(F64).requires_grad_(True)
    (_kp_unnorm(q64, s64, nb, cx, cw, kp64, ext) * gsc).sum().backward()
    ax, aw = x.to(F64).abs().requires_grad_(True), w.to(F64).abs().requires_grad_(True)
    (_kp_unnorm(q64, s64, nb, ax, aw, kp64, ext) * gsc.abs()).sum().backward()
    n_kp, cin, cout = w.shape
    kk = nb.shape[1]
    _check_prod(lw.grad, cw.grad, aw.grad, q.shape[0] * kk, f"{what} dW")
    # contributions per support row: its appearances in nb, each a sum of n_kp * cout products bounded by the
    # n_kp max|dwf| the fixed-point scale is derived from
    app = torch.zeros(s.shape[0] + 1, dtype=F64).index_add_(0, nb.flatten(), torch.ones(nb.numel(), dtype=F64))[:-1]
    dwf_max = float((gsc.abs() @ w.to(F64).abs().reshape(n_kp * cin, cout).t()).max())
    floor = _fx_floor(app[:, None], n_kp * dwf_max)
    _check_prod(lx.grad, cx.grad, ax.grad, n_kp * cout, f"{what} dx", floor=floor)
    return cnt


@pytest.mark.parametrize("cin,cout", [(1, 64), (32, 64), (64, 128), (128, 64), (48, 64), (48, 40)])
@pytest.mark.parametrize("mx,mg,mode", [(1.0, 1.0, 1), (1e-3, 1e-20, 0), (1e3, 1e-8, 1), (1e-5, 1e15, 1)])
def test_kpconv_backward_pooling_neighbourhoods(device, cin, cout, mx, mg, mode):
    """Queries != supports (nq < ns), two clouds, shadow padding, rows without a neighbour, kmax = 80 (two
    neighbour chunks); cin = 1 (own forward kernel, float64 dW), 32 (half-wave form), 64, 128, 48 (general);
    cout = 40 takes the bgemm d wf.  Features non-negative so that the count is the same at every scale.
    |dout| ~ 1e-20 runs the exact-f32 products (mode 0): the split-fp16 planes scale by at most 2^60
    (pow2_exp_for), so a 1e-21 operand is outside their window (dW measured at 4x the per-element bound);
    the fixed-point dX, whose scale is not clamped, is what that case checks."""
    ops.set_gemm_mode(mode)
    q, s, nb, kp, ext = _kp_cloud(700)
    assert int((nb < s.shape[0]).sum(1).max()) > 64 and int((nb == s.shape[0]).any(1).sum()) > 10
    x = synthetic.rand((s.shape[0], cin), 701, 0.0, 1.0) * mx
    x[::7] = 0.0                                   # rows that do not count
    w = synthetic.rand((15, cin, cout), 702) * 0.1
    go = synthetic.rand((q.shape[0], cout), 703) * mg
    try:
        _kp_check(device, q, s, nb, kp, ext, x, w, go, f"kpconv cin={cin} cout={cout} |x|~{mx:g} |dout|~{mg:g}")
    finally:
        ops.set_gemm_mode(1)


@pytest.mark.parametrize("cin", [32, 64, 48, 128])
def test_kpconv_backward_counts_like_the_forward(device, cin):
    """Support rows whose float32 feature sum is exactly 0 or has an order-dependent sign ({1, -1, +-2^-30}: the
    float64 sum is +-2^-30; a float32 sum gives 0 or +-2^-30 depending on where the small term meets the pair).
    The backward must divide by the count the forward used."""
    q, s, nb, kp, ext = _kp_cloud(710, kmax=70)
    ns = s.shape[0]
    g = torch.Generator().manual_seed(711)
    x = synthetic.rand((ns, cin), 712)
    for r in range(ns):
        kind = r % 4
        if kind == 3:
            continue
        x[r] = 0.0
        if kind == 0:
            continue                               # all zeros: sum exactly 0
        i, j, l = torch.randperm(cin, generator=g)[:3].tolist()
        x[r, i], x[r, j] = 1.0, -1.0
        x[r, l] = 2.0 ** -30 if kind == 1 else -(2.0 ** -30)
    w = synthetic.rand((15, cin, 64), 713) * 0.1
    go = synthetic.rand((q.shape[0], 64), 714)
    _kp_check(device, q, s, nb, kp, ext, x, w, go, f"kpconv count cin={cin}")


@pytest.mark.parametrize("mag", [1e-30, 1e-16, 1.0, 1e18])
def test_kpconv_dx_published_range_gives_the_same_bits(device, mag):
    """spr_kpconv_bwd_dx with the range published by the d wf product equals the measured-range form bit for bit."""
    q, s, nb, kp, ext = _kp_cloud(720)
    ns, nq, cin = s.shape[0], q.shape[0], 32
    dwf = (synthetic.rand((nq, 15 * cin), 721) * mag).to(device)
    dq, ds, dkp = q.to(device), s.to(device), kp.to(device)
    nbd = nb.to(torch.int32).to(device).contiguous()
    ops.ensure_range(dwf)
    r, rn = ops._get_range(dwf)
    assert r is not None
    L = _lib.lib()
    outs = []
    for rr, n in ((r, rn), (None, 0)):
        dx = torch.empty((ns, cin), dtype=torch.float32, device=device)
        ws = torch.empty(L.spr_scatter_workspace_bytes(ns, cin), dtype=torch.uint8, device=device)
        _lib.check(L.spr_kpconv_bwd_dx(ops._ptr(dq), nq, ops._ptr(ds), ns, ops._ptr(nbd), nbd.shape[1], nbd.shape[1],
                                       cin, ops._ptr(dkp), 15, ext, ops._ptr(dwf), ops._ptr(rr), n, ops._ptr(dx),
                                       ops._ptr(ws), ws.numel(), ops._stream(dwf)), "spr_kpconv_bwd_dx")
        outs.append(dx.cpu())
    assert torch.equal(outs[0], outs[1])
    assert float(outs[0].abs().max()) > 0


# ---- 6. InstanceNorm and LayerNorm backward --------------------------------------------------------------- #
def _rel_err(got, ref):
    got = got.detach().cpu().to(F64)
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


@pytest.mark.parametrize("center,spread", [(0.0, 1.0), (1e3, 1e-2), (0.0, 1e-4)])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
def test_instnorm_backward_ragged(device, center, spread, offset):
    """Clouds of 1, 700 and 1300 points (1300 > 512: in_nsplit = 3 slices), c = 256 from storage offset by one
    float (offset1) or aligned; mean 1e3 with spread 1e-2."""
    lens = [1, 700, 1300]
    n, c = sum(lens), 256
    base = torch.zeros(n * c + offset)
    base[offset:] = (center + spread * synthetic.rand((n, c), 800)).flatten()
    add, go = synthetic.rand((n, c), 801), synthetic.rand((n, c), 802)
    cu = ops.lengths_to_cu(lens, device)
    dbase = base.to(device)
    lx = dbase[offset:].view(n, c).detach().clone() if offset == 0 else None
    leaf = torch.zeros(n * c + offset, device=device, requires_grad=True) if offset else None
    if offset:
        with torch.no_grad():
            leaf.copy_(dbase)
        xin = leaf[offset:].view(n, c)
    else:
        lx.requires_grad_(True)
        xin = lx
    la = add.clone().to(device).requires_grad_(True)
    y = ops.instnorm(xin, cu, add=la, slope=0.1, max_len=max(lens))
    y.backward(go.to(device))
    pos = y.detach().cpu() > 0          # the LeakyReLU branch the forward took (the reference takes the same)
    gx = leaf.grad[offset:].view(n, c) if offset else lx.grad
    cx = base[offset:].view(n, c).to(F64).requires_grad_(True)
    ca = add.to(F64).requires_grad_(True)
    out = []
    o = 0
    for ln in lens:
        seg = cx[o:o + ln]
        out.append((seg - seg.mean(0)) / torch.sqrt(seg.var(0, unbiased=False) + 1e-5))
        o += ln
    z = torch.cat(out) + ca
    (z * torch.where(pos, 1.0, 0.1).to(F64)).backward(go.to(F64))
    # per cloud and channel dx = rstd (g - m1 - xhat m2), m1 = mean g, m2 = mean(g xhat): float64 partial sums,
    # 2e-5 of the cloud's largest gradient (test_gpu_backward's criterion) -- plus the one error the backward
    # shares with the forward: the per-channel mean is kept in float32 (2^-24 |mean| off), which shifts xhat by
    # delta rstd and dx by rstd^2 delta (m2 + xhat m1).  At mean 1e3, spread 1e-2 that term is ~1e-4 of dx.
    g64 = go.to(F64) * torch.where(pos, 1.0, 0.1).to(F64)
    o = 0
    for ln in lens:
        seg, gs = base[offset:].view(n, c)[o:o + ln].to(F64), g64[o:o + ln]
        mu = seg.mean(0)
        rs = 1.0 / torch.sqrt(seg.var(0, unbiased=False) + 1e-5)
        xh = (seg - mu) * rs
        m1, m2 = gs.mean(0), (gs * xh).mean(0)
        shared = 2 * rs * rs * 2.0 ** -24 * mu.abs() * (m2.abs() + xh.abs() * m1.abs())
        err = (gx[o:o + ln].detach().cpu().to(F64) - cx.grad[o:o + ln]).abs()
        allow = 2e-5 * float(cx.grad[o:o + ln].abs().max()) + shared
        worst = float((err / (allow + 1e-300)).max())
        assert worst <= 1.0, f"instnorm dx cloud of {ln} (center {center:g}, spread {spread:g}, offset {offset}): {worst:.2f}x"
        o += ln
    assert _rel_err(la.grad, ca.grad) <= 1e-6


@pytest.mark.parametrize("c", [64, 192, 256, 512, 1024])
@pytest.mark.parametrize("center,spread", [(0.0, 3.0), (1e3, 1e-2)])
def test_layernorm_backward_widths(device, c, center, spread):
    """Every LayerNorm width form: k_layernorm_bwd<4> (64, 192), k_layernorm_bwd256, k_layernorm_bwd<16>
    (512, 1024); rows with mean 1e3 and spread 1e-2."""
    m = 333
    x = center + spread * synthetic.rand((m, c), 810 + c)
    gam, bet = synthetic.rand((c,), 811, 0.5, 1.5), synthetic.rand((c,), 812)
    g1, g2, p = synthetic.rand((m, c), 813), synthetic.rand((m, c), 814), synthetic.rand((m, c), 815)
    lx, lg, lb = (t.clone().to(device).requires_grad_(True) for t in (x, gam, bet))
    n_, npos = ops.layernorm(lx, lg, lb, 1e-5, pos=p.to(device))
    ((n_ * g1.to(device)).sum() + (npos * g2.to(device)).sum()).backward()
    cx, cg, cb = (t.to(F64).requires_grad_(True) for t in (x, gam, bet))
    y = torch.nn.functional.layer_norm(cx, (c,), cg, cb, 1e-5)
    ((y * g1.to(F64)).sum() + ((y + p.to(F64)) * g2.to(F64)).sum()).backward()
    # dx per row: 2e-5 of the largest dx (test_gpu_backward's criterion); dgamma / dbeta are column sums
    for a, r, nm in ((lx, cx, "dx"), (lg, cg, "dgamma"), (lb, cb, "dbeta")):
        e = _rel_err(a.grad, r.grad)
        assert e <= 2e-5, f"layernorm c={c} center {center:g} spread {spread:g} {nm}: {e:.2e}"


def test_layernorm_backward_unaligned_storage(device):
    """c = 256 with x one float off 16-byte alignment: the generic kernel instead of k_layernorm_bwd256."""
    m, c = 257, 256
    base = synthetic.rand((m * c + 1,), 820, -3.0, 5.0)
    gam, bet = synthetic.rand((c,), 821, 0.5, 1.5), synthetic.rand((c,), 822)
    g1 = synthetic.rand((m, c), 823)
    leaf = base.clone().to(device).requires_grad_(True)
    lg, lb = gam.clone().to(device).requires_grad_(True), bet.clone().to(device).requires_grad_(True)
    n_, _ = ops.layernorm(leaf[1:].view(m, c), lg, lb, 1e-5)
    (n_ * g1.to(device)).sum().backward()
    cx = base[1:].view(m, c).to(F64).requires_grad_(True)
    cg, cb = gam.to(F64).requires_grad_(True), bet.to(F64).requires_grad_(True)
    (torch.nn.functional.layer_norm(cx, (c,), cg, cb, 1e-5) * g1.to(F64)).sum().backward()
    assert float(leaf.grad[0]) == 0.0
    for a, r, nm in ((leaf.grad[1:].view(m, c), cx.grad, "dx"), (lg.grad, cg.grad, "dgamma"), (lb.grad, cb.grad, "dbeta")):
        e = _rel_err(a, r)
        assert e <= 2e-5, f"layernorm unaligned {nm}: {e:.2e}"


def test_kpconv_weighted_features_counts_off_zero_sums(device):
    """spr_kpconv_weighted_features (counting from the forward's flags) gives the neighbour count computed from x on
    the host wherever no row sum is near 0."""
    q, s, nb, kp, ext = _kp_cloud(730)
    ns, nq, cin = s.shape[0], q.shape[0], 64
    x = synthetic.rand((ns, cin), 731)
    x += torch.where(x.sum(1, keepdim=True) > 0, 0.05, -0.05)     # every row sum at least 3 away from 0
    dq, ds, dx, dkp = q.to(device), s.to(device), x.to(device), kp.to(device)
    nbd = nb.to(torch.int32).to(device).contiguous()
    L = _lib.lib()
    wf = torch.empty((nq, 15 * cin), dtype=torch.float32, device=device)
    cnt = torch.empty((nq,), dtype=torch.float32, device=device)
    ws = torch.empty(L.spr_kpconv_weighted_features_workspace_bytes(ns), dtype=torch.uint8, device=device)
    _lib.check(L.spr_kpconv_weighted_features(ops._ptr(dq), nq, ops._ptr(ds), ns, ops._ptr(nbd), nbd.shape[1],
                                              nbd.shape[1], ops._ptr(dx), cin, ops._ptr(dkp), 15, ext, ops._ptr(wf),
                                              ops._ptr(cnt), ops._ptr(ws), ws.numel(), ops._stream(dx)),
               "spr_kpconv_weighted_features")
    ref = (torch.cat([x, torch.zeros(1, cin)])[nb].sum(-1) > 0).sum(1).clamp_min(1).float()
    assert torch.equal(cnt.cpu(), ref)
