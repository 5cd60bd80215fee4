"""GPU: the non-GEMM forward operators of the KPConv encoder and the transformer input -- InstanceNorm (+ add +
LeakyReLU), LayerNorm (+ pos), max-pool / gather_rows, the sine position embedding, KPConv's geometry on every
forward route, and the operand ranges the producers publish -- against float64 restatements (tests/forward_cases.py)
over ragged shapes, operand magnitudes and the kernels' unroll / tile edges.

Bounds (the project's): 2e-6 of the output scale for the norms and the embedding, 1e-5 for KPConv features, 2e-6
between KPConv routes, equality for selections, statistics bits and published maxima.  Where float32 itself cannot
hold the fixed bound (centre 1e3 / spread 1e-2, near-constant clouds, embedding arguments of hundreds) the rule of
tests/test_gpu_range.py applies: err <= max(bound * scale, 4 * err32), err32 = the error of the reference's own
float32 arithmetic on torch-CPU against the same float64 reference.  Observed worst err / max(...) ratios are
written next to each check."""
import numpy as np
import pytest
import torch

import forward_cases as fc
from superpoints_registration_amd import get_config, ops, synthetic

pytestmark = pytest.mark.gpu
T = torch.from_numpy
F64 = torch.float64


def _bounded(got, ref64, base32, bound, what):
    """err <= max(bound * scale, 4 * err32); returns err / that limit."""
    ref64 = torch.as_tensor(ref64, dtype=F64)
    got = torch.as_tensor(got).detach().cpu().to(F64)
    assert torch.isfinite(got).all(), what
    scale = float(ref64.abs().max())
    err = float((got - ref64).abs().max())
    err32 = float((torch.as_tensor(base32).to(F64) - ref64).abs().max()) if base32 is not None else 0.0
    lim = max(bound * scale, 4 * err32)
    print(f"{what}: err {err:.3e} scale {scale:.3e} err32 {err32:.3e} ratio {err / max(lim, 1e-300):.3f}")
    assert scale > 0 and err <= lim, f"{what}: {err:.3e} > max({bound:g} * {scale:.3e}, 4 * {err32:.3e})"
    return err / lim


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- 1. InstanceNorm (+ add + LeakyReLU) ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", fc.IN_WIDTHS)
@pytest.mark.parametrize("centre,spread", fc.IN_REGIMES)
def test_instnorm_ragged_every_regime(device, c, centre, spread):
    """Ragged batch (1, 2, 3, 255, 256, 257, 1300, 77 rows) in every data regime and channel-block class, with
    add + LeakyReLU(0.1).  Observed worst err / limit per regime (centre, spread): (0, 1) 0.30, (1e3, 1e-2) 0.22,
    (0, 1e-4) 0.07, (0, 1e-20) 0.07, (0, 1e15) 0.33 -- clouds of 2 and 3 points are near-constant in some channel at
    every regime, so the err32 term decides throughout."""
    L = fc.IN_LENGTHS
    x = fc.in_data(L, c, centre, spread, 1)
    add = fc.in_add(x.shape[0], c, 2) * float(spread if centre == 0 else 1.0)
    cu = ops.lengths_to_cu(L, device)
    for a, slope in ((None, 0.1), (add, 0.1), (add, 1.0)):
        y = ops.instnorm(x.to(device), cu, add=None if a is None else a.to(device), slope=slope, max_len=max(L))
        _bounded(y, fc.instnorm_f64(x, L, add=a, slope=slope), fc.instnorm_f32(x, L, add=a, slope=slope), 2e-6,
                 f"instnorm c={c} ({centre:g},{spread:g}) add={a is not None} slope={slope}")


@pytest.mark.parametrize("c", [4, 68, 256])
def test_instnorm_constant_and_one_point_clouds(device, c):
    """Variance exactly 0: eps alone decides, the output is (x - mean) / sqrt(eps) = 0 up to the rounding of the mean
    (|x| 2^-24 / sqrt(eps) ~ 6e-5 |x|; float32 cannot do better, hence the err32 rule).  With add, the add survives."""
    L = [1, 7, 600, 1]
    x = fc.in_constant(L, c, 3)
    add = fc.in_add(x.shape[0], c, 4)
    cu = ops.lengths_to_cu(L, device)
    y = ops.instnorm(x.to(device), cu, add=add.to(device), slope=0.1)
    _bounded(y, fc.instnorm_f64(x, L, add=add, slope=0.1), fc.instnorm_f32(x, L, add=add, slope=0.1), 2e-6,
             f"instnorm constant c={c}")                      # observed ratio 0.00: x - mean is exactly 0
    one = ops.instnorm(x[:1].to(device), ops.lengths_to_cu([1], device))
    assert torch.equal(one.cpu(), torch.zeros(1, c))          # a one-point cloud: x - mean is exactly 0


@pytest.mark.parametrize("c", [4, 64, 192])
def test_instnorm_variants_bitwise(device, c):
    """norm=False, out=, and max_len exact / loose / omitted (bitwise equal); a cloud's rows are bitwise the same
    alone and inside the ragged batch (the kernel header's batch invariance); instnorm_stats returns the bits the
    apply pass used."""
    L = fc.IN_LENGTHS
    x = fc.in_data(L, c, 0.5, 2.0, 5)
    add = fc.in_add(x.shape[0], c, 6)
    cu = ops.lengths_to_cu(L, device)
    xd, ad = x.to(device), add.to(device)
    y = ops.instnorm(xd, cu, slope=0.1, max_len=max(L))
    for ml in (None, max(L) + 1, x.shape[0], 10 ** 9):
        assert torch.equal(_bits(y), _bits(ops.instnorm(xd, cu, slope=0.1, max_len=ml))), f"max_len={ml}"
    buf = torch.full_like(xd, float("nan"))
    assert ops.instnorm(xd, cu, slope=0.1, out=buf) is buf and torch.equal(_bits(buf), _bits(y))
    # norm=False: add + LeakyReLU only, exact in float32
    z = ops.instnorm(xd, cu, norm=False, add=ad, slope=0.1)
    s = x + add
    assert torch.equal(z.cpu(), torch.where(s >= 0, s, s * np.float32(0.1)))
    assert torch.equal(ops.instnorm(xd, cu, norm=False, slope=1.0).cpu(), x)
    # batch invariance
    off = 0
    for l in L:
        alone = ops.instnorm(xd[off:off + l].clone(), ops.lengths_to_cu([l], device), slope=0.1)
        assert torch.equal(_bits(alone), _bits(y[off:off + l])), f"cloud of {l} rows differs inside the batch"
        off += l
    # statistics bits: (x - mean) * rstd in float32 on the host reproduces the slope-1 output
    mean, rstd = ops.instnorm_stats(xd, cu, max_len=max(L))
    seg = torch.repeat_interleave(torch.arange(len(L)), torch.as_tensor(L))
    host = (x - mean.cpu()[seg]) * rstd.cpu()[seg]
    assert torch.equal(_bits(ops.instnorm(xd, cu, slope=1.0)), _bits(host))
    m64, r64 = fc.instnorm_stats_f64(x, L)
    assert float((mean.cpu().double() - m64).abs().max()) <= 2.0 ** -23 * float(m64.abs().max())
    assert float(((rstd.cpu().double() - r64) / r64).abs().max()) <= 2e-6


def test_instnorm_zero_length_clouds(device):
    """spr_instnorm accepts clouds without rows (k_in_final's len > 0 branch): the other clouds are unaffected, the
    empty clouds' statistics are mean 0, rstd 1 / sqrt(eps)."""
    L = fc.IN_LENGTHS_EMPTY
    x = fc.in_data(L, 64, 0.0, 1.0, 7)
    cu = ops.lengths_to_cu(L, device)
    y = ops.instnorm(x.to(device), cu, slope=0.1)
    _bounded(y, fc.instnorm_f64(x, L, slope=0.1), fc.instnorm_f32(x, L, slope=0.1), 2e-6, "instnorm with empty clouds")  # 0.03
    dense = [l for l in L if l > 0]
    assert torch.equal(_bits(y), _bits(ops.instnorm(x.to(device), ops.lengths_to_cu(dense, device), slope=0.1)))
    mean, rstd = ops.instnorm_stats(x.to(device), cu)
    for i, l in enumerate(L):
        if l == 0:
            assert float(mean[i].abs().max()) == 0.0
            assert torch.equal(rstd[i].cpu(), torch.full((64,), float(np.float32(1.0 / np.sqrt(np.float64(np.float32(1e-5)))))))
    with pytest.raises(RuntimeError, match="c %"):
        ops.instnorm(x[:, :6].contiguous().to(device), cu)


# ---- 2. LayerNorm (+ pos) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", fc.LN_WIDTHS)
@pytest.mark.parametrize("m", fc.LN_ROWS)
@pytest.mark.parametrize("centre,spread", fc.LN_REGIMES)
def test_layernorm_rows_widths_regimes(device, m, c, centre, spread):
    """Observed worst err / limit: 0.09 at (0, 3), 0.24 at (1e3, 1e-2) (a single row of 1024; before the mean of the
    residuals was added to the kernels' float32 mean: 1.07 at 1 x 256 and 1.27 at 1 x 512)."""
    x, g, b, pos = fc.ln_data(m, c, centre, spread, 11)
    ref, b32 = fc.layernorm_f64(x, g, b), fc.layernorm_f32(x, g, b)
    xd, gd, bd, pd = (t.to(device) for t in (x, g, b, pos))
    n, npos = ops.layernorm(xd, gd, bd, 1e-5, pos=pd)
    _bounded(n, ref, b32, 2e-6, f"layernorm {m}x{c} ({centre:g},{spread:g})")
    assert torch.equal(_bits(npos), _bits(n + pd)), "norm + pos is not the separate sum"
    n2, none = ops.layernorm(xd, gd, bd, 1e-5)
    assert none is None and torch.equal(_bits(n2), _bits(n))
    none, p2 = ops.layernorm(xd, gd, bd, 1e-5, pos=pd, want_norm=False)
    assert none is None and torch.equal(_bits(p2), _bits(npos))


@pytest.mark.parametrize("c", [64, 256, 512])
def test_layernorm_unaligned_storage(device, c):
    """x, pos one float off 16-byte alignment (a row-offset view of a flat buffer)."""
    m = 257
    x, g, b, pos = fc.ln_data(m, c, 0.0, 3.0, 12)
    flat = torch.cat([torch.zeros(1), x.reshape(-1)]).to(device)
    pflat = torch.cat([torch.zeros(1), pos.reshape(-1)]).to(device)
    n, npos = ops.layernorm(flat[1:].view(m, c), g.to(device), b.to(device), 1e-5, pos=pflat[1:].view(m, c))
    n0, np0 = ops.layernorm(x.to(device), g.to(device), b.to(device), 1e-5, pos=pos.to(device))
    _bounded(n, fc.layernorm_f64(x, g, b), fc.layernorm_f32(x, g, b), 2e-6, f"layernorm unaligned c={c}")   # 0.08
    assert torch.equal(_bits(n), _bits(n0)) and torch.equal(_bits(npos), _bits(np0))


# ---- 3. max-pool and gather_rows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", fc.MP_WIDTHS)
@pytest.mark.parametrize("k", fc.MP_K)
def test_maxpool_selection(device, k, c):
    """Equality with numpy for every k (the 4-unrolled loop and its tail) and width; edge rows: all shadow -> 0,
    negative features + one shadow column -> 0 (the zero shadow row), negative features without shadow -> their max."""
    ns, nq = 97, 203                                    # nq not divisible by 8
    x, idx, rows = fc.mp_case(ns, nq, k, c, 21)
    ref = fc.maxpool_np(x, idx)
    xd = T(x).to(device)
    y = ops.maxpool(xd, T(idx.astype(np.int32)).to(device)).cpu().numpy()
    assert np.array_equal(y.view(np.int32), ref.view(np.int32))
    assert np.all(y[rows["all_shadow"]] == 0.0)
    if k > 1:
        assert np.all(y[rows["neg_one_shadow"]] == 0.0)
    assert np.all(y[rows["neg_no_shadow"]] < 0.0)
    # int64 indices; a strided column slice; a walk order
    assert np.array_equal(ops.maxpool(xd, T(idx).to(device)).cpu().numpy(), ref)
    wide = np.full((nq, k + 5), ns, np.int32)
    wide[:, :k] = idx
    assert np.array_equal(ops.maxpool(xd, T(wide).to(device)[:, :k]).cpu().numpy(), ref)
    order = T(np.random.default_rng(k).permutation(nq).astype(np.int32)).to(device)
    assert np.array_equal(ops.maxpool(xd, T(idx.astype(np.int32)).to(device), order=order).cpu().numpy(), ref)


@pytest.mark.parametrize("k", [1, 3, 4, 9])
def test_maxpool_float32_range_ends(device, k):
    """Rows whose true maximum is -FLT_MAX, below -3.0e38 or -inf must come out as that value, not as a finite
    initial value of the running maximum; +FLT_MAX / +inf likewise; with a shadow column the zero row competes."""
    x, idx = fc.mp_extreme(k, 8, 22)
    ref = fc.maxpool_np(x, idx)
    y = ops.maxpool(T(x).to(device), T(idx.astype(np.int32)).to(device)).cpu().numpy()
    assert np.array_equal(y.view(np.int32), ref.view(np.int32)), (y[:6, :2], ref[:6, :2])


def test_maxpool_refuses_bad_widths_and_gather_rows(device):
    x = synthetic.rand((50, 6), 23).to(device)
    idx = torch.zeros((4, 3), dtype=torch.int32, device=device)
    with pytest.raises(RuntimeError, match="maxpool"):
        ops.maxpool(x, idx)                              # c % 4 != 0
    with pytest.raises(ValueError, match="order"):
        ops.maxpool(x[:, :4].contiguous(), idx, order=torch.zeros(3, dtype=torch.int32, device=device))
    for c in (1, 6, 7, 64, 257):                         # gather_rows takes any width
        xs = synthetic.rand((50, c), 24 + c)
        ix = np.array([0, 49, 50, -1, 7, 7, 1000, -50, 3], np.int32)      # shadow (>= n) and negative -> zero rows
        got = ops.gather_rows(xs.to(device), T(ix).to(device)).cpu().numpy()
        assert np.array_equal(got, fc.gather_np(xs.numpy(), ix))
        assert np.all(got[[2, 3, 6, 7]] == 0.0)


# ---- 4. sine position embedding ------------------------------------------------------------------------------------
# the three configs all leave pos_emb_scaling at its default 1.0; 0.25 and 2.0 exercise the kernel's scale argument
PE_SCALES = sorted({float(get_config(n).get("pos_emb_scaling", 1.0)) for n in ("3dmatch", "modelnet", "kitti")}
                   | set(fc.PE_EXTRA_SCALES))


@pytest.mark.parametrize("d_model", fc.PE_DMODEL)
@pytest.mark.parametrize("n", fc.PE_ROWS)
@pytest.mark.parametrize("mag", fc.PE_MAGS)
def test_posemb_magnitudes(device, mag, n, d_model):
    """Arguments x * 2 pi scale reach several thousand at |x| = 1e3, where one ulp of the argument is 4.9e-4: the
    err32 rule, not the 2e-6 of the O(10) golden test.  Observed worst err / limit: 0.02 at |x| = 1e-3, 0.25 at
    1 ... 100, 0.34 at 1e3."""
    xyz = fc.pe_xyz(n, mag, 31)
    npf = d_model // 3 // 2 * 2
    for scale in PE_SCALES:
        y = ops.posemb_sine(xyz.to(device), d_model, scale)
        _bounded(y, fc.posemb_f64(xyz, d_model, scale), fc.posemb_f32(xyz, d_model, scale), 2e-6,
                 f"posemb |x|~{mag:g} n={n} d={d_model} scale={scale}")
        assert y.shape == (n, d_model) and d_model - 3 * npf > 0
        assert torch.equal(y[:, 3 * npf:].cpu(), torch.zeros(n, d_model - 3 * npf))


def test_posemb_lidar_coordinates(device):
    """The realistic 100 m class: coordinates of the synthetic LiDAR pair."""
    src, _, _ = synthetic.make_lidar_pair(6000, seed=2)
    xyz = T(np.ascontiguousarray(src[:1500]))
    assert float(xyz.abs().max()) > 20.0
    y = ops.posemb_sine(xyz.to(device), 256, 1.0)
    _bounded(y, fc.posemb_f64(xyz, 256), fc.posemb_f32(xyz, 256), 2e-6, "posemb lidar")                     # 0.25


# ---- 5. KPConv geometry on every forward route ---------------------------------------------------------------------
def _kp_run(device, q, s, nb, x, w, kp, ext, impl, srt, order=None):
    return ops.kpconv_raw(T(q).to(device), T(s).to(device), T(nb.astype(np.int32)).to(device), T(x).to(device),
                          T(w).to(device), T(kp).to(device), ext, rows_sorted=srt, impl=impl, order=order)


def _kp_check(device, q, s, nb, x, w, kp, ext, impl, srt, what):
    ref = fc.kpconv_f64(q, s, nb, x, w, kp, ext)
    y = _kp_run(device, q, s, nb, x, w, kp, ext, impl, srt)
    _bounded(y, ref, None, 1e-5, what)     # observed worst: 0.09 (offsets), 0.07 (row widths), 0.06 (counts, nq), 0.05 (exact)
    return y, ref


def test_kpconv_routes_are_what_they_name(device):
    """fc.kp_route restates spr_kpconv_fwd's dispatch; the observable that ties it to the code: ops.kpconv_raw leaves a
    tile plan on the neighbour tensor exactly when it takes the ring kernel, and a shape the tile kernel cannot hold
    (rows wider than its LDS) computes instead of failing."""
    want = {"ring32": "ring", "ring64": "ring", "ring32x128": "ring", "tile_cin128": "tile", "tile_big_w": "tile",
            "tile_impl2": "tile", "tile_impl2_64": "tile", "simple_impl1": "simple", "cin1": "cin1",
            "generic48": "simple"}
    for name, (impl, cin, cout) in fc.KP_ROUTES.items():
        assert fc.kp_route(impl, cin, cout, 40) == want[name], name
    assert fc.kp_route(0, 32, 32, 128) == "ring" and fc.kp_route(0, 32, 32, 129) == "simple"   # kmax > 128 leaves the ring,
    assert fc.kp_route(0, 64, 64, 129) == "tile" and fc.kp_route(2, 32, 32, 129) == "simple"    # and the 32-channel tile
    assert fc.kp_route(0, 64, 64, 272) == "tile" and fc.kp_route(0, 64, 64, 273) == "simple"
    ext = 0.25
    for name, (impl, cin, cout) in fc.KP_ROUTES.items():
        for kmax in (1, 40, 128, 129, 273):
            q, s, nb = fc.kp_cloud_case(20, 300, kmax, 1e2, ext, 63, rows_sorted=True)
            nbt = T(nb.astype(np.int32)).to(device)
            y = ops.kpconv_raw(T(q).to(device), T(s).to(device), nbt, T(fc.kp_features(300, cin, 64)).to(device),
                               T(fc.kp_weights(cin, cout, 65)).to(device), T(fc.random_kernel_points(ext, 66)).to(device),
                               ext, rows_sorted=True, impl=impl)
            assert torch.isfinite(y).all()
            assert hasattr(nbt, "_spr_kp_plan") == (fc.kp_route(impl, cin, cout, kmax) == "ring"), (name, kmax)


@pytest.mark.parametrize("route", list(fc.KP_ROUTES))
@pytest.mark.parametrize("offset,ext", [(1e2, 0.03), (1e3, 0.03), (1e2, 0.6), (1e3, 5.0)])
def test_kpconv_offset_coordinates(device, route, offset, ext):
    """KITTI-like geometry: large absolute coordinates, small differences; sorted and unsorted rows."""
    impl, cin, cout = fc.KP_ROUTES[route]
    for srt in (True, False):
        q, s, nb = fc.kp_cloud_case(300, 350, 20, offset, ext, 41, rows_sorted=srt)
        x, w = fc.kp_features(350, cin, 42), fc.kp_weights(cin, cout, 43)
        kp = fc.random_kernel_points(ext, 44)
        _kp_check(device, q, s, nb, x, w, kp, ext, impl, srt, f"kpconv {route} offset {offset:g} ext {ext:g} srt={srt}")


@pytest.mark.parametrize("route", list(fc.KP_ROUTES))
@pytest.mark.parametrize("kmax", [1, 8, 9, 64, 65, 128, 129])
def test_kpconv_row_widths(device, route, kmax):
    impl, cin, cout = fc.KP_ROUTES[route]
    if route.startswith("ring"):
        assert fc.kp_route(impl, cin, cout, kmax) == ("ring" if kmax <= 128 else ("tile" if cin == 64 else "simple"))
    ext = 0.25
    q, s, nb = fc.kp_cloud_case(150, 200, kmax, 1e2, ext, 45, rows_sorted=True, fill=0.9)
    x, w = fc.kp_features(200, cin, 46), fc.kp_weights(cin, cout, 47)
    _kp_check(device, q, s, nb, x, w, fc.random_kernel_points(ext, 48), ext, impl, True, f"kpconv {route} kmax {kmax}")


@pytest.mark.parametrize("route", list(fc.KP_ROUTES))
@pytest.mark.parametrize("nq", [1, 15, 16, 17])
def test_kpconv_query_counts(device, route, nq):
    impl, cin, cout = fc.KP_ROUTES[route]
    ext = 0.125
    for srt in (True, False):
        q, s, nb = fc.kp_cloud_case(nq, 120, 12, 1e2, ext, 49, rows_sorted=srt)
        x, w = fc.kp_features(120, cin, 50), fc.kp_weights(cin, cout, 51)
        _kp_check(device, q, s, nb, x, w, fc.random_kernel_points(ext, 52), ext, impl, srt,
                  f"kpconv {route} nq {nq} srt={srt}")


@pytest.mark.parametrize("route", list(fc.KP_ROUTES))
@pytest.mark.parametrize("offset,ext", [(0.0, 0.0625), (1e2, 0.0625), (1e3, 0.25)])
def test_kpconv_exact_geometry(device, route, offset, ext):
    """Neighbours exactly on a kernel point, exactly at distance extent, one representable step inside / outside it,
    query and support coincident.  Only the centre kernel point carries weights in the isolating run, so that the row
    of the neighbour AT the extent shows the centre influence alone.  Every operation of that influence is exact on this
    lattice in float32 (the coordinate difference is the extent, its square a power of four, 1 / extent a power of
    two, 1 - 1 = 0), so the row is EXACTLY 0 on every route, as in the reference -- also with the hardware's 1-ulp
    square root, which is exact on powers of four (observed: 0.0 on all ten routes).  A 1 / extent one ulp low would
    leave an influence of 2^-24 there."""
    impl, cin, cout = fc.KP_ROUTES[route]
    q, s, nb, names = fc.kp_exact_case(offset, ext)
    ns = s.shape[0]
    x = np.abs(fc.kp_features(ns, cin, 53)) + 0.5
    w = fc.kp_weights(cin, cout, 54)
    kp = fc.lattice_kernel_points(ext)
    for srt in (True, False):
        y, ref = _kp_check(device, q, s, nb, x, w, kp, ext, impl, srt, f"kpconv exact {route} offset {offset:g} srt={srt}")
    # on a kernel point: the float64 influence is exactly 1 -- the row is the plain product x W[p] (+ the other points)
    w0 = np.zeros_like(w)
    w0[0] = w[0]
    y0, ref0 = _kp_check(device, q, s, nb, x, w0, kp, ext, impl, True, f"kpconv exact centre-only {route} offset {offset:g}")
    y0 = y0.cpu().numpy().astype(np.float64)
    full = np.abs(x.astype(np.float64)) @ np.abs(w[0].astype(np.float64))          # [ns, cout]
    assert np.array_equal(ref0[names["at_extent"]], np.zeros(cout)) and np.array_equal(ref0[names["outside"]], np.zeros(cout))
    for r in ("at_extent", "outside"):
        i = names[r]
        print(f"kpconv exact {route} offset {offset:g}: max |out| of the {r} row {np.abs(y0[i]).max():.3e}")
        assert np.all(y0[i] == 0.0), f"{route}: centre influence {r} is not exactly 0: {np.abs(y0[i]).max():.3e}"
    i = names["coincident"]
    assert np.all(np.abs(y0[i] - ref0[i]) <= 2.0 ** -21 * full[i] + 1e-5 * np.abs(ref0[i]))   # influence exactly 1
    assert np.all(ref0[names["inside"]] != 0.0)


@pytest.mark.parametrize("route", list(fc.KP_ROUTES))
def test_kpconv_neighbour_count_edges(device, route):
    """Small-integer features (a row sum is exact in any order, so the count cannot differ from the float64 reference
    by summation order): rows of only shadow entries, rows whose valid neighbours all have a feature sum <= 0 (the
    count clamps at 1), support rows whose features sum to exactly 0."""
    impl, cin, cout = fc.KP_ROUTES[route]
    ext, ns, nq, kmax = 0.125, 160, 90, 10
    q, s, nb = fc.kp_cloud_case(nq, ns, kmax, 1e2, ext, 55, rows_sorted=True, fill=0.8)
    x = fc.kp_features(ns, cin, 56, integer=True)
    if cin > 1:
        x[:40, 0] -= x[:40].sum(1)                       # support rows 0..39 sum to exactly 0
        x[40:80, 0] -= x[40:80].sum(1) + 1               # rows 40..79 sum to -1
    else:
        x[:40], x[40:80] = 0.0, -1.0
    assert np.all(x[:40].sum(1) == 0) and np.all(x[40:80].sum(1) == -1) and np.all(np.abs(x) < 2 ** 10)
    nb[5:25] = np.where(nb[5:25] < ns, nb[5:25] % 80, ns)   # queries 5..24 see only rows with sum <= 0
    nb[3] = ns
    w = fc.kp_weights(cin, cout, 57)
    y, ref = _kp_check(device, q, s, nb, x, w, fc.random_kernel_points(ext, 58), ext, impl, True, f"kpconv counts {route}")
    assert torch.equal(y[3].cpu(), torch.zeros(cout))
    cnt = ((x[np.where(nb < ns, nb, 0)].sum(-1) > 0) & (nb < ns)).sum(1)
    assert np.all(cnt[5:25] == 0) and cnt.max() > 1


@pytest.mark.parametrize("cin,cout", [(32, 32), (64, 64), (32, 128), (64, 128), (128, 64), (48, 24), (1, 64)])
def test_kpconv_routes_agree(device, cin, cout):
    """All routes that accept a shape agree within 2e-6 (as test_kpconv_ring_kernel_vs_oracle does), and the ring
    kernel is bitwise independent of the tile walk."""
    ext = 0.0625
    q, s, nb = fc.kp_cloud_case(333, 400, 37, 1e3, ext, 59, rows_sorted=True)
    x, w, kp = fc.kp_features(400, cin, 60), fc.kp_weights(cin, cout, 61), fc.random_kernel_points(ext, 62)
    ys = {impl: _kp_run(device, q, s, nb, x, w, kp, ext, impl, True).cpu().double() for impl in (0, 1, 2)}
    scale = float(ys[1].abs().max())
    for a, b in ((0, 1), (0, 2), (1, 2)):
        d = float((ys[a] - ys[b]).abs().max())
        assert d <= 2e-6 * scale, f"kpconv {cin}->{cout}: impl {a} vs {b}: {d / scale:.3e}"
    if fc.kp_route(0, cin, cout, 37) == "ring":
        order = T(np.random.default_rng(3).permutation(333).astype(np.int32)).to(device)
        assert torch.equal(_kp_run(device, q, s, nb, x, w, kp, ext, 0, True, order=order).cpu().double(), ys[0])


# ---- 6. published ranges are the true maxima -----------------------------------------------------------------------
KP_WF_SLACK = 2.0 ** 5      # autograd.py: "a bound within 2^3..2^5 of the true maximum"
def _published(t):
    parts, n = ops._get_range(t)
    return None if parts is None else float(parts[:n].max())


def _plant(x, where, value):
    """x with |value| planted at the first element, the last element of the last row, or the first element of a row
    inside the final partial tile / unroll step."""
    x = x.clone()
    m = x.shape[0]
    r, c = {"first": (0, 0), "last": (m - 1, x.shape[1] - 1), "tail_row": (m - 1 - min(2, m - 1), 0)}[where]
    x[r, c] = value
    return x


WHERE = ["first", "last", "tail_row"]


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("n,c", [(1025, 4), (2151, 64), (33, 68), (4100, 256)])
def test_range_instnorm_and_maxpool(device, n, c, where):
    """k_in_apply and k_maxpool publish max |out| over what they wrote; run twice on one stream, the second time with
    smaller data (fresh slots)."""
    cu = ops.lengths_to_cu([n], device)
    for big in (1e4, 1e-3):
        x = _plant(synthetic.rand((n, c), 71) * big * 0.01, where, -big).to(device)
        y = ops.instnorm(x, cu, norm=False, slope=1.0)
        assert _published(y) == float(y.abs().max()) == float(np.float32(big))
        z = ops.instnorm(x, cu, slope=0.1)
        assert _published(z) == float(z.abs().max())
        idx = torch.arange(n, dtype=torch.int32, device=device).view(-1, 1).repeat(1, 3)
        p = ops.maxpool(x.abs(), idx)
        assert _published(p) == float(p.abs().max()) == float(np.float32(big))
        pn = ops.maxpool(x, idx)                          # the planted value is negative: |max| counts
        assert _published(pn) == float(pn.abs().max())


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("m,c", [(1, 64), (257, 256), (4099, 256), (255, 512), (4100, 1024)])
def test_range_layernorm_both_outputs(device, m, c, where):
    for big in (50.0, 0.5):
        x, g, b, pos = fc.ln_data(m, c, 0.0, 1.0, 72)
        x = _plant(x, where, 40.0 * big)                  # that row's normalised value is the tensor's largest
        pos = _plant(pos * 0.01, where, big)
        n, npos = ops.layernorm(x.to(device), g.to(device), b.to(device), 1e-5, pos=pos.to(device))
        assert _published(n) == float(n.abs().max())
        assert _published(npos) == float(npos.abs().max())
        _, p2 = ops.layernorm(x.to(device), g.to(device), b.to(device), 1e-5, pos=pos.to(device), want_norm=False)
        assert _published(p2) == float(p2.abs().max())


@pytest.mark.parametrize("where", WHERE)
@pytest.mark.parametrize("act", [ops.ACT_NONE, ops.ACT_RELU, ops.ACT_SIGMOID])
@pytest.mark.parametrize("m,k,n,kernel", [(1153, 256, 300, "persistent"), (8200, 64, 1000, "256x256"),
                                          (300, 64, 96, "128x64"), (129, 256, 257, "128x64")])
def test_range_linear_tiles(device, m, k, n, kernel, act, where):
    """spr_linear without residual publishes one maximum per output tile: the persistent 128x256 tiles (k = 256,
    1024 <= m < 32768, n >= 256), the 256x256 tiles (>= 128 of them) and the 128x64 tiles."""
    persistent = n >= 256 and k == 256 and 1024 <= m < 32768
    big_tiles = not persistent and n >= 256 and m >= 256 and -(-n // 256) * -(-m // 256) >= 128
    assert {"persistent": persistent, "256x256": big_tiles, "128x64": not persistent and not big_tiles and n > 32}[kernel]
    ops.set_gemm_mode(1)
    w = (synthetic.rand((n, k), 73) * 0.05).to(device)
    for big in (30.0, 0.25):
        bias = (synthetic.rand((n,), 70) * 0.01 * big).to(device)
        x = synthetic.rand((m, k), 74) * 0.01 * big
        row = {"first": 0, "last": m - 1, "tail_row": m - 3}[where]
        x[row] *= 40.0                                    # the largest outputs sit in that row, for every activation
        y = ops.linear(x.to(device), w, bias, act=act)
        parts, cnt = ops._get_range(y)
        tiles = -(-n // 256) * -(-m // 128) if persistent else (-(-n // 256) * -(-m // 256) if big_tiles
                                                               else -(-n // 64) * -(-m // 128))
        assert cnt == tiles
        assert float(parts[:cnt].max()) == float(y.abs().max())
        assert int(y.abs().max(1)[0].argmax()) == row


def test_range_linear_not_published(device):
    """n <= 32 publishes nothing; with a residual nothing; more tiles than the caller's capacity: nothing, not a
    partial set ("only if it fits")."""
    ops.set_gemm_mode(1)
    x = synthetic.rand((300, 64), 75).to(device)
    assert ops._get_range(ops.linear(x, synthetic.rand((32, 64), 76).to(device))) == (None, 0)
    w = synthetic.rand((96, 64), 77).to(device)
    assert ops._get_range(ops.linear(x, w, residual=torch.zeros(300, 96, device=device))) == (None, 0)
    m = 128 * 1366 + 5                                    # 3 column tiles x 1367 row tiles = 4101 > 4096
    xl = synthetic.rand((m, 32), 69).to(device)
    y = ops.linear(xl, synthetic.rand((192, 32), 78).to(device))
    assert ops._get_range(y) == (None, 0) and not hasattr(y, "_spr_range")
    y = ops.linear(xl[:128 * 1365], synthetic.rand((192, 32), 78).to(device))    # 4095 tiles fit
    assert ops._get_range(y)[1] == 4095 and _published(y) == float(y.abs().max())


@pytest.mark.parametrize("T_", [256, 515])
def test_range_attention_inproj_is_a_bound(device, T_):
    """The fused in-projection + attention publishes a derived BOUND of its output (one slot): the output is a convex
    combination of value rows, |v| <= vb = max|x_v| * max_row L1(W_v) + max|b_v|, and the slot holds the power of two
    2^(15 - ev) with vb 2^ev in [2^14, 2^15) (csrc/attention.hip k_plane_scales): >= the true maximum, <= 2 vb."""
    d, nhead = 256, 8
    lens = [T_ - 100, 100]
    for big in (5.0, 0.05):
        x = synthetic.rand((T_, d), 79) * big
        w_in, b_in = synthetic.rand((3 * d, d), 80) * 0.05, synthetic.rand((3 * d,), 81) * 0.1
        cu = ops.lengths_to_cu(lens, device)
        kv = torch.arange(len(lens), dtype=torch.int32, device=device)
        xd = x.to(device)
        y = ops.attention_inproj(xd, xd, w_in.to(device), b_in.to(device), cu, kv, max(lens), nhead)
        parts, cnt = ops._get_range(y)
        assert cnt == 1
        true = float(y.abs().max())
        vb = float(x.abs().max()) * float(w_in[2 * d:].abs().double().sum(1).max()) + float(b_in[2 * d:].abs().max())
        assert true <= float(parts[0]) <= 2.0 * vb * (1 + 1e-6), (true, float(parts[0]), vb)


def test_range_block_tail(device):
    """spr_block_tail publishes max |out| over what it wrote (tail rows of the last statistics tile included)."""
    ka, n_out = 64, 256
    assert ops.block_tail_tile_rows(ka, 0, n_out) > 0
    for where in WHERE:
        L = [257, 1301, 77]
        n = sum(L)
        for big in (100.0, 0.01):
            xa = synthetic.rand((n, ka), 82)
            wa = (synthetic.rand((n_out, ka), 83) * 0.1)
            add = _plant(synthetic.rand((n, n_out), 84) * big * 0.01, where, big)
            out = ops.block_tail(xa.to(device), wa.to(device), ops.lengths_to_cu(L, device), add=add.to(device))
            assert _published(out) == float(out.abs().max())


@pytest.mark.parametrize("kmax,fill", [(1, 1.0), (8, 0.9), (40, 0.7), (50, 0.9), (50, 0.05), (51, 0.9), (129, 0.9), (129, 0.05)])
@pytest.mark.parametrize("cin,cout", [(32, 32), (64, 64)])
def test_range_kpconv_backward_weighted_features_bound(device, monkeypatch, cin, cout, kmax, fill):
    """The KPConv backward attaches kmax * max|x| to its weighted features wf (autograd.py: every influence is <= 1)
    instead of scanning them: a BOUND, exactly kmax times x's published maximum, >= max |wf|, and within the 2^5 the
    code's comment states.  Observed published / true: 1.0 at kmax 1, 3.1 at 8, 16.6 at 40; 35 at 64 with mostly-shadow
    rows and 49 / 55 at 129 broke the 2^5 of the comment as first written, so rows wider than
    autograd.KP_WF_BOUND_MAX_ROW = 50 now get no bound and the consuming product measures wf."""
    from superpoints_registration_amd import autograd as ag
    ext, nq, ns = 0.25, 200, 260
    q, s, nb = fc.kp_cloud_case(nq, ns, kmax, 1e2, ext, 91, rows_sorted=True, fill=fill)
    x0 = T(fc.kp_features(ns, cin, 92)).to(device)
    x = ops.instnorm(x0, ops.lengths_to_cu([ns], device), norm=False, slope=1.0)      # publishes max |x|
    xmax = _published(x)
    assert xmax == float(x0.abs().max())
    x.requires_grad_(True)
    w = T(fc.kp_weights(cin, cout, 93)).to(device).requires_grad_(True)
    seen = []
    real = ops._set_range

    def spy(t, parts, n, guard=None):
        if t.dim() == 2 and t.shape == (nq, 15 * cin) and parts.numel() == ops._STREAM_SLOTS:   # (d wf has the same
            seen.append((t, parts, n))                       # shape; its range is a linear product's, _RANGE_CAP slots)
        return real(t, parts, n, guard)

    monkeypatch.setattr(ag._ops, "_set_range", spy)
    y = ops.kpconv(T(q).to(device), T(s).to(device), T(nb.astype(np.int32)).to(device), x, w,
                   T(fc.random_kernel_points(ext, 94)).to(device), ext, rows_sorted=True)
    y.sum().backward()
    assert float((x.grad.abs().max())) > 0 and float(w.grad.abs().max()) > 0
    if kmax > ag.KP_WF_BOUND_MAX_ROW:
        assert not seen, "a row this wide must be measured, not bounded"
        return
    assert len(seen) == 1, "the backward did not attach a range to its weighted features"
    wf, parts, n = seen[0]
    pub, true = float(parts[:n].max()), float(wf.abs().max())
    print(f"kpconv backward wf bound kmax={kmax} fill={fill} cin={cin}: published {pub:.3e} true {true:.3e} ratio {pub / true:.1f}")
    assert pub == float(np.float32(xmax) * np.float32(kmax))
    assert true > 0 and pub >= true
    assert pub <= KP_WF_SLACK * true
