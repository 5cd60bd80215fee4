"""Host: the case generators and float64 references of tests/forward_cases.py (used by the GPU module
tests/test_gpu_forward_range.py) are anchored without a GPU -- they agree with oracle/torch_oracle.py on the generated
cases, the oracle agrees with the reference project's golden vectors (tests/golden/ops.npz) on the golden inputs, and
no generated case is vacuous: the float32 baseline is finite and the float64 reference is nonzero."""
import numpy as np
import pytest
import torch

import forward_cases as fc
from conftest import load_golden
from oracle import torch_oracle as O
from oracle.gen_golden import ops_inputs

T = torch.from_numpy
F64 = torch.float64


def _live(ref64, base32, what):
    ref64 = torch.as_tensor(ref64)
    assert torch.isfinite(torch.as_tensor(base32)).all(), f"{what}: float32 baseline not finite"
    assert torch.isfinite(ref64).all() and float(ref64.abs().max()) > 0.0, f"{what}: float64 reference is vacuous"


# ---- the oracle against the reference's goldens --------------------------------------------------------------------
def test_oracle_matches_reference_goldens():
    gold, inp = load_golden("ops.npz"), ops_inputs()
    lens = [int(v) for v in inp["kp.lens"]]
    y = O.lrelu(O.instance_norm(inp["in.x"], lens))
    assert float((y - T(gold["in.y"])).abs().max()) <= 2e-6 * float(np.abs(gold["in.y"]).max())
    assert np.array_equal(O.max_pool(inp["in.x"], T(gold["mp.idx"].astype(np.int64))).numpy(), gold["mp.y"])
    pe = O.posemb_sine(inp["pe.xyz"], 256)
    assert float((pe - T(gold["pe.y"])).abs().max()) <= 2e-6
    pts, nb = T(inp["kp.pts"]), T(gold["kp.nb"].astype(np.int64))
    for tag in ("c1", "c32", "c64", "c128", "c48"):
        y = O.kpconv(pts, pts, nb, inp[f"kp.{tag}.x"], inp[f"kp.{tag}.w"], T(gold[f"kp.{tag}.kpts"]), inp["kp.extent"])
        g = gold[f"kp.{tag}.y"]
        assert float((y - T(g)).abs().max()) <= 1e-5 * float(np.abs(g).max()), tag


def test_new_references_match_goldens_too():
    """The float64 restatements themselves on the golden inputs (float32 goldens: 2e-6 / 1e-5 of scale)."""
    gold, inp = load_golden("ops.npz"), ops_inputs()
    lens = [int(v) for v in inp["kp.lens"]]
    y = fc.instnorm_f64(inp["in.x"], lens, slope=0.1)
    assert float((y - T(gold["in.y"]).double()).abs().max()) <= 2e-6 * float(np.abs(gold["in.y"]).max())
    assert np.array_equal(fc.maxpool_np(inp["in.x"].numpy(), gold["mp.idx"]), gold["mp.y"])
    # the golden is the reference's float32 evaluation: three roundings of an argument of up to max|x| 2 pi
    arg = float(inp["pe.xyz"].abs().max()) * 2 * np.pi
    assert float((fc.posemb_f64(inp["pe.xyz"], 256) - T(gold["pe.y"]).double()).abs().max()) <= 3 * arg * 2.0 ** -24 + 2.0 ** -23
    for tag in ("c1", "c32", "c48"):
        y = fc.kpconv_f64(inp["kp.pts"], inp["kp.pts"], gold["kp.nb"], inp[f"kp.{tag}.x"].numpy(),
                          inp[f"kp.{tag}.w"].numpy(), gold[f"kp.{tag}.kpts"], inp["kp.extent"])
        g = gold[f"kp.{tag}.y"]
        assert np.abs(y - g).max() <= 1e-5 * np.abs(g).max(), tag


# ---- the new references against the oracle on the generated cases --------------------------------------------------
@pytest.mark.parametrize("c", fc.IN_WIDTHS)
@pytest.mark.parametrize("centre,spread", fc.IN_REGIMES)
def test_instnorm_cases(c, centre, spread):
    L = fc.IN_LENGTHS
    assert sum(L) % 2 == 1 and (sum(L) * (c // 4)) % 1024 != 0        # the last cloud ends off an unroll boundary
    assert max(L) > 2 * 512                                           # several statistics slices
    x = fc.in_data(L, c, centre, spread, 1)
    add = fc.in_add(x.shape[0], c, 2) * float(spread if centre == 0 else 1.0)
    ref = fc.instnorm_f64(x, L, slope=0.1)
    orc = O.lrelu(O.instance_norm(x.double(), L))                     # the oracle, kept in float64
    assert float((ref - orc).abs().max()) <= 1e-9 * float(ref.abs().max())
    _live(ref, fc.instnorm_f32(x, L, slope=0.1), f"instnorm c={c} ({centre:g},{spread:g})")
    for a, slope in ((add, 0.1), (add, 1.0)):
        _live(fc.instnorm_f64(x, L, add=a, slope=slope), fc.instnorm_f32(x, L, add=a, slope=slope), "instnorm + add")
    # every cloud of more than one point contributes a nonzero block
    off = 0
    for l in L:
        assert l == 1 or float(ref[off:off + l].abs().max()) > 0
        off += l


def test_instnorm_edge_cases():
    for c in (4, 68, 256):
        L = [1, 7, 600, 1]
        x, add = fc.in_constant(L, c, 3), fc.in_add(609, c, 4)
        m, r = fc.instnorm_stats_f64(x, L)
        assert float((r - 1.0 / np.sqrt(1e-5)).abs().max()) <= 1e-9 / np.sqrt(1e-5)  # variance exactly 0 (up to f64 rounding)
        _live(fc.instnorm_f64(x, L, add=add, slope=0.1), fc.instnorm_f32(x, L, add=add, slope=0.1), "constant clouds")
    L = fc.IN_LENGTHS_EMPTY
    x = fc.in_data(L, 64, 0.0, 1.0, 7)
    dense = [l for l in L if l > 0]
    assert torch.equal(fc.instnorm_f64(x, L), fc.instnorm_f64(x, dense))
    m, r = fc.instnorm_stats_f64(x, L)
    assert float(m[1].abs().max()) == 0.0 and float((r[1] - 1e-5 ** -0.5).abs().max()) < 1e-9
    _live(fc.instnorm_f64(x, L), fc.instnorm_f32(x, L), "empty clouds")


@pytest.mark.parametrize("centre,spread", fc.LN_REGIMES)
def test_layernorm_cases(centre, spread):
    for m in fc.LN_ROWS:
        for c in fc.LN_WIDTHS:
            x, g, b, pos = fc.ln_data(m, c, centre, spread, 11)
            ref = fc.layernorm_f64(x, g, b)
            orc = torch.nn.functional.layer_norm(x.double(), (c,), g.double(), b.double(), 1e-5)
            assert float((ref - orc).abs().max()) <= 1e-9 * float(ref.abs().max())
            _live(ref, fc.layernorm_f32(x, g, b), f"layernorm {m}x{c}")


def test_maxpool_cases():
    for k in fc.MP_K:
        for c in fc.MP_WIDTHS:
            x, idx, rows = fc.mp_case(97, 203, k, c, 21)
            ref = fc.maxpool_np(x, idx)
            assert np.array_equal(ref, O.max_pool(T(x), T(idx)).numpy())
            assert np.all(ref[rows["all_shadow"]] == 0) and np.all(ref[rows["neg_no_shadow"]] < 0)
            assert k == 1 or np.all(ref[rows["neg_one_shadow"]] == 0)
            assert (idx == 97).any() and (ref > 0).any() and (ref < 0).any()
    for k in (1, 3, 4, 9):
        x, idx = fc.mp_extreme(k, 8, 22)
        ref = fc.maxpool_np(x, idx)
        assert np.array_equal(ref.view(np.int32), O.max_pool(T(x), T(idx)).numpy().view(np.int32))
        assert np.isneginf(ref).any() and (ref == -fc.F32_MAX).any() and (ref == np.float32(-3.2e38)).any()
        assert np.isposinf(ref).any() and (ref == fc.F32_MAX).any() and (ref == 0).any()
    x = np.arange(12, dtype=np.float32).reshape(4, 3)
    assert np.array_equal(fc.gather_np(x, [3, 4, -1, 0]), np.stack([x[3], 0 * x[0], 0 * x[0], x[0]]))


@pytest.mark.parametrize("mag", fc.PE_MAGS)
def test_posemb_cases(mag):
    for n in fc.PE_ROWS:
        for d in fc.PE_DMODEL:
            xyz = fc.pe_xyz(n, mag, 31)
            for scale in fc.PE_EXTRA_SCALES:
                rs, bs = fc.posemb_f64(xyz, d, scale), fc.posemb_f32(xyz, d, scale)
                _live(rs, bs, f"posemb {mag:g} scale {scale}")
                assert torch.equal(bs, O.posemb_sine(xyz, d, scale))
                assert float((bs.double() - rs).abs().max()) <= 4 * max(mag * scale * 2 * np.pi, 1.0) * 2.0 ** -23
            ref, b32 = fc.posemb_f64(xyz, d), fc.posemb_f32(xyz, d)
            _live(ref, b32, f"posemb {mag:g}")
            assert torch.equal(b32, O.posemb_sine(xyz, d))            # the baseline IS the oracle's float32 expression
            npf = d // 3 // 2 * 2
            assert d - 3 * npf >= 2 and float(ref[:, 3 * npf:].abs().max()) == 0.0
            err32 = float((b32.double() - ref).abs().max())
            # one rounding of the argument: |x| 2 pi 2^-24 per operation, three operations
            assert err32 <= 4 * max(mag * 2 * np.pi, 1.0) * 2.0 ** -23
    assert fc.PE_DMODEL[1] - 3 * (fc.PE_DMODEL[1] // 3 // 2 * 2) != 256 - 3 * 84


# ---- KPConv --------------------------------------------------------------------------------------------------------
def test_kpconv_routes_named():
    assert {fc.kp_route(i, ci, co, 40) for i, ci, co in fc.KP_ROUTES.values()} == {"ring", "tile", "simple", "cin1"}
    assert fc.kp_route(0, 64, 128, 40) == "tile" and fc.kp_route(0, 128, 64, 40) == "tile"     # cin * cout > 4096, cin = 128
    assert fc.kp_route(0, 64, 64, 129) == "tile" and fc.kp_route(0, 32, 32, 129) == "simple" and fc.kp_route(2, 64, 64, 8) == "tile"
    assert fc.kp_route(1, 32, 32, 8) == "simple" and fc.kp_route(0, 48, 24, 8) == "simple"


@pytest.mark.parametrize("offset,ext", [(1e2, 0.03), (1e3, 0.03), (1e2, 0.6), (1e3, 5.0)])
def test_kpconv_cloud_cases_match_oracle(offset, ext):
    for cin, cout in ((1, 64), (32, 32), (48, 24)):
        for srt in (True, False):
            q, s, nb = fc.kp_cloud_case(300, 350, 20, offset, ext, 41, rows_sorted=srt)
            x, w, kp = fc.kp_features(350, cin, 42), fc.kp_weights(cin, cout, 43), fc.random_kernel_points(ext, 44)
            ref = fc.kpconv_f64(q, s, nb, x, w, kp, ext)
            orc = O.kpconv(T(q).double(), T(s).double(), T(nb), T(x).double(), T(w).double(), T(kp).double(), ext)
            assert np.abs(ref - orc.numpy()).max() <= 1e-9 * np.abs(ref).max()
            assert np.isfinite(ref).all() and np.abs(ref).max() > 0
            assert (nb[3] == 350).all() and nb[0, 0] == 0 and np.array_equal(q[0], s[0])
            assert np.abs(q).max() >= 0.9 * offset
            if srt:
                valid = nb < 350
                assert np.all(valid[:, 1:] <= valid[:, :-1])         # shadow entries trail
            else:
                assert ((nb[:, 0] == 350) & (nb[:, 1:] < 350).any(1)).any()
            # influences are not trivial: a fair share of (neighbour, kernel point) pairs lies inside the extent
            d = np.linalg.norm((s.astype(np.float64)[np.where(nb < 350, nb, 0)] - q.astype(np.float64)[:, None])[:, :, None]
                               - kp.astype(np.float64)[None, None], axis=-1)
            assert ((d < ext) & (nb < 350)[:, :, None]).mean() > 0.02


@pytest.mark.parametrize("offset,ext", [(0.0, 0.0625), (1e2, 0.0625), (1e3, 0.25)])
def test_kpconv_exact_case_is_exact(offset, ext):
    q, s, nb, names = fc.kp_exact_case(offset, ext)
    kp = fc.lattice_kernel_points(ext).astype(np.float64)
    assert np.array_equal(kp[0], np.zeros(3)) and kp.shape == (15, 3)
    rel = s.astype(np.float64) - q[:1].astype(np.float64)
    d0 = np.linalg.norm(rel, axis=1)                                  # distance to the centre kernel point
    assert d0[names["coincident"]] == 0.0 and d0[names["at_extent"]] == ext
    assert 0 < ext - d0[names["inside"]] <= 2.0 ** -13 * max(abs(offset), 2 * ext)
    assert 0 < d0[names["outside"]] - ext <= 2.0 ** -13 * max(abs(offset), 2 * ext)
    for p in names["on_kp"]:
        assert np.array_equal(rel[p], kp[p])
    x = np.abs(fc.kp_features(s.shape[0], 32, 53)) + 0.5
    w = fc.kp_weights(32, 32, 54)
    w0 = np.zeros_like(w)
    w0[0] = w[0]
    ref0 = fc.kpconv_f64(q, s, nb, x, w0, kp, ext)
    assert np.all(ref0[names["at_extent"]] == 0) and np.all(ref0[names["outside"]] == 0)
    assert np.all(ref0[names["inside"]] != 0) and np.allclose(ref0[0], x[0].astype(np.float64) @ w[0], rtol=1e-12)
    orc = O.kpconv(T(q).double(), T(s).double(), T(nb), T(x).double(), T(w).double(), T(kp), ext)
    assert np.abs(fc.kpconv_f64(q, s, nb, x, w, kp, ext) - orc.numpy()).max() <= 1e-9


def test_kpconv_integer_features_make_the_count_order_free():
    x = fc.kp_features(160, 64, 56, integer=True)
    assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 2
    for perm_seed in range(3):
        p = np.random.default_rng(perm_seed).permutation(64)
        assert np.array_equal(x.sum(1), x[:, p].sum(1, dtype=np.float32))


def _kp_live(q, s, nb, x, w, kp, ext, what):
    ref = fc.kpconv_f64(q, s, nb, x, w, kp, ext)
    orc = O.kpconv(T(q).double(), T(s).double(), T(nb), T(x).double(), T(w).double(), T(kp).double(), ext)
    assert np.abs(ref - orc.numpy()).max() <= 1e-9 * np.abs(ref).max(), what
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0, what
    return ref


@pytest.mark.parametrize("route", list(fc.KP_ROUTES))
def test_kpconv_every_other_generated_case_is_live(route):
    """The row-width, query-count, count-edge and route-agreement cases of the GPU module, with its seeds."""
    impl, cin, cout = fc.KP_ROUTES[route]
    for kmax in (1, 8, 9, 64, 65, 128, 129):
        q, s, nb = fc.kp_cloud_case(150, 200, kmax, 1e2, 0.25, 45, rows_sorted=True, fill=0.9)
        _kp_live(q, s, nb, fc.kp_features(200, cin, 46), fc.kp_weights(cin, cout, 47), fc.random_kernel_points(0.25, 48),
                 0.25, f"kmax {kmax}")
    for nq in (1, 15, 16, 17):
        for srt in (True, False):
            q, s, nb = fc.kp_cloud_case(nq, 120, 12, 1e2, 0.125, 49, rows_sorted=srt)
            _kp_live(q, s, nb, fc.kp_features(120, cin, 50), fc.kp_weights(cin, cout, 51),
                     fc.random_kernel_points(0.125, 52), 0.125, f"nq {nq}")
    q, s, nb = fc.kp_cloud_case(333, 400, 37, 1e3, 0.0625, 59, rows_sorted=True)
    _kp_live(q, s, nb, fc.kp_features(400, cin, 60), fc.kp_weights(cin, cout, 61), fc.random_kernel_points(0.0625, 62),
             0.0625, "routes agree")
    q, s, nb = fc.kp_cloud_case(90, 160, 10, 1e2, 0.125, 55, rows_sorted=True, fill=0.8)
    x = fc.kp_features(160, cin, 56, integer=True)
    _kp_live(q, s, nb, x, fc.kp_weights(cin, cout, 57), fc.random_kernel_points(0.125, 58), 0.125, "integer features")
