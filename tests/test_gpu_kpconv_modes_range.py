"""GPU: KPConv's six rigid modes (csrc/kpconv_modes.hip) on every forward route and the two backward kernels, at the
geometry, shape and magnitude edges that section 5 of tests/test_gpu_forward_range.py holds the shipped linear / sum
kernels to: KITTI-like offsets, row widths around the 64-column staging chunk, query counts around the 32-query tile,
odd staged-neighbour counts, exact lattice geometry, exact arg-min ties, neighbour-count edges, kernel-point counts up
to the limits of each entry point, influence underflow; then operand magnitudes and ranges of the split-fp16 tile
kernel.  Inputs and their conditions: tests/kpconv_modes_cases.py, checked without a GPU by
tests/test_kpconv_modes_range_host.py.

Reference: kpconv_modes_cases.kpconv_ref in float64 (differentiated by autograd for d x, d W).  Bounds, the module's
own (tests/test_gpu_kpconv_modes.py): forward <= 1e-5 of the output's scale, d x and d W <= 2e-5 of theirs.

Near-ties in `closest`: float32 and float64 may pick different kernel points where the two lowest d2 differ by less
than GAP_MIN (relative).  A query row holding such an item (kpconv_modes_cases.near_tie_rows, float64 values alone; at
most 10 % of a case's live rows, asserted on the CPU) leaves the strict comparison and must only be finite; in the
backward its output gradient is zero, so that it contributes to neither d x nor d W.  The `sum` modes exclude nothing,
and an exact tie is not a near-tie: both arithmetics see it.

Observed worst err / bound ratios (forward, d x, d W) are written next to each check."""
import numpy as np
import pytest
import torch

import kpconv_modes_cases as kc
from superpoints_registration_amd import kpconv_modes, ops, synthetic

pytestmark = pytest.mark.gpu
T = torch.from_numpy
FWD, BWD = 1e-5, 2e-5
_REF = {}


def _dev(case, device):
    return {k: (v.clone().to(device) if isinstance(v, torch.Tensor) else v) for k, v in case.items()}


def _run(d, mode, impl):
    return kpconv_modes.kpconv(d["q"], d["s"], d["idx"], d["x"], d["w"], d["kp"], d["extent"], mode[0], mode[1], impl=impl)


def _strict(case, mode):
    """The rows compared strictly: all of them in a sum mode; in closest all but the near-tie rows, which may be at most
    NEAR_TIE_CAP of the live rows -- asserted here for every case that comes through, whatever the host module lists."""
    rows = torch.ones(case["q"].shape[0], dtype=torch.bool)
    if mode[1] != 'closest':
        return rows
    out, live = kc.near_tie_share(case)
    assert out <= kc.NEAR_TIE_CAP * live, f"{out} of {live} live rows hold a near-tie: over the cap, pick another case"
    return rows & ~kc.near_tie_rows(case)


def _go(case, strict):
    go = synthetic.rand((case["q"].shape[0], case["w"].shape[2]), 77)
    return go * strict.unsqueeze(1).to(go.dtype)


def _ref(key, case, mode, backward):
    """(strict rows, go, out64, dx64, dw64) of a case, computed once per (key, mode)."""
    k = (key, mode, backward)
    if k not in _REF:
        if len(_REF) >= 16:
            _REF.clear()                      # a reference serves the checks of one test; nothing is kept for long
        strict = _strict(case, mode)
        if backward:
            go = _go(case, strict)
            _REF[k] = (strict, go) + tuple(kc.ref64(case, mode[0], mode[1], go))
        else:
            _REF[k] = (strict, None, kc.ref64(case, mode[0], mode[1]), None, None)
    return _REF[k]


def _ratio(what, got, ref, bound, rows=None):
    """err / (bound * scale) over the strict rows, printed; everything finite."""
    got = got.detach().double().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    scale = float(ref.abs().max())
    diff = (got - ref).abs()
    err = float((diff if rows is None else diff[rows]).max()) if diff.numel() else 0.0
    ratio = err / max(bound * scale, 1e-300)
    print(f"{what}: err {err:.3e} scale {scale:.3e} ratio {ratio:.3f}")
    assert scale > 0, f"{what}: a vacuous case"
    assert err <= bound * scale, f"{what}: {err:.3e} > {bound:g} * {scale:.3e}"
    return ratio


def check(device, key, case, route, mode, backward=False, what=None):
    """Forward (and d x, d W through KPConvModesFn) of one case on one route in one mode against float64."""
    impl = kc.ROUTES[route][0]
    what = what or f"{key} {route} {'-'.join(mode)}"
    strict, go, ref, dx_ref, dw_ref = _ref(key, case, mode, backward)
    d = _dev(case, device)
    with torch.no_grad():
        out = _run(d, mode, impl)
    _ratio(what, out, ref, FWD, strict)
    if backward:
        x, w = d["x"].requires_grad_(True), d["w"].requires_grad_(True)
        y = _run(dict(d, x=x, w=w), mode, impl)
        assert torch.equal(y.detach(), out), f"{what}: the differentiable call gives other bits"
        y.backward(go.to(device))
        _ratio(what + " dx", x.grad, dx_ref, BWD)
        _ratio(what + " dW", w.grad, dw_ref, BWD)
    return out


def test_routes_are_what_they_name():
    for name, (impl, cin, cout, n_kp) in kc.ROUTES.items():
        assert kc.modes_route(impl, cin, cout, n_kp) == kc.ROUTE_KERNEL[name], name


# ---- 1. geometry and shape edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["tile32", "tile64", "simple48", "cin1"])
@pytest.mark.parametrize("offset,ext", kc.OFFSETS)
def test_offset_coordinates(device, route, offset, ext):
    """KITTI-like geometry: coordinates of 1e2 / 1e3 and differences of an extent, sorted and unsorted rows, all six
    modes.  Observed worst ratios: forward 0.10 (tile64, offset 1e3, extent 5, unsorted, linear / sum)."""
    for srt in (True, False):
        case = kc.offset_case(route, offset, ext, srt)
        for mode in kc.MODES:
            check(device, ("offset", route, offset, ext, srt), case, route, mode)


@pytest.mark.parametrize("route", ["tile32", "tile64", "simple48"])
@pytest.mark.parametrize("kmax", kc.ROW_WIDTHS)
def test_row_widths(device, route, kmax):
    """Rows of 1 .. 129 columns: one, two and three staging passes of 64.  Sorted rows (fill 0.9: the columns right
    behind a boundary are mostly shadow) and unsorted rows (real neighbours in the last column).  Forward in all six
    modes; backward (weighted features with the `*dst + v` second pass, d x, d W) at 64, 65 and 129.
    Observed worst ratios: forward 0.16 (simple48, kmax 129, constant / sum), d x 0.014, d W 0.029."""
    for srt in (True, False):
        case = kc.width_case(route, kmax, srt)
        for mode in kc.MODES:
            check(device, ("width", route, kmax, srt), case, route, mode, backward=kmax in kc.BACKWARD_WIDTHS)


@pytest.mark.parametrize("route", list(kc.ROUTES))
@pytest.mark.parametrize("nq", kc.QUERY_COUNTS)
def test_query_counts(device, route, nq):
    """Query counts around the 32-query tile and the 4-query aux workgroup, forward and backward, all six modes; nq 33
    and 65 leave one live row in the last tile and in the last aux workgroup.
    Observed worst ratios: forward 0.12 (tile128x256, constant / sum), d x 0.024, d W 0.017."""
    for srt in (True, False):
        case = kc.count_case(route, nq, srt)
        for mode in kc.MODES:
            check(device, ("count", route, nq, srt), case, route, mode, backward=True)


@pytest.mark.parametrize("route", ["tile32", "tile64", "simple48"])
def test_odd_staged_neighbour_counts(device, route):
    """Rows with exactly 1, 3, 7, 9 valid entries: at 32-channel chunks the half-waves take the even and the odd staged
    neighbours, the last even one has no partner.  Observed worst ratios: forward 0.06, d x 0.013, d W 0.009."""
    case = kc.odd_valid_case(route)
    counts = kc.valid_counts(case).tolist()
    assert set(counts) == {0, 1, 3, 7, 9} and all(counts.count(c) >= 9 for c in kc.ODD_COUNTS)
    for mode in kc.MODES:
        out = check(device, ("odd", route), case, route, mode, backward=True)
        assert float(out[3].abs().max()) == 0.0


@pytest.mark.parametrize("route", list(kc.ROUTES))
@pytest.mark.parametrize("offset,ext", [(0.0, 0.0625), (1e2, 0.0625), (1e3, 0.25)])
def test_exact_geometry(device, route, offset, ext):
    """Neighbours exactly on a kernel point, exactly at the extent, one float32 step inside / outside it.
      linear: on kernel point p the influence is exactly 1 (float64), compared at the bound in both aggregations;
      linear / sum with centre-only weights: the row AT the extent and the one outside are EXACTLY 0;
      closest with weights on ONE kernel point only: every single-neighbour row whose nearest point is another one is
        EXACTLY 0, in every influence;
      constant / sum: the row is the plain sum  (sum_k x_k) (sum_p W_p) / count;
      gaussian: compared at the bound.
    Observed worst ratio 0.10 (tile128x256, offset 1e3, gaussian / sum); the exact rows are exactly 0 on every route."""
    case, names = kc.exact_case(route, offset, ext)
    n_kp, cout = case["kp"].shape[0], case["w"].shape[2]
    key = ("exact", route, offset, ext)
    for mode in kc.MODES:
        check(device, key, case, route, mode)
    infl = kc.influences_64(case, 'linear')
    for p in range(1, min(n_kp, 15)):
        assert float(infl[names["on_kp"][p - 1], 0, p]) == 1.0
    # centre-only weights
    w0 = torch.zeros_like(case["w"])
    w0[0] = case["w"][0]
    c0 = dict(case, w=w0)
    y0 = check(device, key + ("w0",), c0, route, ('linear', 'sum')).cpu()
    for r in ("at_extent", "outside"):
        print(f"exact {route} offset {offset:g}: max |out| of the {r} row {float(y0[names[r]].abs().max()):.3e}")
        assert torch.equal(y0[names[r]], torch.zeros(cout)), f"{route}: centre influence {r} is not exactly 0"
    assert bool((y0[names["inside"]] != 0).any())
    # closest, weights on one kernel point only: rows 0..17 hold ONE neighbour each
    d2, _ = kc._d2_64(case)
    nearest = torch.argmin(d2[:18, 0, :], 1)
    for p_only in (0, min(3, n_kp - 1)):
        wp = torch.zeros_like(case["w"])
        wp[p_only] = case["w"][p_only]
        cp = dict(case, w=wp)
        for influence in kc.INFLUENCES:
            y = check(device, key + ("only", p_only), cp, route, (influence, 'closest')).cpu()
            others = torch.nonzero(nearest != p_only).flatten()
            assert others.numel() >= 10
            assert torch.equal(y[others], torch.zeros(others.numel(), cout)), f"{route} {influence}: another point's row is not 0"
            if influence == 'constant':
                mine = torch.nonzero(nearest == p_only).flatten()
                assert mine.numel() >= 1 and bool((y[mine].abs().max(1)[0] > 0).all())
    # constant / sum: the plain sum
    idx = case["idx"].long()
    ns = case["s"].shape[0]
    valid = (idx >= 0) & (idx < ns)
    xs = (case["x"].double()[torch.where(valid, idx, torch.zeros_like(idx))] * valid.unsqueeze(2)).sum(1)
    plain = xs @ case["w"].double().sum(0) / kc.ref_counts(case).unsqueeze(1)
    yc = check(device, key, case, route, ('constant', 'sum'))
    _ratio(f"exact {route} constant-sum against the plain sum", yc, plain, FWD)


@pytest.mark.parametrize("route", list(kc.ROUTES))
def test_exact_argmin_ties(device, route):
    """Every real neighbour is equidistant, in exact float32 arithmetic, from kernel point 0 and from two to four
    others (asserted on the CPU).  torch.argmin takes the first; the kernels document "lowest p wins".  The weights
    differ by 0.25 p: another pick is an O(1) error.  Forward in the three closest modes (and, as the control, the
    three sum modes), d x and d W through KPConvModesFn.  Observed worst ratios: forward 0.13, d x 0.018, d W 0.015
    (with `<=` for `<` in the kernels' arg-min all eight routes fail, at errors of the output's own size)."""
    case = kc.tie_case(route)
    d2, valid = kc.d2_float32(case)
    items = d2[valid]
    assert np.all(items.min(1) == items[:, 0]) and np.all((items == items[:, :1]).sum(1) >= 3)
    assert not bool(kc.near_tie_rows(case).any())
    for mode in kc.MODES:
        check(device, ("tie", route), case, route, mode, backward=True)


@pytest.mark.parametrize("route", list(kc.ROUTES))
def test_neighbour_count_edges(device, route):
    """Integer features (a row sum is exact in any order): support rows summing to exactly 0 and to -1, queries that
    see only those (the count clamps at 1), an all-shadow row; every mode, forward and the cnt of weighted_features.
    Observed worst ratio 0.10 (tile128x256, gaussian / sum); the counts are equal."""
    case = kc.count_edge_case(route)
    cnt_ref = kc.ref_counts(case)
    assert bool((cnt_ref[5:25] == 1).all()) and int(cnt_ref.max()) > 1
    d = _dev(case, device)
    for mode in kc.MODES:
        out = check(device, ("edges", route), case, route, mode)
        assert float(out[3].abs().max()) == 0.0
        if case["kp"].shape[0] <= kc.AUX_KP_MAX:
            _, cnt = kpconv_modes.weighted_features(d["q"], d["s"], d["idx"], d["x"], d["kp"], d["extent"],
                                                    *kpconv_modes.mode_codes(*mode))
            assert torch.equal(cnt.cpu().double(), cnt_ref.double()), f"{route} {mode}: counts"


@pytest.mark.parametrize("mode", kc.MODES, ids=lambda m: "-".join(m))
def test_seventeen_kernel_points_run_forward_and_refuse_the_backward(device, mode):
    """spr_kpconv_modes_fwd takes up to 32 kernel points (the one-thread-per-output kernel), the backward kernels 16:
    n_kp 17 computes forward against float64, and its backward raises the operator's own error instead of returning
    gradients.  (n_kp 16, forward and backward, is route kp16 in every test of this module.)  Observed ratio 0.05."""
    case = kc.cloud_case("impl1", 33, 120, 12, 1e2, 0.125, 49, n_kp=17)
    assert case["w"].shape[0] == 17 == kc.AUX_KP_MAX + 1 <= kc.FWD_KP_MAX
    for impl_route in ("tile32", "impl1"):               # impl 0 at a tile shape: 17 points leave the tile kernel
        check(device, ("kp17",), case, impl_route, mode, what=f"kp17 impl {kc.ROUTES[impl_route][0]} {mode}")
    d = _dev(case, device)
    x, w = d["x"].requires_grad_(True), d["w"].requires_grad_(True)
    y = _run(dict(d, x=x, w=w), mode, 0)
    with pytest.raises(RuntimeError, match="kpconv_modes_weighted_features"):
        y.backward(torch.ones_like(y))
    assert x.grad is None and w.grad is None
    with pytest.raises(RuntimeError, match="kpconv_modes_bwd_dx"):
        kpconv_modes.bwd_dx(d["q"], d["s"], d["idx"], 32, d["kp"], d["extent"], *kpconv_modes.mode_codes(*mode),
                            torch.zeros((33, 17 * 32), device=device))
    w33 = torch.zeros((33, 32, 32), device=device)
    with pytest.raises(RuntimeError, match="kpconv_modes"):
        kpconv_modes.kpconv_raw(d["q"], d["s"], d["idx"], d["x"], w33, torch.zeros((33, 3), device=device), d["extent"],
                                *kpconv_modes.mode_codes(*mode))


@pytest.mark.parametrize("route", ["tile32", "tile64", "simple48"])
def test_influence_underflow(device, route):
    """An extent of 2^-10 under a cloud spaced ~0.05: every Gaussian influence underflows float32, every linear one is
    0 (asserted on the float64 values).  The output is finite with |out| <= 1e-30, linear is exactly 0, constant / sum
    still matches float64, and the counts of weighted_features are the reference's.  With every neighbour 16 extents
    away all kernel points are nearly equidistant: the case is over the near-tie cap by construction (10 of 32 live
    rows, asserted on the host), so no closest mode is compared strictly here -- linear and gaussian / closest must be
    0 whatever the pick, constant / closest must be finite.  Observed: max |out| exactly 0 in the four linear /
    gaussian modes on every route; constant / sum 0.07 of its bound."""
    case = kc.underflow_case(route)
    assert float(kc.influences_64(case, 'gaussian').max()) < 2.0 ** -150
    assert float(kc.influences_64(case, 'linear').max()) == 0.0
    cnt_ref = kc.ref_counts(case)
    assert int(cnt_ref.max()) > 3
    d = _dev(case, device)
    impl = kc.ROUTES[route][0]
    for mode in kc.MODES:
        if mode == ('constant', 'sum'):
            check(device, ("underflow", route), case, route, mode)
        else:
            with torch.no_grad():
                out = _run(d, mode, impl).cpu()
            m = float(out.abs().max())
            print(f"underflow {route} {mode}: max |out| {m:.3e}")
            assert bool(torch.isfinite(out).all()) and (mode[0] == 'constant' or m <= 1e-30)
            if mode[0] == 'linear':
                assert m == 0.0
        wf, cnt = kpconv_modes.weighted_features(d["q"], d["s"], d["idx"], d["x"], d["kp"], d["extent"],
                                                 *kpconv_modes.mode_codes(*mode))
        assert torch.equal(cnt.cpu().double(), cnt_ref.double()) and bool(torch.isfinite(wf).all())
        if mode[0] != 'constant':
            assert float(wf.abs().max()) <= 1e-30


# ---- 2. operand magnitudes of the tile kernel ---------------------------------------------------------------------------------
def _published(x, device):
    """x on the device as a producer's output: ops.instnorm(norm=False, slope=1) copies it exactly and publishes its
    range."""
    xd = x.to(device)
    y = ops.instnorm(xd, ops.lengths_to_cu([x.shape[0]], device), norm=False, slope=1.0)
    assert torch.equal(y, xd) and ops._get_range(y)[0] is not None
    return y


def _magnitude_check(device, key, case, route, mode, what):
    """Forward and backward with x as a plain tensor (range measured in the call) and as a producer's output (range
    published), each against float64."""
    strict, go, ref, dx_ref, dw_ref = _ref(key, case, mode, True)
    outs = []
    for published in (False, True):
        d = _dev(case, device)
        if published:
            d["x"] = _published(case["x"], device)
        assert (ops._get_range(d["x"])[0] is not None) == published
        x, w = d["x"].requires_grad_(True), d["w"].requires_grad_(True)
        assert (ops._get_range(x)[0] is not None) == published
        y = _run(dict(d, x=x, w=w), mode, 0)
        tag = f"{what} {'published' if published else 'measured'}"
        _ratio(tag, y, ref, FWD, strict)
        y.backward(go.to(device))
        _ratio(tag + " dx", x.grad, dx_ref, BWD)
        _ratio(tag + " dW", w.grad, dw_ref, BWD)
        outs.append(y.detach())
    return outs


@pytest.mark.parametrize("mode", kc.MAG_MODES, ids=lambda m: "-".join(m))
@pytest.mark.parametrize("route", kc.MAG_ROUTES)
def test_operand_scales(device, route, mode):
    """x scaled by 2^-20, 1, 2^13 and W by 2^-10, 1, 2^7 (all nine pairs): the criterion is relative to the output's
    scale and the scales are powers of two, so the float64 reference is the scaled reference and the bound is the same.
    Observed worst ratios: forward 0.12, d x 0.009, d W 0.011 -- the same at every pair of scales."""
    base = kc.magnitude_case(route)
    for sx in kc.X_SCALES:
        for sw in kc.W_SCALES:
            case = dict(base, x=base["x"] * sx, w=base["w"] * sw)
            _magnitude_check(device, ("mag", route, sx, sw), case, route, mode, f"scales {route} {mode} x*{sx:g} W*{sw:g}")


@pytest.mark.parametrize("mode", kc.MAG_MODES, ids=lambda m: "-".join(m))
@pytest.mark.parametrize("route", kc.MAG_ROUTES)
def test_mixed_magnitudes_and_power_of_two_edges(device, route, mode):
    """One tensor whose halves differ by 2^12; then kmax * max|x| exactly 2^6 and one float32 step below / above it,
    where pow2_exp_for's exponent changes.  (The weighted features of these random-sign tensors stay far below that
    bound: test_operand_bound_is_reached is the case in which a wrong exponent overflows.)
    Observed worst ratios: mixed forward 0.07, d x 0.009, d W 0.014; edges forward 0.10, d x 0.009, d W 0.012."""
    base = kc.magnitude_case(route)
    _magnitude_check(device, ("mixed", route), dict(base, x=kc.mixed_x(base["x"])), route, mode, f"mixed {route} {mode}")
    for edge in kc.POW2_EDGES:
        case = dict(base, x=kc.pow2_edge_x(base["x"], edge))
        _magnitude_check(device, ("pow2", route, edge), case, route, mode, f"pow2 {edge} {route} {mode}")


@pytest.mark.parametrize("edge", kc.POW2_EDGES)
@pytest.mark.parametrize("route", kc.MAG_ROUTES)
def test_operand_bound_is_reached(device, route, edge):
    """Equal features in full rows: in constant / sum every weighted-feature sum of a live row equals kmax * max|x|, the
    bound the tile kernel scales its split-fp16 operand by (asserted on the host), at 2^6 and one float32 step either
    side.  An exponent one too large puts the operands at 2^16 - where fp16 ends - in the `below` case; gaussian / sum
    runs beside it on the same tensor.  Observed worst ratios: forward 0.07, d x 0.010, d W 0.011; with `+ 1` on the
    operand exponent both `below` cases fail and no other test of this section does."""
    case = kc.saturating_case(route, edge)
    for mode in (('constant', 'sum'), ('gaussian', 'sum')):
        _magnitude_check(device, ("saturating", route, edge), case, route, mode, f"saturating {edge} {route} {mode}")


@pytest.mark.parametrize("mode", kc.MAG_MODES, ids=lambda m: "-".join(m))
@pytest.mark.parametrize("route", kc.MAG_ROUTES)
def test_weight_planes_fresh_cached_and_edited(device, route, mode):
    """Fresh weights (planes built in the call) and re-used weights (the cached planes) give the same bits; after
    w.mul_(2) the cache is stale, the planes are rebuilt and the output doubles exactly (a power of two moves only the
    weight scale's exponent)."""
    d = _dev(kc.magnitude_case(route), device)
    with torch.no_grad():
        first = _run(d, mode, 0)
        assert getattr(d["w"], "_spr_kp_wplanes", None) is not None, "the call kept no planes on the weights"
        planes = d["w"]._spr_kp_wplanes[1]
        again = _run(d, mode, 0)
        assert d["w"]._spr_kp_wplanes[1] is planes, "the second call rebuilt the planes"
        fresh = _run(dict(d, w=d["w"].clone()), mode, 0)
        assert torch.equal(first, again) and torch.equal(first, fresh)
        d["w"].mul_(2)
        doubled = _run(d, mode, 0)
        assert d["w"]._spr_kp_wplanes[1] is not planes
    assert float(first.abs().max()) > 0 and torch.equal(doubled, first * 2)
