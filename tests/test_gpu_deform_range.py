"""GPU: deformable / modulated KPConv (csrc/kpconv_deform.hip: the fused tile forward at 32- and 64-channel chunks, the
one-thread forward, min_d2, the weighted-features / d x kernel, the offset-gradient kernel) and its regulariser
(csrc/deform_reg.hip) at the geometry, shape and magnitude edges the rigid routes are held to by
tests/test_gpu_kpconv_modes_range.py: KITTI-like offsets, row widths around the 64-column staging chunk (with rows whose
first chunk stages nothing and rows that stage all 64 slots), query counts around the 32-query tile and beyond the tile
kernel's grid, fully cut rows, odd in-range counts, negative feature sums, repeated and negative indices, offset and
modulation magnitudes, items exactly on a kernel point, kernel-point counts 1 .. 16, operand magnitudes and ranges of the
split-fp16 tile kernel and of the fixed-point d x scatter.  Inputs and their conditions: tests/deform_range_cases.py,
checked without a GPU by tests/test_deform_range_host.py.

Reference: deform_cases.kpconv_deform_ref / deform_reg_cases.reg_ref in float64, differentiated by autograd; where an
item sits exactly on a kernel point, deform_range_cases.guarded_ref (h = 1, no positional gradient there).  The kernels
are handed the float32-rounded offsets of the float64 offset convolution.  Bounds, the modules' own, relative to the
reference's largest magnitude: forward 1e-5; d x, d W, d offset_features 2e-5; sqrt(min_d2) within 1e-5 of the extent on
rows with a real neighbour; the regulariser's fit, rep and d offset_features 1e-5.  Every check asserts the input
conditions first; nothing is excluded from any comparison.

Observed worst err / bound ratios are written next to each check.  What these tests see that the feature tests
(test_gpu_deform*.py, test_gpu_deform_reg*.py) do not, each tried on a scratch build:
    the tile kernel's operand scale from kmax instead of 2 kmax      test_operand_bound_is_reached[*-below] fails
    lcnt[] not rewritten on the tile loop's second trip               test_more_tiles_than_the_grid fails
    k_deform_reg_final stepping by 512                                test_regulariser_more_than_256_workgroups fails
    `dist >= 0` in the offset kernel (0 / 0 at d2 == 0)               test_items_exactly_on_a_kernel_point and
                                                                      test_operand_bound_is_reached fail
with the feature tests passing in all four.  Two more are seen by both: `acc[p]` for `*dst + acc[p]` in the weighted
features (here test_row_widths_backward at 65 and 129; there the 70-column case) and `m` for `m (1 - m / 2)` in d logit
(every modulated backward)."""
import pytest
import torch

import deform_cases as dc
import deform_range_cases as drc
import deform_reg_cases as rc
import kpconv_modes_cases as kc
from superpoints_registration_amd import deform_reg, deformable, ops, synthetic
from test_gpu_kpconv_modes import arithmetic  # noqa: F401  (the fixture: default / split-fp16 / exact-f32)

pytestmark = pytest.mark.gpu
FWD, BWD, REG = 1e-5, 2e-5, 1e-5
MOD, mod_id = drc.MOD, drc.mod_id


def _dev(case, device):
    return {k: (v.clone().to(device) if isinstance(v, torch.Tensor) else v) for k, v in case.items()}


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def _ratio(what, got, ref, bound, scale=None):
    """err / (bound * scale), printed; everything finite.  scale: the reference's largest magnitude unless given."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    scale = float(ref.abs().max()) if scale is None else scale
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    ratio = err / max(bound * scale, 1e-300)
    print(f"{what}: err {err:.3e} scale {scale:.3e} ratio {ratio:.3f}")
    assert scale > 0, f"{what}: a vacuous case"
    assert err <= bound * scale, f"{what}: {err:.3e} > {bound:g} * {scale:.3e}"
    return ratio


def _forward(d, of, want_min_d2=False):
    impl = drc.ROUTES[d["route"]][0]
    return deformable.kpconv_deform(d["q"], d["s"], d["idx"], d["x"], d["w"], d["kp"], d["extent"], of, d["modulated"],
                                    impl=impl, want_min_d2=want_min_d2)


def _grads(d, of, go):
    x, w, of = (t.detach().clone().requires_grad_(True) for t in (d["x"], d["w"], of))
    y = _forward(dict(d, x=x, w=w), of)
    y.backward(go)
    return y.detach(), dict(dx=x.grad, dw=w.grad, d_of=of.grad)


def check(device, what, case, zeros=False, forward=True, backward=False, x_scale=1.0, go_scale=1.0, of=None):
    """One case against float64: the conditions, then the forward (with min_d2 and the in-range counts) and / or d x, d W
    and d offset_features through KPConvDeformFn.  of: the device tensor handed over as the offsets (a view of
    case['of'] otherwise).  Returns (out, grads, aux)."""
    go = synthetic.rand((case["q"].shape[0], case["w"].shape[2]), 77) * go_scale if backward else None
    ref, aux, gref = drc.ref64(case, go, guarded=zeros)
    drc.check_conditions(case, aux, zeros, x_scale)
    d = _dev(case, device)
    of = d["of"] if of is None else of
    out = grads = None
    if forward:
        with torch.no_grad():
            out, min_d2 = _forward(d, of, want_min_d2=True)
            _, cnt = deformable.weighted_features(d["q"], d["s"], d["idx"], d["x"], d["kp"], d["extent"], of)
        _ratio(what, out, ref, FWD)
        real = aux["valid"].any(1)
        if bool(real.any()):
            _ratio(what + " sqrt(min_d2)", min_d2.double().cpu()[real].sqrt(), aux["min_d2"][real].sqrt(), FWD,
                   scale=case["extent"])
        assert torch.equal(cnt.cpu().long(), aux["count"]), f"{what}: the in-range counts differ from the float64 counts"
    if backward:
        y, grads = _grads(d, of, go.to(device))
        if forward:
            assert torch.equal(y, out), f"{what}: the differentiable call gives other bits"
        for k in ("dx", "dw", "d_of"):
            _ratio(f"{what} {k}", grads[k], gref[k], BWD)
    return out, grads, aux


def test_routes_are_what_they_name():
    for name, (impl, cin, cout, n_kp) in drc.ROUTES.items():
        assert drc.deform_route(impl, cin, cout, n_kp) == drc.ROUTE_KERNEL[name], name


# ---- 1. offset coordinates -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", drc.FWD_ROUTES)
@pytest.mark.parametrize("offset,ext", kc.OFFSETS)
def test_offset_coordinates(device, route, offset, ext):
    """KITTI-like geometry: coordinates of 1e2 / 1e3, extents 0.03 .. 5, sorted and unsorted rows, modulated off and on.
    Observed worst ratios: forward 0.07 (tile64, offset 1e2, extent 0.6, sorted, plain), sqrt(min_d2) 0.03."""
    for srt in (True, False):
        for mod in MOD:
            name = drc.offset_name(route, offset, ext, srt, mod)
            check(device, name, drc.get(name))


@pytest.mark.parametrize("route", drc.BWD_ROUTES)
@pytest.mark.parametrize("offset,ext", kc.OFFSETS)
def test_offset_coordinates_backward(device, arithmetic, route, offset, ext):
    """Observed worst ratios: d x 0.02, d W 0.04, d offset_features 0.02."""
    for srt in (True, False):
        for mod in MOD:
            name = drc.offset_name(route, offset, ext, srt, mod)
            check(device, f"{name} {arithmetic}", drc.get(name), forward=False, backward=True)


# ---- 2. row widths -----------------------------------------------------------------------------------------------------------
def _width_names(route, kmax, mod):
    variants = drc.WIDTH_VARIANTS + (drc.WIDE_VARIANTS if kmax == 129 else ())
    return [drc.width_name(route, kmax, v, mod) for v in variants]


@pytest.mark.parametrize("route", ("tile32", "tile64", "simple48"))
@pytest.mark.parametrize("kmax", drc.DEFORM_WIDTHS)
def test_row_widths(device, route, kmax):
    """Rows of 1 .. 129 columns: one, two and three staging passes of 64.  Sorted rows (fill 0.9) and rows in random
    column order (in-range neighbours in every chunk); at 129 also rows whose first 64 columns are valid but out of range
    (the pass stages nothing) and rows under an extent that stages all 64 slots of a pass.
    Observed worst ratios: forward 0.31 and sqrt(min_d2) 0.23, both in the late-chunk rows (a single in-range neighbour
    sets the output's scale; the kernel points sit several extents from the query)."""
    for mod in MOD:
        for name in _width_names(route, kmax, mod):
            check(device, name, drc.get(name))


@pytest.mark.parametrize("route", drc.BWD_ROUTES)
@pytest.mark.parametrize("kmax", kc.BACKWARD_WIDTHS)
def test_row_widths_backward(device, arithmetic, route, kmax):
    """The weighted features' second and third pass (`*dst + acc`, after a first pass that stored zeros in the late-chunk
    rows), the offset kernel's skipped chunks, the scatter.  Observed worst ratios: d x 0.16, d W 0.04,
    d offset_features 0.15 (all three in the late-chunk rows)."""
    for mod in MOD:
        for name in _width_names(route, kmax, mod):
            check(device, f"{name} {arithmetic}", drc.get(name), forward=False, backward=True)


# ---- 3. query counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", drc.FWD_ROUTES)
@pytest.mark.parametrize("nq", kc.QUERY_COUNTS)
def test_query_counts(device, route, nq):
    """Query counts around the 32-query tile and the 4-query workgroups of the backward kernels.
    Observed worst ratios: forward 0.08, sqrt(min_d2) 0.02."""
    for mod in MOD:
        name = drc.count_name(route, nq, mod)
        check(device, name, drc.get(name))


@pytest.mark.parametrize("route", drc.BWD_ROUTES)
@pytest.mark.parametrize("nq", kc.QUERY_COUNTS)
def test_query_counts_backward(device, arithmetic, route, nq):
    """Observed worst ratios: d x 0.02, d W 0.02, d offset_features 0.02."""
    for mod in MOD:
        name = drc.count_name(route, nq, mod)
        check(device, f"{name} {arithmetic}", drc.get(name), forward=False, backward=True)


@pytest.mark.parametrize("route", drc.TILE_ROUTES)
def test_more_tiles_than_the_grid(device, route):
    """nq = 32 * (compute units * residency) + 33: every workgroup of the capped grid takes its tile, workgroup 0 a full
    second one (lcnt[] rewritten behind the barrier, first[] reloaded) and workgroup 1 a tile of one live row.  Every row
    is compared like all the others; the second trip's rows are reported on their own.
    Observed worst ratios: forward 0.06, second-trip rows 0.03."""
    n_cu = torch.cuda.get_device_properties(device).multi_processor_count
    cc = 64 if drc.ROUTES[route][1] % 64 == 0 else 32
    case = drc.get_grid(route, n_cu)
    nq = case["q"].shape[0]
    first_trip = 32 * n_cu * drc.residency(cc)
    assert nq == first_trip + 33 and -(-nq // 32) > n_cu * drc.residency(cc)
    out, _, aux = check(device, f"grid {route} nq {nq}", case)
    ref = drc.ref64(case)[0]
    assert float(ref[first_trip:].abs().max()) > 0
    _ratio(f"grid {route} second-trip rows", out[first_trip:], ref[first_trip:], FWD, scale=float(ref.abs().max()))
    with torch.no_grad():
        again = _forward(_dev(case, device), case["of"].to(device))
    assert torch.equal(out, again), "two runs differ"


# ---- 4. in-range edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", drc.FWD_ROUTES)
def test_in_range_edges(device, route):
    """Rows whose valid neighbours are all cut (output exactly 0); rows with exactly 1, 3, 7, 9 in-range neighbours between
    out-of-range ones (the half-wave walk of the 32-channel tile kernel); rows whose in-range neighbours all have a
    negative feature sum (numerator live, count 1); a neighbour index three times in a row; shadow entries written as -1,
    ns and ns + 5.  Observed worst ratios: forward 0.08 (odd, tile64); sqrt(min_d2) 0.45 in the cut rows, whose kernel
    points sit 69 extents from the query (a float32 step of that distance is 4e-6 extents)."""
    for mod in MOD:
        name = drc.edge_name("cut", route, mod)
        out, _, aux = check(device, name, drc.get(name))
        assert float(out[drc.CUT_ROWS].abs().max()) == 0.0, "a fully cut row is not exactly 0"
        for kind in ("odd", "edges"):
            name = drc.edge_name(kind, route, mod)
            check(device, name, drc.get(name))


@pytest.mark.parametrize("route", drc.BWD_ROUTES)
def test_in_range_edges_backward(device, arithmetic, route):
    """A fully cut row's d offset_features row is exactly 0 and it adds nothing to d x: the cut rows ALONE give d x == 0
    everywhere.  Observed worst ratios: d x 0.02, d W 0.03, d offset_features 0.02."""
    for mod in MOD:
        name = drc.edge_name("cut", route, mod)
        case = drc.get(name)
        _, g, _ = check(device, f"{name} {arithmetic}", case, forward=False, backward=True)
        assert float(g["d_of"][drc.CUT_ROWS].abs().max()) == 0.0
        d = _dev(case, device)
        rows = torch.tensor(drc.CUT_ROWS, device=device)
        alone = dict(d, q=d["q"][rows].contiguous(), idx=d["idx"][rows].contiguous())
        y, g = _grads(alone, d["of"][rows].contiguous(), torch.ones((rows.numel(), case["w"].shape[2]), device=device))
        for k, v in dict(g, out=y).items():
            assert float(v.abs().max()) == 0.0, f"{name}: {k} of the cut rows alone is not exactly 0"
        for kind in ("odd", "edges"):
            name = drc.edge_name(kind, route, mod)
            check(device, f"{name} {arithmetic}", drc.get(name), forward=False, backward=True)


# ---- 5. offset and modulation magnitudes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", drc.FWD_ROUTES)
def test_offset_magnitudes(device, route):
    """Offset features scaled by 2^-20, 1, 8 and 32.  Observed worst ratios: forward 0.06, sqrt(min_d2) 0.05."""
    for mod in MOD:
        for sc in drc.OF_SCALES:
            name = drc.edge_name(f"of*{sc:g}", route, mod)
            check(device, name, drc.get(name))


@pytest.mark.parametrize("route", drc.BWD_ROUTES)
def test_offset_magnitudes_backward(device, arithmetic, route):
    """Observed worst ratios: d x 0.01, d W 0.02, d offset_features 0.02."""
    for mod in MOD:
        for sc in drc.OF_SCALES:
            name = drc.edge_name(f"of*{sc:g}", route, mod)
            check(device, f"{name} {arithmetic}", drc.get(name), forward=False, backward=True)


@pytest.mark.parametrize("route", drc.FWD_ROUTES)
def test_modulation_logits(device, arithmetic, route):
    """Logits of 0, +-20 and +-90: expf overflows at -(-90), m is exactly 0 or 2 (asserted on the host in float32
    arithmetic) and m (1 - m / 2) cancels.  Everything is finite; d logit is compared on its own, at 2e-5 of the whole
    gradient's scale, and is exactly 0 where the logit is +-90.
    Observed worst ratios: forward 0.04, d offset_features 0.02, d logit 0.002."""
    name = drc.edge_name("logits", route, True)
    case = drc.get(name)
    K = case["kp"].shape[0]
    go = synthetic.rand((case["q"].shape[0], case["w"].shape[2]), 77)
    _, g, _ = check(device, f"{name} {arithmetic}", case, backward=True)
    ref = drc.ref64(case, go)[2]["d_of"]
    _ratio(f"{name} d logit", g["d_of"][:, 3 * K:], ref[:, 3 * K:], BWD, scale=float(ref.abs().max()))
    assert float(ref[:, 3 * K:].abs().max()) > 1e-3 * float(ref.abs().max())
    sat = (case["of"][:, 3 * K:].abs() == 90).to(device)
    assert float(g["d_of"][:, 3 * K:][sat].abs().max()) == 0.0


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
@pytest.mark.parametrize("route", ("tile32", "tile64", "simple48"))
def test_offsets_as_a_column_slice_between_nan(device, route, modulated):
    """The offsets as a column slice of a wider matrix whose other columns are NaN -- for modulated=False these are the K
    columns where logits would sit.  The forward (the slice reaches the kernel when no gradient is asked for) is compared
    with float64; the forward and the three backward kernels, called directly, give the bits of the contiguous call."""
    name = drc.edge_name("of*1", route, modulated)
    case = drc.get(name)
    K, od, nq, cin = case["kp"].shape[0], case["of"].shape[1], case["q"].shape[0], case["x"].shape[1]
    wide = torch.full((nq, 4 * K + 5), float("nan"), device=device)
    wide[:, :od] = case["of"].to(device)
    view = wide[:, :od]
    assert view.stride(0) == 4 * K + 5 and bool(torch.isnan(wide[:, od:]).all()) and od in (3 * K, 4 * K)
    out, _, _ = check(device, name + " sliced", case, of=view)
    d = _dev(case, device)
    dwfm = synthetic.rand((nq, K * cin), 78).to(device)
    geo = (d["q"], d["s"], d["idx"])
    with torch.no_grad():
        assert torch.equal(bits(out), bits(_forward(d, d["of"])))
        for of in (view, d["of"]):
            wf, cnt = deformable.weighted_features(*geo, d["x"], d["kp"], d["extent"], of)
            dx = deformable.bwd_dx(*geo, cin, d["kp"], d["extent"], of, modulated, dwfm)
            d_of = deformable.bwd_offsets(*geo, d["x"], d["kp"], d["extent"], of, modulated, dwfm)
            got = (wf, cnt, dx, d_of)
            assert all(bool(torch.isfinite(t).all()) for t in got) and float(d_of.abs().max()) > 0
            if of is view:
                sliced = got
        for a, b in zip(sliced, got):
            assert torch.equal(bits(a), bits(b)), "the sliced offsets give other bits"


# ---- 6. d2 == 0 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ("tile32", "tile64", "simple48"))
def test_items_exactly_on_a_kernel_point(device, arithmetic, route):
    """A same-level block with zero offsets at kernel point 0 (kp[0] == 0): every query is its own neighbour at d2 == 0
    exactly, the other kernel points are deformed.  Forward within the bound; d offset_features finite and within the
    bound of the guarded float64 restatement (the item contributes its influence 1 to d logit and nothing to the
    positional gradient), modulation included; two runs give the same bits.
    Observed worst ratios: forward 0.08, d x 0.02, d W 0.02, d offset_features 0.02."""
    for mod in MOD:
        name = drc.edge_name("zero", route, mod)
        case = drc.get(name)
        out, g, _ = check(device, f"{name} {arithmetic}", case, zeros=True, backward=True)
        out2, g2, _ = check(device, f"{name} {arithmetic} again", case, zeros=True, backward=True)
        assert torch.equal(bits(out), bits(out2))
        for k in g:
            assert torch.equal(bits(g[k]), bits(g2[k])), f"two runs differ in {k}"


# ---- 7. kernel-point counts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ("kp1", "kp7", "kp16"))
def test_kernel_point_counts(device, arithmetic, route):
    """1, 7 and 16 (kKPmax) kernel points: the one-thread forward and all three backward kernels.
    Observed worst ratios: forward 0.03, d x 0.01, d W 0.01, d offset_features 0.02."""
    for mod in MOD:
        name = drc.edge_name("points", route, mod)
        check(device, f"{name} {arithmetic}", drc.get(name), backward=True)


# ---- 8. operand magnitudes of the tile kernel, the scatter and the products ----------------------------------------------------
def _published(x, device):
    """x on the device as a producer's output: ops.instnorm(norm=False, slope=1) copies it exactly and publishes its
    range."""
    xd = x.to(device)
    y = ops.instnorm(xd, ops.lengths_to_cu([x.shape[0]], device), norm=False, slope=1.0)
    assert torch.equal(y, xd) and ops._get_range(y)[0] is not None
    return y


def _magnitude_check(device, what, case, zeros=False, x_scale=1.0, go_scale=1.0):
    """Forward and backward with x as a plain tensor (range measured in the call) and as a producer's output (range
    published), each against float64."""
    go = synthetic.rand((case["q"].shape[0], case["w"].shape[2]), 77) * go_scale
    ref, aux, gref = drc.ref64(case, go, guarded=zeros)
    drc.check_conditions(case, aux, zeros, x_scale)
    for published in (False, True):
        d = _dev(case, device)
        if published:
            d["x"] = _published(case["x"], device)
        assert (ops._get_range(d["x"])[0] is not None) == published
        x, w, of = d["x"].requires_grad_(True), d["w"].requires_grad_(True), d["of"].requires_grad_(True)
        y = _forward(dict(d, x=x, w=w), of)
        tag = f"{what} {'published' if published else 'measured'}"
        _ratio(tag, y, ref, FWD)
        y.backward(go.to(device))
        for k, v in (("dx", x.grad), ("dw", w.grad), ("d_of", of.grad)):
            _ratio(f"{tag} {k}", v, gref[k], BWD)


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
@pytest.mark.parametrize("route", drc.TILE_ROUTES)
def test_operand_scales(device, route, modulated):
    """x scaled by 2^-20, 1, 2^13 and W by 2^-10, 1, 2^7 (all nine pairs) at kmax 16: powers of two, so the row-sum
    condition is the unscaled tensor's.  Observed worst ratios: forward 0.04, d x 0.01, d W 0.01,
    d offset_features 0.01 -- the same at every pair of scales."""
    base = drc.get(drc.edge_name("mag", route, modulated))
    for sx in kc.X_SCALES:
        for sw in kc.W_SCALES:
            case = dict(base, x=base["x"] * sx, w=base["w"] * sw)
            _magnitude_check(device, f"scales {route} {mod_id(modulated)} x*{sx:g} W*{sw:g}", case, x_scale=sx)


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
@pytest.mark.parametrize("route", drc.TILE_ROUTES)
def test_mixed_magnitudes_and_power_of_two_edges(device, route, modulated):
    """One tensor whose halves differ by 2^12; then 2 * kmax * max|x| exactly 2^7 and one float32 step below / above it,
    where pow2_exp_for's exponent changes.  Observed worst ratios: forward 0.05, d x 0.01,
    d W 0.01, d offset_features 0.02."""
    base = drc.get(drc.edge_name("mag", route, modulated))
    _magnitude_check(device, f"mixed {route} {mod_id(modulated)}", dict(base, x=kc.mixed_x(base["x"])))
    for edge in kc.POW2_EDGES:
        _magnitude_check(device, f"pow2 {edge} {route} {mod_id(modulated)}", dict(base, x=kc.pow2_edge_x(base["x"], edge)))


@pytest.mark.parametrize("edge", kc.POW2_EDGES)
@pytest.mark.parametrize("route", drc.TILE_ROUTES)
def test_operand_bound_is_reached(device, route, edge):
    """Rows of 16 copies of the query's own index, zero offset on kernel point 0, logit +90, constant features at 4 or one
    float32 step from it: wf[n, 0, :] IS 2 * kmax * max|x| (asserted on the host), the bound the tile kernel scales its
    split-fp16 operand by, at 2^7 and one step either side.  The items sit on kernel point 0 exactly: the guarded
    reference.  Observed worst ratios: forward 0.11 (tile64, below), d x 0.01, d W 0.01,
    d offset_features 0.01."""
    name = f"saturating {route} {edge}"
    _magnitude_check(device, name, drc.get(name), zeros=True)


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
@pytest.mark.parametrize("route", drc.TILE_ROUTES)
def test_output_gradient_scales(device, arithmetic, route, modulated):
    """The output gradient scaled by 2^-20, 1 and 2^13: the fixed-point scatter of d x (factor (modulated ? 2 : 1) n_kp
    times max |dWFm|) and the two products.  Observed worst ratios: d x 0.01, d W 0.02,
    d offset_features 0.01 -- the same at every scale."""
    case = drc.get(drc.edge_name("mag", route, modulated))
    for sg in drc.GO_SCALES:
        check(device, f"go*{sg:g} {route} {mod_id(modulated)} {arithmetic}", case, forward=False, backward=True, go_scale=sg)


# ---- the regulariser -----------------------------------------------------------------------------------------------------------
def _close(what, got, ref, bound=REG):
    got, ref = float(got), float(ref)
    assert got == got and abs(got) != float("inf"), f"{what}: not finite"
    ratio = abs(got - ref) / (bound * abs(ref)) if ref != 0 else (0.0 if got == 0 else float("inf"))
    print(f"{what}: {got:.8e} against {ref:.8e}, ratio {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: {got:.8e} against {ref:.8e}"
    return ratio


def _reg_run(d, of, repulse):
    of = of.detach().clone().requires_grad_(True)
    value, fit, rep = deform_reg.deform_reg(d["q"], d["s"], d["idx"], of, d["kp"], d["extent"], repulse)
    value.backward()
    return value.detach(), fit, rep, of.grad


def reg_check(device, name, repulse=rc.R_DEFAULT, case=None):
    """Value and gradient of one case against float64: the argmin gap first, then fit, rep, value and d offset_features;
    two runs give the same bits; the modulation columns' gradient is exactly 0."""
    case = drc.get(name, drc.REG_CASES) if case is None else case
    rc.check_gap(case, case["of"])
    ref = rc.ref64(case, repulse, offset_features=case["of"])
    d = _dev(case, device)
    value, fit, rep, d_of = _reg_run(d, d["of"], repulse)
    what = f"{name} R {repulse:g}"
    _close(what + " fit", fit, ref["fit"])
    _close(what + " rep", rep, ref["rep"])
    _close(what + " value", value, ref["value"])
    _ratio(what + " d_of", d_of, ref["d_of"], REG)
    K = case["kp"].shape[0]
    if case["modulated"]:
        assert float(d_of[:, 3 * K:].abs().max()) == 0.0
    for a, b in zip((value, fit, rep, d_of), _reg_run(d, d["of"], repulse)):
        assert torch.equal(bits(a), bits(b)), f"{what}: two runs differ"
    return value, fit, rep, d_of, ref


@pytest.mark.parametrize("offset,ext", kc.OFFSETS)
def test_regulariser_offset_coordinates(device, offset, ext):
    """Observed worst ratios: fit 0.01, rep 0.04, d offset_features 0.02."""
    for srt in (True, False):
        for mod in MOD:
            reg_check(device, f"reg offset {offset:g} {ext:g} {drc.srt_id(srt)} {mod_id(mod)}")


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
def test_regulariser_offset_magnitudes(device, modulated):
    """Observed worst ratios: fit 0.01, rep 0.07 (scale 32), d offset_features 0.02."""
    for sc in drc.OF_SCALES:
        reg_check(device, f"reg of*{sc:g} {mod_id(modulated)}")


@pytest.mark.parametrize("kmax", drc.REG_WIDTHS)
def test_regulariser_row_widths(device, kmax):
    """Rows around the 16-lane group: a lane loads the columns k = lane (mod 16).
    Observed worst ratios: fit 0.01, rep 0.03, d offset_features 0.03."""
    for mod in MOD:
        reg_check(device, f"reg width {kmax} {mod_id(mod)}")


@pytest.mark.parametrize("nq", drc.REG_COUNTS)
def test_regulariser_query_counts(device, nq):
    """Query counts around four per wave and 16 per workgroup.
    Observed worst ratios: fit 0.01, rep 0.03, d offset_features 0.03."""
    for mod in MOD:
        reg_check(device, f"reg count {nq} {mod_id(mod)}")


def test_regulariser_more_than_256_workgroups(device):
    """nq = 16 * 256 + 17: 258 partials, k_deform_reg_final's threads 0 and 1 take a second one.
    Observed worst ratios: fit 0.002, rep 0.02, d offset_features 0.02."""
    case = drc.get("reg many workgroups", drc.REG_CASES)
    assert -(-case["q"].shape[0] // 16) == 258
    reg_check(device, "reg many workgroups", case=case)


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
def test_regulariser_kernel_point_counts(device, modulated):
    """One kernel point: no pair, rep exactly 0 and the gradient is the fitting term's; 16: every lane of a group live.
    Observed worst ratios: fit 0.004, rep 0.03, d offset_features 0.02."""
    _, _, rep, _, _ = reg_check(device, f"reg points kp1 {mod_id(modulated)}")
    assert float(rep) == 0.0
    reg_check(device, f"reg points kp16 {mod_id(modulated)}")


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
def test_regulariser_repulse_extents(device, modulated):
    """repulse_extent 0: rep exactly 0 and its gradient exactly 0 -- with every row all shadow (no fitting term either) the
    whole gradient is exactly 0; 50: every pair of every query active (asserted on the host).
    Observed worst ratios: fit 0.002, rep 0.004, d offset_features 0.02."""
    name = f"reg of*8 {mod_id(modulated)}"
    _, _, rep, _, _ = reg_check(device, name, repulse=0.0)
    assert float(rep) == 0.0
    case = drc.get(name, drc.REG_CASES)
    d = _dev(case, device)
    value, fit, rep, d_of = _reg_run(dict(d, idx=torch.full_like(d["idx"], case["s"].shape[0])), d["of"], 0.0)
    assert float(value) == 0.0 and float(fit) == 0.0 and float(rep) == 0.0 and float(d_of.abs().max()) == 0.0
    _, _, rep, _, ref = reg_check(device, name, repulse=50.0)
    assert float(ref["rep"]) > 100.0


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
def test_regulariser_shadow_rows_and_single_neighbours(device, modulated):
    """Rows 8..15 all shadow (no fitting term: their gradient is the repulsive term's alone, bit for bit the row of a run
    in which EVERY row is all shadow), rows 16..23 a single real neighbour.
    Observed worst ratios: fit 0.002, rep 0.03, d offset_features 0.02."""
    name = f"reg rows {mod_id(modulated)}"
    _, _, rep, d_of, _ = reg_check(device, name)
    case = drc.get(name, drc.REG_CASES)
    d = _dev(case, device)
    _, fit0, rep0, d_rep = _reg_run(dict(d, idx=torch.full_like(d["idx"], case["s"].shape[0])), d["of"], rc.R_DEFAULT)
    assert float(fit0) == 0.0 and torch.equal(bits(rep0), bits(rep))
    assert torch.equal(bits(d_of[8:16]), bits(d_rep[8:16])) and not torch.equal(bits(d_of[16:24]), bits(d_rep[16:24]))
