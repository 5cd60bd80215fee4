"""GPU: the encoder stem spr_kpconv_stem (Cin = 1 KPConv + per-cloud InstanceNorm + LeakyReLU, csrc/kpconv.hip) and
the Cin = 1 gather of ops.kpconv_raw against float64 -- tests/test_gpu_stem.py holds the stem to the operator route
ops.kpconv -> ops.instnorm only, which shares its gather and its MFMA step.

Reference: forward_cases.kpconv_f64 -> forward_cases.instnorm_f64(slope=...), float64 on the float32 inputs.
Bound per cloud and channel:  |out - ref| <= 1e-5 max|raw_ref| rstd_ref + 2e-6 |ref|  -- KPConv's own 1e-5 of the raw
tensor's scale carried through the normalisation (a raw error e moves the normalised value by e rstd), plus the
InstanceNorm allowance of tests/test_gpu_forward_range.py.  Statistics (return_stats) against
forward_cases.instnorm_stats_f64 by the rule test_gpu_forward_range.py::test_instnorm_variants_bitwise applies to
ops.instnorm_stats: |mean - mean64| <= 2^-23 max|mean64|, |rstd - rstd64| <= 2e-6 rstd64, where mean64 / rstd64 are
the float64 statistics of the float32 tensor the statistics are taken of (there the input; here the raw KPConv rows,
which the stem does not write and ops.kpconv_raw does, with the same bits).  Held against the statistics of the
float64 raw tensor instead, that rule measures KPConv's float32 error, not the statistics passes': a one-row cloud's
mean IS its raw row (observed 2.04 times 2^-23 max|mean| on the first case).  That comparison is made too, with
KPConv's 1e-5 of the raw scale carried along (_stem_check, (b)).

Cases: the ragged batch STEM_LENGTHS of tests/test_gpu_stem.py crossed (a lean cross; each case names the path it
reaches) with kernel-point counts 1 / 7 / 15 / 16 (the sixteen influence slots: one used, partly used, one padded,
full), row widths 1 / 20 / 64 / 65 / 130 (one staged chunk of 64 index columns, exactly one, two, three), sorted rows
and unsorted rows with shadow and negative holes, output widths 16 / 32 / 128 (one, two, eight MFMA tiles), slope 0.2,
eps 1e-5 / 1e-3, int64 and strided index matrices; then degenerate clouds and weight scales.
Observed worst ratios: output 0.03 of its bound (the degenerate batch at W 2^-10; 0.002 on the ragged batch), mean 0.39
of 2^-23 max|mean| and rstd 0.03 of 2e-6 against the float32 rows' statistics, 0.014 / 0.026 against the float64 rows'
with the carried allowance; ops.kpconv_raw at 1 / 7 / 16 kernel points 0.03 of 1e-5 of its scale."""
import numpy as np
import pytest
import torch

import forward_cases as fc
from superpoints_registration_amd import ops, stem
from test_gpu_stem import EXT, STEM_LENGTHS, _check, _features

pytestmark = pytest.mark.gpu
T = torch.from_numpy
F64 = torch.float64
SLOPE = 0.2

# name -> (n_kp, kmax, sorted rows, cout, eps, index form); the path the case reaches is its name
STEM_CASES = {
    "one pass, 15 points padded to 16, two tiles": (15, 20, True, 32, 1e-5, "int32"),
    "one column, one kernel point, one tile": (1, 1, True, 16, 1e-5, "int32"),
    "one column with shadow entries, eight tiles": (15, 1, False, 128, 1e-5, "int32"),
    "exactly one staged chunk, unsorted holes, 7 points, eps 1e-3": (7, 64, False, 32, 1e-3, "int32"),
    "exactly one staged chunk, sorted, one tile, eps 1e-3": (15, 64, True, 16, 1e-3, "rowstride"),
    "two passes, sorted (waves stop early), 16 points, eight tiles, int64": (16, 65, True, 128, 1e-5, "int64"),
    "two passes, unsorted, one kernel point": (1, 65, False, 32, 1e-5, "int32"),
    "three passes, unsorted holes, 16 points, row stride": (16, 130, False, 16, 1e-5, "rowstride"),
    "three passes, sorted, 7 points, eight tiles, eps 1e-3": (7, 130, True, 128, 1e-3, "int32"),
    "one pass, unsorted holes, 16 points, column stride": (16, 20, False, 32, 1e-5, "colstride"),
}


def _holes(nb, ns, seed):
    """Shadow (= ns, > ns) and negative entries in the middle of the rows, as
    test_gpu_stem.py::test_cin1_gather_shadow_rows_and_holes plants them; column 0 is kept."""
    r = fc.rng_of(711, seed)
    hole = r.random(nb.shape) < 0.2
    hole[:, 0] = False
    return np.where(hole, r.choice(np.array([-1, -7, ns, ns + 5]), nb.shape), nb)


def _index_tensor(nb, form, device):
    nq, kmax = nb.shape
    if form == "int64":
        return T(nb.astype(np.int64)).to(device)
    if form == "rowstride":                      # a column slice of a wider matrix whose tail holds VALID indices
        wide = np.concatenate([nb, np.zeros((nq, 3), nb.dtype)], 1).astype(np.int32)
        t = T(wide).to(device)[:, :kmax]
        assert t.stride(0) == kmax + 3
        return t
    if form == "colstride":                      # every other column of a wider matrix: stride(1) = 2
        wide = np.zeros((nq, 2 * kmax), np.int32)
        wide[:, ::2] = nb
        t = T(wide).to(device)[:, ::2]
        assert t.stride(1) == 2
        return t
    return T(nb.astype(np.int32)).to(device)


def _stem_check(device, what, lengths, q, s, nb, x, w, kp, srt, eps, form="int32"):
    """One fused call against float64: output at the bound of the module docstring, statistics by the
    instnorm_stats rule; returns (out, ref, ratio)."""
    raw = fc.kpconv_f64(q, s, nb, x, w, kp, EXT)
    ref = fc.instnorm_f64(T(raw), lengths, eps=eps, slope=SLOPE)
    m64, r64 = fc.instnorm_stats_f64(T(raw), lengths, eps=eps)
    cu = ops.lengths_to_cu(lengths, device)
    args = (T(q).to(device), T(s).to(device), _index_tensor(nb, form, device), T(x).to(device), T(w).to(device),
            T(kp).to(device), EXT, cu)
    kw = dict(eps=eps, slope=SLOPE, rows_sorted=srt, max_len=max(lengths))
    out, mean, rstd = stem.kpconv_stem(*args, return_stats=True, **kw)
    assert torch.equal(out, stem.kpconv_stem(*args, **kw)), f"{what}: two launches differ"
    got = out.cpu().to(F64)
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
    seg = torch.repeat_interleave(torch.arange(len(lengths)), torch.as_tensor(lengths))
    raw_max = float(np.abs(raw).max())
    lim = 1e-5 * raw_max * r64[seg] + 2e-6 * ref.abs()
    ratio = float(((got - ref).abs() / lim).max())
    # statistics, (a): the rule of test_instnorm_variants_bitwise as it stands there -- the float64 statistics of the
    # float32 tensor the statistics are OF.  The stem never writes that tensor; its rows have ops.kpconv_raw's bits
    # (include/spr.h), so that call supplies it.
    raw32 = ops.kpconv_raw(*args[:7], rows_sorted=srt).cpu()
    m32, r32 = fc.instnorm_stats_f64(raw32, lengths, eps=eps)
    mean, rstd = mean.cpu().to(F64), rstd.cpu().to(F64)
    e_mean = float((mean - m32).abs().max()) / max(2.0 ** -23 * float(m32.abs().max()), 1e-300)
    e_rstd = float(((rstd - r32) / r32).abs().max()) / 2e-6
    # (b): against the statistics of the float64 raw tensor, with KPConv's own allowance carried along: a mean of
    # values each within e = 1e-5 max|raw_ref| is within e; var moves by at most 2 sigma e + e^2, so rstd moves by
    # at most rstd^2 sigma e <= e rstd relative (sigma rstd <= 1)
    e = 1e-5 * raw_max
    c_mean = float(((mean - m64).abs() / (e + 2.0 ** -23 * float(m64.abs().max()))).max())
    c_rstd = float((((rstd - r64) / r64).abs() / (e * r64 + 2e-6)).max())
    print(f"{what}: err {float((got - ref).abs().max()):.3e} scale {float(ref.abs().max()):.3e} raw scale {raw_max:.3e} "
          f"ratio {ratio:.3f}; statistics of the float32 rows: mean ratio {e_mean:.3f}, rstd ratio {e_rstd:.3f}; "
          f"of the float64 rows: mean ratio {c_mean:.3f}, rstd ratio {c_rstd:.3f}")
    assert raw_max > 0 and ratio <= 1.0, f"{what}: output {ratio:.3f} of its bound"
    assert e_mean <= 1.0, f"{what}: mean {e_mean:.3f} of 2^-23 max|mean|"
    assert e_rstd <= 1.0, f"{what}: rstd {e_rstd:.3f} of 2e-6 relative"
    assert c_mean <= 1.0 and c_rstd <= 1.0, f"{what}: statistics against the float64 rows: {c_mean:.3f}, {c_rstd:.3f}"
    (parts, n) = ops._get_range(out)
    assert parts is not None and float(parts[:n].max()) == float(out.abs().max())
    return out.cpu(), ref, ratio


@pytest.mark.parametrize("name", list(STEM_CASES))
def test_stem_against_float64(device, name):
    """The ragged batch (clouds of 1, 15, 16, 0, 17, 511, 512, 513, 1030 rows) on every path of the lean cross."""
    n_kp, kmax, srt, cout, eps, form = STEM_CASES[name]
    nq, ns = sum(STEM_LENGTHS), sum(STEM_LENGTHS) + 85
    # sorted rows wider than one chunk: fill 0.95, so that rows end in the last pass as well as before it
    q, s, nb = fc.kp_cloud_case(nq, ns, kmax, 1e2, EXT, 91, rows_sorted=srt, fill=0.95 if kmax > 64 else 0.7)
    if not srt:
        nb = _holes(nb, ns, kmax)
        assert (nb == ns).any() and (kmax == 1 or ((nb < 0).any() and (nb > ns).any()))   # (column 0 keeps its entry)
    if kmax > 64 and srt:
        nb[16:32, 20:] = ns                      # a whole wave is done after the first chunk
        nb[100:140, 70:] = ns                    # rows that end early in the second
        assert ((nb < ns).sum(1) == kmax).any() and ((nb < ns).sum(1) < 64).any()   # rows that end in either pass
    x = _features(ns, "random", 92)
    w, kp = fc.kp_weights(1, cout, 93, n_kp), fc.random_kernel_points(EXT, 94, n_kp)
    out, _, _ = _stem_check(device, f"stem [{name}]", STEM_LENGTHS, q, s, nb, x, w, kp, srt, eps, form)
    assert STEM_LENGTHS[0] == 1 and torch.equal(out[0], torch.zeros(cout)), "a one-row cloud is exactly 0"


@pytest.mark.parametrize("n_kp", [1, 7, 16])
def test_cin1_gather_kernel_point_counts(device, n_kp):
    """test_gpu_stem.py::test_cin1_gather_shapes' check (ops.kpconv_raw, Cin = 1, 1e-5 of the output's scale against
    float64) at the kernel-point counts it never runs: one, seven, and all sixteen slots."""
    for nq, kmax in ((1, 1), (17, 5), (65, 41), (1000, 40), (85, 70)):
        ns = nq + 37
        w, kp = fc.kp_weights(1, 64, 71, n_kp), fc.random_kernel_points(EXT, 72, n_kp)
        for srt in (True, False):
            q, s, nb = fc.kp_cloud_case(nq, ns, kmax, 1e2, EXT, 73, rows_sorted=srt)
            for pad in (0, 3):
                for kind in ("ones", "random"):
                    _check(device, q, s, nb, _features(ns, kind, 74), w, kp, srt, pad,
                           f"cin1 n_kp {n_kp} nq {nq} kmax {kmax} srt={srt} stride {kmax + pad} x={kind}")


DEGENERATE = [40, 1, 50, 100]          # all-shadow rows / one row / identical rows / an ordinary cloud


@pytest.mark.parametrize("w_scale", [2.0 ** -10, 1.0, 2.0 ** 10])
@pytest.mark.parametrize("eps", [1e-5, 1e-3])
def test_stem_degenerate_clouds_and_weight_scales(device, w_scale, eps):
    """A cloud whose every row is all shadow (raw 0: output exactly 0), a one-row cloud (exactly 0), a cloud of
    identical rows (variance 0: eps alone decides; the float64 output is exactly 0), next to an ordinary cloud, with the
    weights scaled by 2^-10, 1 and 2^10 (eps makes the operator scale dependent: each scale has its own reference)."""
    nq, ns, kmax, cout = sum(DEGENERATE), 260, 20, 32
    q, s, nb = fc.kp_cloud_case(nq, ns, kmax, 1e2, EXT, 95, rows_sorted=True)
    nb[:40] = ns
    q[41:91] = q[41]
    nb[41:91] = nb[41]
    assert (nb[41] < ns).sum() > 3 and (nb[91:] < ns).any(1).sum() > 90
    x = _features(ns, "random", 96)
    w = fc.kp_weights(1, cout, 97) * np.float32(w_scale)
    kp = fc.random_kernel_points(EXT, 98)
    out, ref, _ = _stem_check(device, f"stem degenerate W*{w_scale:g} eps {eps:g}", DEGENERATE, q, s, nb, x, w, kp, True, eps)
    assert torch.equal(out[:41], torch.zeros(41, cout)), "all-shadow rows and the one-row cloud are exactly 0"
    assert float(ref[41:91].abs().max()) <= 1e-10             # float64: the mean of 50 equal numbers, to rounding
    # fifty equal float32 rows: their float64 sum and its fiftieth are exact, so the mean IS the row and x - mean is 0
    assert torch.equal(out[41:91], torch.zeros(50, cout)), "the cloud of identical rows is exactly 0"
    assert float(out[91:].abs().max()) > 0.5 * float(ref[91:].abs().max()) > 0      # the ordinary cloud is live at every scale
