"""Seeded cases of KPConv on per-point input features (2 <= Cin <= 8: spr_kpconv_fwd's small-Cin kernel), on top of
tests/forward_cases.py, shared by tests/test_point_feats_host.py (conditions, without a GPU), tests/test_gpu_point_feats.py
and scripts/gen_point_feats_golden.py.

The neighbour count of KPConv is the number of valid neighbours whose feature SUM is positive, so a row whose sum sits
at rounding distance from 0 could be counted by one summation order and not by another.  Every features builder here
keeps the stated condition (check_conditions): a support row either

    has |sum_c f| >= 1e-3 * sum_c |f|     (float32 summation in any order errs by at most (C - 1) 2^-24 sum |f|, C <= 8)

or holds small integers only (|f| < 2^10: every partial sum is exact in float32 and float64, in any order).  The sign
of the sum is then the same in float32 and float64 and in every order, and kpconv_f64's count is the kernel's."""
import numpy as np
import torch

import forward_cases as fc
from superpoints_registration_amd import synthetic

WIDTHS = [2, 3, 4, 5, 8]                 # both record sizes (two / three 16-byte pieces) and every batch setting
MARGIN = 1e-3


def _enforce_margin(x, r):
    """Rows of x (float64 work copy) whose sum is within the margin get column 0 moved so that the sum is +-(0.25 ..
    0.5) of the row's absolute sum: the sign is drawn, so rows that do not count stay in the case."""
    s, a = x.sum(1), np.abs(x).sum(1)
    bad = np.abs(s) < 4 * MARGIN * a
    sign = np.where(r.random(x.shape[0]) < 0.5, -1.0, 1.0)
    x[bad, 0] += (sign * r.uniform(0.25, 0.5, x.shape[0]) * np.maximum(a, 1e-30) - s)[bad]
    return x


def features(ns, c, seed, kind="signed"):
    """[ns, c] float32.
    'signed'   uniform in (-0.6, 0.4): about half of the rows have a negative sum and do not count;
    'colour'   [1, r, g, b, ...]: a column of ones, then uniform (0, 1) -- the KPConv convention (ones first);
    'negative' every entry negative: no neighbour counts, the divisor is 1 everywhere;
    'integer'  small integers in [-2, 2]; rows 0 .. ns/4 sum to exactly 0, the next ns/4 to exactly -1."""
    r = fc.rng_of(801, seed, ns, c)
    if kind == "integer":
        x = r.integers(-2, 3, (ns, c)).astype(np.float64)
        a, b = ns // 4, ns // 2
        x[:a, 0] -= x[:a].sum(1)
        x[a:b, 0] -= x[a:b].sum(1) + 1
        return x.astype(np.float32)
    if kind == "colour":
        x = r.random((ns, c))
        x[:, 0] = 1.0
        return x.astype(np.float32)
    if kind == "negative":
        return (-0.05 - r.random((ns, c))).astype(np.float32)
    assert kind == "signed", kind
    x = _enforce_margin(r.random((ns, c)) - 0.6, r).astype(np.float32)
    return x


def magnitude_features(ns, c, seed, lo=-12, hi=12):
    """Each column its own magnitude, 10^lo .. 10^hi spread over the columns in a seeded order, entries +-(0.25 .. 1) of
    it: the largest column decides every row's sum (|sum| >= 0.25 m - (c - 1) m / 10^(step))."""
    r = fc.rng_of(802, seed, ns, c)
    mags = 10.0 ** r.permutation(np.linspace(lo, hi, c))
    x = r.uniform(0.25, 1.0, (ns, c)) * np.where(r.random((ns, c)) < 0.5, -1.0, 1.0) * mags[None, :]
    return x.astype(np.float32), mags


def magnitude_weights(c, cout, seed, n_kp=15, lo=-12, hi=12):
    """Weights whose [input column, output column] blocks have their own magnitude 10^lo .. 10^hi per OUTPUT column and
    O(1) across input columns: with magnitude_features an output column's scale is (largest feature magnitude) x (its
    own), at most 10^(hi + hi) = 1e24, inside float32."""
    r = fc.rng_of(803, seed, c, cout)
    mags = 10.0 ** r.uniform(lo, hi, cout)
    w = (r.random((n_kp, c, cout)) - 0.5) * mags[None, None, :]
    return w.astype(np.float32), mags


def check_conditions(x):
    """The stated condition, row by row, in float64 on the float32 values."""
    x = np.asarray(x, np.float32).astype(np.float64)
    assert x.ndim == 2 and 1 <= x.shape[1] <= 8 and np.isfinite(x).all()
    integer = np.all(x == np.round(x), axis=1) & np.all(np.abs(x) < 2 ** 10, axis=1)
    s, a = x.sum(1), np.abs(x).sum(1)
    ok = integer | (np.abs(s) >= MARGIN * a) & (a > 0)
    assert ok.all(), f"{int((~ok).sum())} rows sit within {MARGIN:g} of a zero sum: the count would depend on the order"
    return integer


def count_f64(nb, x):
    """The divisor's count restated: valid neighbours whose float64 feature sum is > 0."""
    nb = np.asarray(nb, np.int64)
    ns = x.shape[0]
    ok = (nb >= 0) & (nb < ns)
    pos = np.asarray(x, np.float64).sum(1) > 0
    return (pos[np.where(ok, nb, 0)] & ok).sum(1)


def kernel_case(nq, ns, kmax, c, cout, seed, kind="signed", offset=1e2, ext=0.125, rows_sorted=True, n_kp=15, fill=0.7):
    """(q, s, nb, x, w, kp, ext) of one kernel call: fc.kp_cloud_case geometry, features(kind), fc.kp_weights."""
    q, s, nb = fc.kp_cloud_case(nq, ns, kmax, offset, ext, seed, rows_sorted=rows_sorted, fill=fill)
    x = features(ns, c, seed + 1, kind)
    w = fc.kp_weights(c, cout, seed + 2, n_kp=n_kp)
    kp = fc.random_kernel_points(ext, seed + 3, n_kp=n_kp) if n_kp > 1 else np.zeros((1, 3), np.float32)
    return q, s, nb, x, w, kp, ext


# every (nq, ns, kmax, c, cout, kind, rows_sorted, n_kp) the GPU tests run through kernel_case: one representative per
# class -- query counts around the 16-query wave and the 64-query workgroup, row widths around the record batches
# (4 / 6 / 8) and the 64-column staged chunk, every width, cout with and without a partial 16-column block
SHAPE_CASES = [
    (1, 40, 1, 2, 16, "signed", True, 15), (15, 60, 8, 3, 40, "colour", True, 15), (16, 60, 9, 4, 64, "signed", False, 15),
    (17, 80, 63, 5, 16, "signed", True, 15), (63, 90, 64, 8, 40, "colour", False, 15), (64, 120, 65, 2, 64, "signed", True, 15),
    (65, 150, 129, 4, 40, "signed", False, 15), (300, 350, 40, 8, 64, "signed", True, 15), (300, 350, 40, 5, 64, "colour", True, 16),
    (70, 100, 12, 3, 64, "signed", True, 1), (300, 350, 129, 8, 16, "signed", True, 16), (33, 64, 7, 4, 1, "signed", True, 15),
]
COUNT_KINDS = ["negative", "integer", "signed"]


# ---- the encoder fixture (tests/golden/point_feats.npz) ------------------------------------------------------------------
GOLDEN_SEED = 17
GOLDEN_SIZES = (600, 500)
GOLDEN_C = 4


def golden_inputs():
    """One small 3DMatch-like pair, features [1, r, g, b]-like per point and the seed of the cotangent, all regenerable:
    (src [600, 3], tgt [500, 3], feats_src, feats_tgt)."""
    n, m = GOLDEN_SIZES
    src, tgt, _ = synthetic.make_pair(max(n, m), seed=GOLDEN_SEED, extent=0.4, jitter=0.002, trans=(0.03, -0.02, 0.01))
    src, tgt = np.ascontiguousarray(src[:n]), np.ascontiguousarray(tgt[:m])
    fs, ft = features(n, GOLDEN_C, GOLDEN_SEED + 1, "colour"), features(m, GOLDEN_C, GOLDEN_SEED + 2, "colour")
    return src, tgt, fs, ft


def golden_cotangent(shape):
    return synthetic.rand(tuple(int(v) for v in shape), GOLDEN_SEED + 3)


def grad_sample_indices(name, numel, k=64):
    """Pinned positions of a large gradient tensor (oracle.gen_golden.grad_sample_indices' rule, restated so that the
    test needs no generator module)."""
    rng = np.random.default_rng(synthetic._seed_of(name, 123) % (2 ** 32))
    return rng.integers(0, numel, size=min(k, numel))


def model_feats(lens, c, seed, device=None):
    """Per-cloud feature tensors for the model-level tests: 'colour' features of each length."""
    out = [torch.from_numpy(features(int(n), c, seed + i, "colour")) for i, n in enumerate(lens)]
    return [t.to(device) for t in out] if device is not None else out
