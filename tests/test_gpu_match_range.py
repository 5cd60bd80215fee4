"""GPU: the matching head, the pose solve and the loss terms across shapes, score ranges and geometries.

test_gpu_ops.py checks the dual softmax and Sinkhorn at one 60 x 47 pair, the Procrustes solve on well-conditioned
clouds and each loss at one shape.  Here every dispatch path of match_pose.hip meets a float64 torch reference on the
CPU (loops per pair):
  * dual softmax (match_dualsoftmax / _top2): batches whose max_m crosses every k_row_lse threshold (v<4> up to 1024,
    v<8> up to 2048, v<16> up to 4096, the generic kernel above), min_m < 4 (k_col_lse) and m = 1, 2, 3 mod 4
    (k_col_lse_v's shifted last quad), N > M, N = M and N < M in one batch (k_match_cols / k_match_rows), every
    grouped-GEMM tile (max_m <= 32, <= 255, >= 256), d in {32, 96, 256}, both gemm modes; flat, unit and sharp
    scores (|score| up to ~100: exp overflows unless the maximum is subtracted, the product underflows), near and
    exact duplicates, and pairs whose features differ by 1e+-4 in one batch (one range measurement for all pairs);
  * Sinkhorn (sinkhorn_correspondences, match_and_sinkhorn): n_iters 0..5, both softplus branches, 1 / (e^beta +
    0.02) from 0.05 to 50, target coordinates at 1 and 1e3; every head of spr_match_sinkhorn (fused <4> / <8>,
    unfused at n_iters = 0, max_m > 2048, min_m < 4) against float64 and bit for bit against the two operators;
  * weighted Procrustes: near-planar, colinear, mirrored, isotropic, 180-degree and far-off-origin sets, weight sums
    below the 1e-6 clamp, zero and single weights, 1..3 points, empty segments; pose_residuals and pose_scores;
  * the backward of Sinkhorn (double potentials: k_row_lse_v<4/8, double>, generic k_row_lse<double>,
    k_col_lse<double>), the dual softmax and Procrustes at those shapes;
  * the forward loss terms (InfoNCE, BCE, transform L1, overlap pooling) at their edges.

Bounds (derived next to each check):
  * scores: e_ij = (2^-21 + sqrt(d) 2^-24) sum_k |fs_ik||ft_jk| / sqrt(d)  (test_gpu_range._check_gemm) plus
    2^-22 |score_ij| (the float32 1/sqrt(d) and its product);
  * dual softmax: log-sum-exp is 1-Lipschitz in max-norm, so log attn_ij = 2 c_ij - rowlse_i - collse_j moves by
    at most 2 e_ij + max_j e_ij + max_i e_ij, plus the float32 rounding of the two logs, of their sums and of the
    two exp arguments;
  * Sinkhorn: an affinity error eps moves every half-step (a log-sum-exp) by at most eps more than its input
    potential, so u_t and v_t are off by at most (2t + 1)(eps + gamma), gamma being one pass's own float32 rounding;
    log P_ij = A_ij - u_i - v_j then by delta = eps + 2 (2n + 1)(eps + gamma) + the rounding of its argument, and w,
    t_hat = sum_j P_ij t_j / (w + 1e-6) follow as relative sums (plus m 2^-125 for underflowed terms);
  * Procrustes: R per element by 2^-23 (output rounding) + kappa n 2^-52 (1 + |c| / extent), kappa = s1 / (s2 + s3)
    the conditioning of the polar factor; where R is not unique (rank <= 1), R R^T = I, det R = 1 and the weighted
    cost against the float64 optimum instead.
"""
import math

import pytest
import torch

from oracle import torch_oracle as O
from superpoints_registration_amd import ops, synthetic

pytestmark = pytest.mark.gpu
F64 = torch.float64
U = 2.0 ** -24
TINY = 2.0 ** -126


@pytest.fixture
def gemm_mode(request):
    ops.set_gemm_mode(request.param)
    yield request.param
    ops.set_gemm_mode(1)


def _coef(k):
    return 2.0 ** -21 + math.sqrt(k) * 2.0 ** -24


def _cu(ns, ms):
    cu = [0]
    for x in list(ns) + list(ms):
        cu.append(cu[-1] + x)
    return cu


# ---- batches ------------------------------------------------------------------------------------------------ #
# name -> (d, [(n, m), ...]).  max_m picks the row kernel and the GEMM tile, min_m the column kernel.
BATCHES = {
    "tiny": (32, [(1, 1), (2, 2), (3, 3), (5, 4), (4, 5), (63, 1), (1, 65), (64, 3)]),     # max_m 65, k_col_lse
    "tile32": (32, [(3, 1), (1, 2), (2, 3), (40, 32), (30, 31)]),                          # 128 x 32 tile
    "quads": (96, [(63, 64), (64, 63), (65, 65), (130, 66), (66, 67), (200, 5), (7, 9)]),  # k_col_lse_v, m % 4 = 0..3
    "m1023": (96, [(1000, 1023), (1023, 1021), (6, 6)]),                                   # v<4>
    "m1024": (256, [(1100, 1024), (1023, 1022), (9, 7)]),                                  # v<4>, 256 tile
    "m1025": (256, [(1025, 1025), (700, 1023), (1030, 4)]),                                # v<8>
    "m2048": (256, [(2049, 2048), (2047, 2047)]),                                          # v<8>
    "m2049": (256, [(2000, 2049), (2100, 6), (5, 2)]),                                     # v<16>, k_col_lse
    "m4096": (256, [(4097, 4096), (65, 7)]),                                               # v<16>
    "m4097": (256, [(4096, 4097), (3, 1)]),                                                # generic k_row_lse
}
SMALL = ["tiny", "tile32", "quads"]
REGIMES = {"flat": 0.05, "unit": 1.0, "sharp": 4.5}      # feature sigma: score ~ sigma^2 (sharp: |score| ~ 100)


def _features(name, regime, seed=0):
    """Per pair fs [n, d], ft [m, d] (float32), packed as src tokens of every pair, then tgt tokens."""
    d, pairs = BATCHES[name]
    g = torch.Generator().manual_seed(1000 + 17 * seed + sum(n + 3 * m for n, m in pairs))
    fs, ft = [], []
    for k, (n, m) in enumerate(pairs):
        if regime == "mixed":               # one range measurement for the whole batch: pairs 1e4 apart
            sig = 2.0 * (1.0, 1e-4, 1e4)[k % 3]
        else:
            sig = REGIMES.get(regime, 1.0)
        a = torch.randn((n, d), generator=g) * sig
        b = torch.randn((m, d), generator=g) * sig
        if regime == "neardup":             # rows and columns 1e-6 apart: near-ties in the arg-max
            a[1::2] = a[0:n - 1:2] + 1e-6 * torch.randn((n // 2, d), generator=g)
            b[1::2] = b[0:m - 1:2] + 1e-6 * torch.randn((m // 2, d), generator=g)
        fs.append(a)
        ft.append(b)
    return fs, ft


def _pack(fs, ft):
    return torch.cat(fs + ft).contiguous(), _cu([t.shape[0] for t in fs], [t.shape[0] for t in ft])


_REF = {}


def _score_ref(a, b):
    """float64 scaled correlation, its per-element bound e_ij."""
    d = a.shape[1]
    a64, b64 = a.to(F64), b.to(F64)
    c = a64 @ b64.t() / math.sqrt(d)
    e = _coef(d) * (a64.abs() @ b64.abs().t()) / math.sqrt(d) + 2.0 ** -22 * c.abs()
    return c, e


def _ds_ref(a, b):
    """Per pair: (log attn on the matching side [K, L]: max over dim 1, its per-element bound)."""
    n, m = a.shape[0], b.shape[0]
    c, e = _score_ref(a, b)
    rl = torch.logsumexp(c, 1, keepdim=True)
    cl = torch.logsumexp(c, 0, keepdim=True)
    la = 2 * c - rl - cl
    bnd = 2 * e + e.amax(1, keepdim=True) + e.amax(0, keepdim=True)
    # float32: rowlse / collse rounded (|lse| 2^-24, sums of up to max(n, m) terms in lanes, the log), the two exp
    # arguments c - lse formed in float32, two expf and their product
    bnd = bnd + U * (rl.abs() + cl.abs()) + (max(n, m) / 16 + 40) * U + 2 * U * ((c - rl).abs() + (c - cl).abs())
    if n > m:
        return la.t().contiguous(), bnd.t().contiguous()
    return la, bnd


def _ds_cached(name, regime):
    key = ("ds", name, regime)
    if key not in _REF:
        fs, ft = _features(name, regime)
        _REF[key] = [_ds_ref(a, b) for a, b in zip(fs, ft)]
    return _REF[key]


def _check_dual_softmax(name, fs, ft, refs, val, val2, ind, what):
    cu = _cu([t.shape[0] for t in fs], [t.shape[0] for t in ft])
    B = len(fs)
    val, ind = val.cpu().to(F64), ind.cpu().long()
    val2 = None if val2 is None else val2.cpu().to(F64)
    for k, (a, b) in enumerate(zip(fs, ft)):
        n, m = a.shape[0], b.shape[0]
        beg = cu[B + k] if n > m else cu[k]           # N > M: one match per tgt token, else per src token
        K = m if n > m else n
        la, bnd = refs[k]
        v, i = val[beg:beg + K], ind[beg:beg + K]
        assert bool(((i >= 0) & (i < la.shape[1])).all()), f"{what} pair {k}: index out of range"
        top = la.topk(min(2, la.shape[1]), 1)
        l1 = top.values[:, 0]
        l2 = top.values[:, 1] if la.shape[1] > 1 else torch.full_like(l1, -math.inf)
        bmax = bnd.amax(1)
        # order statistics are 1-Lipschitz in max-norm; only entries within 2 max(B) of one can take its place
        b1 = torch.where(la >= (l1 - 2 * bmax)[:, None], bnd, torch.zeros_like(bnd)).amax(1)
        v64 = l1.exp()
        under = v64 < TINY
        # where the float64 value is below 2^-126 the float32 product of two expf underflows the same way: the
        # kernel returns a value <= 2^-126 (a denormal or 0) there, and any index (no arg-max is asserted)
        assert bool((v[under] <= TINY * 1.01).all()), f"{what} pair {k}: underflowed value above 2^-126"
        ok = ~under
        allow = v64 * torch.expm1(b1) + 2.0 ** -148
        err = (v - v64).abs()
        bad = ok & (err > allow)
        assert not bool(bad.any()), (f"{what} pair {k}: val row {int(bad.nonzero()[0])} err "
                                     f"{float(err[bad][0]):.3e} > {float(allow[bad][0]):.3e} (val64 {float(v64[bad][0]):.3e})")
        # the index: the float64 arg-max, or a member of its near-tie set
        lk = la.gather(1, top.indices[:, :1])[:, 0]
        li = la.gather(1, i[:, None])[:, 0]
        tie = li >= lk - bnd.gather(1, top.indices[:, :1])[:, 0] - bnd.gather(1, i[:, None])[:, 0]
        bad = ok & ~tie
        assert not bool(bad.any()), (f"{what} pair {k}: ind of row {int(bad.nonzero()[0])} = {int(i[bad][0])} is not "
                                     f"in the near-tie set of {int(top.indices[bad, 0][0])}")
        if val2 is not None and la.shape[1] > 1:
            v2 = val2[beg:beg + K]
            b2 = torch.where(la >= (l2 - 2 * bmax)[:, None], bnd, torch.zeros_like(bnd)).amax(1)
            w64 = l2.exp()
            u2 = w64 < TINY
            assert bool((v2[u2] <= TINY * 1.01).all()), f"{what} pair {k}: underflowed val2 above 2^-126"
            err2 = (v2 - w64).abs()
            bad = ~u2 & (err2 > w64 * torch.expm1(b2) + 2.0 ** -148)
            assert not bool(bad.any()), f"{what} pair {k}: val2 row {int(bad.nonzero()[0])} err {float(err2[bad][0]):.3e}"


# ---- 1. dual softmax ------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("regime", ["flat", "unit", "sharp"])
@pytest.mark.parametrize("name", list(BATCHES))
@pytest.mark.parametrize("gemm_mode", [1, 0], indirect=True, ids=["split", "f32"])
def test_dual_softmax_every_path(device, name, regime, gemm_mode):
    fs, ft = _features(name, regime)
    feat, cu_host = _pack(fs, ft)
    cu = torch.tensor(cu_host, dtype=torch.int32, device=device)
    val, val2, ind = ops.match_dualsoftmax_top2(feat.to(device), cu, cu_host, len(fs))
    _check_dual_softmax(name, fs, ft, _ds_cached(name, regime), val, val2, ind, f"{name} {regime} mode {gemm_mode}")
    # the single-output entry point runs the same kernels: the same bits
    v1, i1 = ops.match_dualsoftmax(feat.to(device), cu, cu_host, len(fs))
    assert torch.equal(v1, val) and torch.equal(i1, ind)


@pytest.mark.parametrize("regime", ["neardup", "mixed"])
@pytest.mark.parametrize("name", SMALL + ["m1024"])
@pytest.mark.parametrize("gemm_mode", [1, 0], indirect=True, ids=["split", "f32"])
def test_dual_softmax_near_ties_and_mixed_magnitudes(device, name, regime, gemm_mode):
    """Rows / columns 1e-6 apart (the index must lie in the float64 near-tie set); pairs of score magnitude 4, 4e-8
    and 4e8 in one batch: the small pair's products keep their own per-element bound under the shared range."""
    fs, ft = _features(name, regime)
    feat, cu_host = _pack(fs, ft)
    cu = torch.tensor(cu_host, dtype=torch.int32, device=device)
    val, val2, ind = ops.match_dualsoftmax_top2(feat.to(device), cu, cu_host, len(fs))
    _check_dual_softmax(name, fs, ft, _ds_cached(name, regime), val, val2, ind, f"{name} {regime} mode {gemm_mode}")


@pytest.mark.parametrize("gemm_mode", [1, 0], indirect=True, ids=["split", "f32"])
def test_dual_softmax_exact_ties_take_the_lowest_index(device, gemm_mode):
    """Duplicated features give bit-identical scores, row and column sums: the lowest index must win, in
    k_match_rows (N <= M, duplicated targets) and in k_match_cols (N > M, duplicated sources), for duplicates in
    the same lane (64 apart) and in different lanes (1 and 5 apart)."""
    g = torch.Generator().manual_seed(77)
    d = 64
    fs, ft, expect = [], [], []
    for n, m in ((150, 300), (300, 150), (260, 260)):
        big, small = max(n, m), min(n, m)
        base = torch.randn((big, d), generator=g)
        for off in (1, 5, 64):
            for j in range(3 * off, big - off, 7 * off + 3):
                base[j + off] = base[j]
        probe = torch.randn((small, d), generator=g) * 0.3
        pick = torch.randint(0, big, (small,), generator=g)
        probe += base[pick] * 1.5                       # each probe close to one (possibly duplicated) row
        a, b = (probe, base) if n <= m else (base, probe)
        fs.append(a)
        ft.append(b)
        # lowest index among exact float64 ties of the maximum
        c = (probe.to(F64) @ base.to(F64).t()) / math.sqrt(d)
        la = torch.log_softmax(c, 0) + torch.log_softmax(c, 1)      # [probe, base]: the matching side's rows
        best = la.amax(1, keepdim=True)
        first = torch.where(la == best, torch.arange(big)[None, :], big).amin(1)
        expect.append((first, int((la == best).sum(1).gt(1).sum())))
    feat, cu_host = _pack(fs, ft)
    cu = torch.tensor(cu_host, dtype=torch.int32, device=device)
    val, ind = ops.match_dualsoftmax(feat.to(device), cu, cu_host, 3)
    ind = ind.cpu().long()
    B = 3
    for k, (a, b) in enumerate(zip(fs, ft)):
        n, m = a.shape[0], b.shape[0]
        beg, K = (cu_host[B + k], m) if n > m else (cu_host[k], n)
        first, nties = expect[k]
        assert nties > 10, "the case must contain exact ties"
        # rows whose float64 maximum is an exact tie (or unique with a clear gap) must pick the lowest index
        got = ind[beg:beg + K]
        bad = got != first
        assert not bool(bad.any()), f"pair {k} ({n} x {m}): row {int(bad.nonzero()[0])} picked {int(got[bad][0])}, " \
                                    f"the lowest tied index is {int(first[bad][0])}"


# ---- 2. Sinkhorn ------------------------------------------------------------------------------------------------ #
def _softplus(al):
    return al if al > 20.0 else math.log1p(math.exp(al))


def _sk_ref(a, b, xt, alpha, beta, n_iters):
    """float64 slack Sinkhorn in potential form (= the oracle's padded-matrix form, se3_torch.py:186-197) and the
    per-row bounds of w and t_hat."""
    n, m = a.shape[0], b.shape[0]
    al, be = float(torch.tensor(alpha, dtype=torch.float32)), float(torch.tensor(beta, dtype=torch.float32))
    c, e = _score_ref(a, b)
    sp, inv = _softplus(al), 1.0 / (math.exp(be) + 0.02)
    A = -(c.clamp_min(0.0) - sp) * inv
    u = torch.zeros(n, dtype=F64)
    v = torch.zeros(m, dtype=F64)
    zero = torch.zeros(1, dtype=F64)
    for _ in range(n_iters):
        u = torch.logsumexp(torch.cat([A - v[None, :], zero.expand(n, 1)], 1), 1)
        v = torch.logsumexp(torch.cat([A - u[:, None], zero.expand(1, m)], 0), 0)
    lp = A - u[:, None] - v[None, :]
    P = lp.exp()
    w = P.sum(1)
    t64 = xt.to(F64)
    that = P @ t64 / (w[:, None] + 1e-6)
    # eps: affinity error (score bound times 1/den, plus the float32 evaluation of the affinity and of sp, 1/den)
    amax = float(A.abs().max())
    eps = inv * float(e.max()) + 2.0 ** -22 * (amax + inv * (float(c.clamp_min(0).max()) + sp))
    pmax = max(float(u.abs().max()), float(v.abs().max()), 1.0)
    # gamma: one log-sum-exp pass in float32 (arguments A - pot, exp, lane sums of up to max(n, m) terms, the log)
    gamma = 2 * U * (amax + pmax) + 4 * U + (max(n, m) / 16 + 40) * U + U * pmax
    delta = eps + 2 * (2 * n_iters + 1) * (eps + gamma) + 2 * U * (amax + 2 * pmax) + 4 * U
    rel = math.expm1(delta) + (m / 64 + 8) * U
    bw = w * rel + m * 2.0 ** -125
    tabs = t64.abs()
    num_b = (P @ tabs) * (rel + 2 * U) + m * 2.0 ** -125 * float(tabs.max())
    den = w + 1e-6
    bt = (num_b / den[:, None] + that.abs() * ((bw + 2 * U * den) / den)[:, None]) * 1.01 + 2 * U * that.abs()
    # rows whose sums exceed the float32 range (n_iters = 0 with softplus(alpha) / den ~ 1000: e^A overflows,
    # float64 too beyond e^709); the float32 reference overflows the same way
    over = ~torch.isfinite(w) | (w * (1 + rel) > 1e38) | ~torch.isfinite(P @ tabs).all(1) | \
        ((P @ tabs) * (1 + rel) > 1e38).any(1)
    return w, that, bw, bt, over


def _check_sinkhorn(fs, ft, xyz_t, w, that, alpha, beta, n_iters, what, cache_key=None):
    B = len(fs)
    cu = _cu([t.shape[0] for t in fs], [t.shape[0] for t in ft])
    w, that = w.cpu().to(F64), that.cpu().to(F64)
    for k in range(B):
        key = None if cache_key is None else cache_key + (k,)
        if key is not None and key in _REF:
            ref = _REF[key]
        else:
            ref = _sk_ref(fs[k], ft[k], xyz_t[k], alpha, beta, n_iters)
            if key is not None:
                _REF[key] = ref
        w64, t64, bw, bt, over = ref
        s = slice(cu[k], cu[k + 1])
        wk, tk = w[s][~over], that[s][~over]
        # where the sums overflow float32 the kernel overflows too: w is inf or beyond 1e38 (no t_hat asserted)
        assert bool((w[s][over] > 0.99e38).all()), f"{what} pair {k}: finite w where float32 overflows"
        assert torch.isfinite(wk).all() and torch.isfinite(tk).all(), f"{what} pair {k}: non-finite output"
        ew = (wk - w64[~over]).abs()
        assert bool((ew <= bw[~over]).all()), (f"{what} pair {k}: w err {float(ew.max()):.3e}, worst ratio "
                                               f"{float((ew / bw[~over]).max()):.2f}")
        et = (tk - t64[~over]).abs()
        assert bool((et <= bt[~over]).all()), (f"{what} pair {k}: t_hat err {float(et.max()):.3e}, worst ratio "
                                               f"{float((et / bt[~over]).max()):.2f}")


def _xyz(fs, ft, scale, seed):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn((t.shape[0], 3), generator=g) * scale for t in fs]
    xt = [torch.randn((t.shape[0], 3), generator=g) * scale + 0.3 * scale for t in ft]
    return xs, xt


@pytest.mark.parametrize("n_iters", [0, 1, 3, 5])
@pytest.mark.parametrize("name", SMALL)
@pytest.mark.parametrize("gemm_mode", [1, 0], indirect=True, ids=["split", "f32"])
def test_sinkhorn_parameter_grid(device, name, n_iters, gemm_mode):
    """alpha on both softplus branches, 1 / (e^beta + 0.02) from 0.05 to 50, coordinates at 1 and 1e3."""
    fs, ft = _features(name, "unit")
    feat, cu_host = _pack(fs, ft)
    cu = torch.tensor(cu_host, dtype=torch.int32, device=device)
    dfeat = feat.to(device)
    for scale in (1.0, 1e3):
        xs, xt = _xyz(fs, ft, scale, 5)
        xyz = torch.cat(xs + xt).to(device)
        for alpha in (-30.0, 0.0, 19.9, 20.1, 30.0):
            for beta in (-8.0, 0.0, 3.0):
                w, that = ops.sinkhorn_correspondences(dfeat, xyz, cu, cu_host, len(fs), alpha, beta, n_iters)
                _check_sinkhorn(fs, ft, xt, w, that, alpha, beta, n_iters,
                                f"{name} it={n_iters} alpha={alpha} beta={beta} xyz~{scale:g} mode {gemm_mode}",
                                ("sk", name, "unit", scale, alpha, beta, n_iters))


@pytest.mark.parametrize("regime", ["flat", "unit", "sharp"])
@pytest.mark.parametrize("name", [n for n in BATCHES if n not in SMALL])
@pytest.mark.parametrize("gemm_mode", [1, 0], indirect=True, ids=["split", "f32"])
def test_sinkhorn_and_fused_head_large(device, name, regime, gemm_mode):
    """Every row / column kernel at the large thresholds, through sinkhorn_correspondences and through
    match_and_sinkhorn (fused <4> / <8> head up to max_m 2048 with min_m >= 4, the separate passes beyond),
    both against float64; the fused head's dual softmax against the same reference as §1."""
    fs, ft = _features(name, regime)
    feat, cu_host = _pack(fs, ft)
    cu = torch.tensor(cu_host, dtype=torch.int32, device=device)
    dfeat = feat.to(device)
    xs, xt = _xyz(fs, ft, 1e3 if regime == "unit" else 1.0, 6)
    xyz = torch.cat(xs + xt).to(device)
    alpha, beta, it = (0.8, -0.4, 3) if regime != "sharp" else (25.0, 1.0, 5)
    key = ("sk", name, regime, alpha, beta, it)
    w, that = ops.sinkhorn_correspondences(dfeat, xyz, cu, cu_host, len(fs), alpha, beta, it)
    _check_sinkhorn(fs, ft, xt, w, that, alpha, beta, it, f"{name} {regime} mode {gemm_mode}", key)
    v, v2, i, w1, t1 = ops.match_and_sinkhorn(dfeat, xyz, cu, cu_host, len(fs), alpha, beta, it, top2=True)
    _check_sinkhorn(fs, ft, xt, w1, t1, alpha, beta, it, f"{name} {regime} fused mode {gemm_mode}", key)
    _check_dual_softmax(name, fs, ft, _ds_cached(name, regime), v, v2, i, f"{name} {regime} fused mode {gemm_mode}")


@pytest.mark.parametrize("n_iters", [0, 1, 3])
@pytest.mark.parametrize("name", ["tiny", "quads", "m1025", "m2049"])
@pytest.mark.parametrize("gemm_mode", [1, 0], indirect=True, ids=["split", "f32"])
def test_match_and_sinkhorn_is_the_two_operators_bit_for_bit_every_head(device, name, n_iters, gemm_mode):
    """Sibling of test_gpu_ops' bit-for-bit test at the shapes of every head: unfused (min_m < 4: tiny, m2049;
    max_m > 2048: m2049; n_iters = 0), fused <4> (quads) and fused <8> (m1025)."""
    fs, ft = _features(name, "unit", seed=1)
    feat, cu_host = _pack(fs, ft)
    cu = torch.tensor(cu_host, dtype=torch.int32, device=device)
    dfeat = feat.to(device)
    xs, xt = _xyz(fs, ft, 1.0, 7)
    xyz = torch.cat(xs + xt).to(device)
    alpha, beta = torch.tensor(0.8, device=device), torch.tensor(-0.4, device=device)
    w0, t0 = ops.sinkhorn_correspondences(dfeat, xyz, cu, cu_host, len(fs), alpha, beta, n_iters)
    v0, v20, i0 = ops.match_dualsoftmax_top2(dfeat, cu, cu_host, len(fs))
    v1, v21, i1, w1, t1 = ops.match_and_sinkhorn(dfeat, xyz, cu, cu_host, len(fs), alpha, beta, n_iters, top2=True)
    for a, b, nm in ((v0, v1, "val"), (v20, v21, "val2"), (i0, i1, "ind"), (w0, w1, "w"), (t0, t1, "t_hat")):
        assert torch.equal(a, b), nm


# ---- 3. weighted Procrustes ------------------------------------------------------------------------------------- #
def _rot(g, angle=None, axis=None):
    if axis is None:
        axis = torch.randn(3, generator=g, dtype=F64)
    axis = axis / axis.norm()
    th = float(torch.rand(1, generator=g)) * math.pi if angle is None else angle
    K = torch.tensor([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], dtype=F64)
    return torch.eye(3, dtype=F64) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def _procrustes64(a, b, w):
    """compute_rigid_transform (utils/se3_torch.py:109-163) in float64, without the final float32 rounding, and the
    singular values of its covariance."""
    a, b = a.to(F64), b.to(F64)
    if w is not None:
        wn = w.to(F64)[:, None] / torch.clamp_min(w.to(F64).sum(), 1e-6)
        ca, cb = (a * wn).sum(0), (b * wn).sum(0)
        cov = (a - ca).t() @ ((b - cb) * wn)
    else:
        ca, cb = a.mean(0), b.mean(0)
        cov = (a - ca).t() @ (b - cb)
    u, s, vh = torch.linalg.svd(cov)
    v = vh.t()
    rot = v @ u.t()
    if torch.det(rot) <= 0:
        v = v.clone()
        v[:, 2] *= -1
        rot = v @ u.t()
    return rot, cb - rot @ ca, s, ca, cb


def _pcase(kind, g):
    """(a, b, w, unique): float32 point sets; unique = False where R is not determined (rank <= 1)."""
    R0 = _rot(g)
    t0 = torch.randn(3, generator=g, dtype=F64)
    n = 500
    a = torch.randn((n, 3), generator=g, dtype=F64)
    w = torch.rand(n, generator=g, dtype=F64)
    unique = True
    if kind.startswith("planar"):
        thick = float(kind.split("_")[1])
        a[:, 2] *= thick
        a = a @ _rot(g).t()
    elif kind == "colinear":
        a = torch.randn((n, 1), generator=g, dtype=F64) * torch.randn((1, 3), generator=g, dtype=F64)
        unique = False
    elif kind == "mirror":
        R0 = R0 @ torch.diag(torch.tensor([1.0, 1.0, -1.0], dtype=F64))       # det R0 = -1: the flip must fire
    elif kind == "cube":
        a = torch.tensor([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)], dtype=F64)
        w = None
    elif kind == "tetra":
        a = torch.tensor([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=F64)
        w = torch.ones(4, dtype=F64)
    elif kind == "rot180":
        R0 = _rot(g, angle=math.pi)
    elif kind in ("off1e3", "off1e4"):
        t0 = torch.full((3,), float(kind[3:]), dtype=F64)
        a = a + torch.tensor([-1.0, 2.0, 0.5], dtype=F64) * float(kind[3:])
    elif kind == "wsum_tiny":
        w = w / w.sum() * 1e-8                                                  # below the 1e-6 clamp
        a = a + 3.0
    elif kind == "w_zero":
        w = torch.zeros(n, dtype=F64)
        unique = False
    elif kind == "w_one":
        w = torch.zeros(n, dtype=F64)
        w[17] = 0.7
        unique = False
    elif kind.startswith("pts"):
        k = int(kind[3:])
        a, w = a[:k], w[:k]
        unique = k >= 3
    elif kind == "unweighted":
        w = None
    noise = 0.0 if kind in ("cube", "tetra") else 0.01
    b = a @ R0.t() + t0 + noise * torch.randn(a.shape, generator=g, dtype=F64)
    return a.float(), b.float(), None if w is None else w.float(), unique


PCASES = ["planar_0", "planar_1e-7", "planar_1e-6", "planar_1e-5", "planar_1e-3", "colinear", "mirror", "cube",
          "tetra", "rot180", "off1e3", "off1e4", "wsum_tiny", "w_zero", "w_one", "pts1", "pts2", "pts3", "unweighted"]


def _cost(a, b, w, R, t):
    a, b = a.to(F64), b.to(F64)
    r = ((b - (a @ R.t() + t)) ** 2).sum(1)
    return float((r * (1.0 if w is None else w.to(F64))).sum())


def _check_pose(got, a, b, w, unique, what):
    got = got.cpu().to(F64)
    R, t = got[:, :3], got[:, 3]
    R64, t64, s, ca, cb = _procrustes64(a, b, w)
    if unique and float(s[1]) > 0:
        n = a.shape[0]
        kappa = float(s[0] / (s[1] + s[2]))
        ext = float((a.to(F64) - ca).abs().max().clamp_min(1e-30))
        off = float(ca.abs().max())
        br = 2.0 ** -23 + 4 * kappa * (n + 10) * 2.0 ** -52 * (1 + off / ext)
        eR = (R - R64).abs().max()
        assert float(eR) <= br, f"{what}: R err {float(eR):.3e} > {br:.3e} (kappa {kappa:.2e})"
        bt = br * (R64.abs() @ ca.abs() + cb.abs()) + 2.0 ** -23 * t64.abs() + 2.0 ** -60
        et = (t - t64).abs()
        assert bool((et <= bt).all()), f"{what}: t err {et.tolist()} > {bt.tolist()}"
    else:
        # R is not determined: a rotation, and the weighted cost of the float64 optimum, up to 1e-6 relative and
        # the float32 rounding of R and t (|dR| <= 2^-24 per element)
        assert float((R @ R.t() - torch.eye(3, dtype=F64)).abs().max()) <= 1e-6, f"{what}: R R^T != I"
        assert abs(float(torch.det(R)) - 1.0) <= 1e-6, f"{what}: det R = {float(torch.det(R))}"
        c64 = _cost(a, b, w, R64, t64)
        c = _cost(a, b, w, R, t)
        ww = torch.ones(a.shape[0], dtype=F64) if w is None else w.to(F64)
        dr = float(((3 * 2.0 ** -24 * a.to(F64).abs().sum(1) + 2.0 ** -23 * float(t64.abs().max()) + 2.0 ** -23 *
                     b.to(F64).abs().max()) ** 2 * 3 * ww).sum())
        allow = 1e-6 * c64 + 2 * math.sqrt(max(c64, 0.0) * dr) + dr + 1e-30
        assert c - c64 <= allow, f"{what}: cost {c:.6e} vs optimum {c64:.6e} (allow {allow:.3e})"


def test_procrustes_geometries_one_batch(device):
    """All cases in one call, with empty segments between them (pair_cu): the kernel returns [I | 0] for an empty
    set, where the reference's mean of no points is NaN -- that difference is deliberate."""
    g = torch.Generator().manual_seed(90)
    cases = [(k, *_pcase(k, g)) for k in PCASES]
    # w=None sets join a weighted batch with weight 1 (the same sums)
    A, Bv, W, cu, slots = [], [], [], [0], []
    for idx, (kind, a, b, w, unique) in enumerate(cases):
        if idx % 4 == 1:
            cu.append(cu[-1])                          # an empty segment before this set
            slots.append(None)
        A.append(a)
        Bv.append(b)
        W.append(torch.ones(a.shape[0]) if w is None else w)
        cu.append(cu[-1] + a.shape[0])
        slots.append(idx)
    cu.append(cu[-1])
    slots.append(None)
    pc = torch.tensor(cu, dtype=torch.int32, device=device)
    out = ops.weighted_procrustes(torch.cat(A).to(device), torch.cat(Bv).to(device), torch.cat(W).to(device), pc).cpu()
    ident = torch.cat([torch.eye(3), torch.zeros(3, 1)], 1)
    for s, idx in enumerate(slots):
        if idx is None:
            assert torch.equal(out[s], ident), f"empty segment {s}: {out[s]}"
            continue
        kind, a, b, w, unique = cases[idx]
        ww = torch.ones(a.shape[0]) if w is None else w
        _check_pose(out[s], a, b, ww, unique, kind)
    # and the unweighted entry point (w = None: plain means) on the unweighted sets
    for kind in ("cube", "unweighted", "off1e4", "planar_1e-6"):
        a, b, w, unique = _pcase(kind, torch.Generator().manual_seed(91))
        pc = torch.tensor([0, a.shape[0]], dtype=torch.int32, device=device)
        out = ops.weighted_procrustes(a.to(device), b.to(device), None, pc).cpu()
        _check_pose(out[0], a, b, None, unique, f"{kind} w=None")


def _res_bound(pose, a, b):
    R, t = pose[:, :3].to(F64), pose[:, 3].to(F64)
    a64, b64 = a.to(F64), b.to(F64)
    d = b64 - (a64 @ R.t() + t)
    res = d.norm(dim=1)
    # per component: 4 roundings of terms of size |x R| + |t| and 1 of |b|; the squares, sum and sqrt: 4 ulp of res
    mag = ((a64.abs() @ R.abs().t() + t.abs() + b64.abs()) * 5 * U).norm(dim=1)
    return res, mag + 4 * U * res


@pytest.mark.parametrize("n", [1, 63, 64, 65, 5000])
def test_pose_residuals_and_scores(device, n):
    g = torch.Generator().manual_seed(95 + n)
    poses = []
    for h in range(7):
        poses.append(torch.cat([_rot(g), torch.randn(3, 1, generator=g, dtype=F64) * 1e3], 1).float())
    poses = torch.stack(poses)
    a = (torch.randn((n, 3), generator=g) * 30 + 1e3)
    b = (a.to(F64) @ poses[0, :, :3].to(F64).t() + poses[0, :, 3].to(F64)).float() + torch.randn((n, 3), generator=g)
    da, db, dp = a.to(device), b.to(device), poses.to(device)
    for nh in (1, 3, 5, 7):                              # hypothesis counts off a multiple of 4
        sc = ops.pose_scores(dp[:nh], da, db).cpu().to(F64)
        for h in range(nh):
            res, bnd = _res_bound(poses[h], a, b)
            ref = float(res.mean())
            allow = float(bnd.mean()) + (n / 64 + 8) * U * ref + 2 * U * ref
            assert abs(float(sc[h]) - ref) <= allow, f"pose_scores n={n} h={h}: {float(sc[h]):.9e} vs {ref:.9e}"
    # residuals: one pose per set, empty sets inside pair_cu
    cut = [0, 0, n // 3, n // 3, n, n]
    pc = torch.tensor(cut, dtype=torch.int32, device=device)
    res = ops.pose_residuals(dp[:5], da, db, pc).cpu().to(F64)
    for s in range(5):
        if cut[s + 1] == cut[s]:
            continue
        sl = slice(cut[s], cut[s + 1])
        ref, bnd = _res_bound(poses[s], a[sl], b[sl])
        err = (res[sl] - ref).abs()
        assert bool((err <= bnd).all()), f"pose_residuals n={n} set {s}: err {float(err.max()):.3e}"


# ---- 4. backward at the new dispatch shapes ---------------------------------------------------------------------- #
def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


@pytest.mark.parametrize("pairs", [[(1000, 1000), (40, 4)], [(1500, 2000), (9, 7)], [(2100, 2100), (3, 3)],
                                   [(300, 290), (64, 1), (5, 2)]],
                         ids=["v4", "v8", "generic", "col_lse"])
def test_sinkhorn_backward_double_potentials(device, pairs):
    """spr_sinkhorn_bwd re-runs the forward with double potentials: k_row_lse_v<4 / 8, double> up to max_m 2048,
    the generic k_row_lse<double> above, k_col_lse<double> when min_m < 4.  d feat, d alpha, d beta against float64
    autograd at the existing backward test's relative bound (5e-5)."""
    g = torch.Generator().manual_seed(200 + pairs[0][1])
    d = 64
    fs = [torch.randn((n, d), generator=g) * 0.8 for n, _ in pairs]
    ft = [torch.randn((m, d), generator=g) * 0.8 for _, m in pairs]
    xt = [torch.randn((m, 3), generator=g) for _, m in pairs]
    xs = [torch.randn((n, 3), generator=g) for n, _ in pairs]
    feat, cu_host = _pack(fs, ft)
    cu = torch.tensor(cu_host, dtype=torch.int32, device=device)
    tsrc = sum(n for n, _ in pairs)
    gw, gt = synthetic.rand((tsrc,), 201), synthetic.rand((tsrc, 3), 202)
    df = feat.clone().to(device).requires_grad_(True)
    al = torch.tensor(0.9, device=device, requires_grad=True)
    be = torch.tensor(1.1, device=device, requires_grad=True)
    w, that = ops.sinkhorn_correspondences(df, torch.cat(xs + xt).to(device), cu, cu_host, len(pairs), al, be, 3)
    ((w * gw.to(device)).sum() + (that * gt.to(device)).sum()).backward()
    cf = feat.double().requires_grad_(True)
    ca = torch.tensor(0.9, dtype=F64, requires_grad=True)
    cb = torch.tensor(1.1, dtype=F64, requires_grad=True)
    B = len(pairs)
    loss = 0.0
    affs = []
    for k in range(B):       # oracle.sinkhorn_soft_correspondences in potential form, the affinity kept for its gradient
        a_ = cf[cu_host[k]:cu_host[k + 1]]
        b_ = cf[cu_host[B + k]:cu_host[B + k + 1]]
        aff = -(torch.clamp(a_ @ b_.t() / math.sqrt(d), min=0.0) - torch.nn.functional.softplus(ca)) / (cb.exp() + 0.02)
        aff.retain_grad()
        affs.append(aff)
        u_ = torch.zeros(aff.shape[0], dtype=F64)
        v_ = torch.zeros(aff.shape[1], dtype=F64)
        for _ in range(3):
            u_ = torch.log1p(torch.exp(aff - v_[None, :]).sum(1))
            v_ = torch.log1p(torch.exp(aff - u_[:, None]).sum(0))
        P = torch.exp(aff - u_[:, None] - v_[None, :])
        wr = P.sum(1)
        tr = P @ xt[k].double() / (wr[:, None] + 1e-6)
        s = slice(cu_host[k], cu_host[k + 1])
        loss = loss + (wr * gw[s].double()).sum() + (tr * gt[s].double()).sum()
    loss.backward()
    assert _rel(df.grad, cf.grad) <= 5e-5, f"sinkhorn dfeat {_rel(df.grad, cf.grad):.2e}"
    # d alpha = sig(alpha) / den sum dA_ij, d beta = -e^beta / den sum dA_ij A_ij: sums of N x M float32 terms that
    # cancel down to the slack mass (at 1000 x 1000, |sum| ~ 1e-2 sum |.|).  Bound: 5e-5 relative (the existing
    # test's), or 16 ulp of every term (the float32 chain that forms dA_ij) summed by magnitude
    den = math.exp(1.1) + 0.02
    sig = 1.0 / (1.0 + math.exp(-0.9))
    mag_a = sum(float(a.grad.abs().sum()) for a in affs) * sig / den
    mag_b = sum(float((a.grad * a.detach()).abs().sum()) for a in affs) * math.exp(1.1) / den
    for got, ref, mag, nm in ((al.grad, ca.grad, mag_a, "alpha"), (be.grad, cb.grad, mag_b, "beta")):
        err = abs(float(got) - float(ref))
        assert err <= max(5e-5 * abs(float(ref)), 16 * U * mag), f"sinkhorn d{nm}: {float(got):.9e} vs {float(ref):.9e}"


@pytest.mark.parametrize("name", ["tiny", "quads", "m1025"])
def test_dual_softmax_backward_shapes(device, name):
    fs, ft = _features(name, "unit", seed=2)
    feat, cu_host = _pack(fs, ft)
    cu = torch.tensor(cu_host, dtype=torch.int32, device=device)
    T = feat.shape[0]
    gv = synthetic.rand((T,), 210)
    B = len(fs)
    side = torch.zeros(T, dtype=torch.bool)             # the tokens that carry a match
    for k, (a_, b_) in enumerate(zip(fs, ft)):
        n, m = a_.shape[0], b_.shape[0]
        if n > m:
            side[cu_host[B + k]:cu_host[B + k + 1]] = True
        else:
            side[cu_host[k]:cu_host[k + 1]] = True
    gv = gv * side
    df = feat.clone().to(device).requires_grad_(True)
    val, ind = ops.match_dualsoftmax(df, cu, cu_host, len(fs))
    (val * gv.to(device)).sum().backward()
    cf = feat.double().requires_grad_(True)
    loss = 0.0
    for k in range(B):
        a_ = cf[cu_host[k]:cu_host[k + 1]]
        b_ = cf[cu_host[B + k]:cu_host[B + k + 1]]
        n, m = a_.shape[0], b_.shape[0]
        _, _, attn = O.dual_softmax_match(a_, b_)
        # the gradient flows through the kernel's own choice of index (ties decided the same way)
        if n > m:
            i = ind[cu_host[B + k]:cu_host[B + k] + m].long().cpu()
            loss = loss + (attn[i, torch.arange(m)] * gv[cu_host[B + k]:cu_host[B + k] + m].double()).sum()
        else:
            i = ind[cu_host[k]:cu_host[k] + n].long().cpu()
            loss = loss + (attn[torch.arange(n), i] * gv[cu_host[k]:cu_host[k] + n].double()).sum()
    loss.backward()
    assert _rel(df.grad, cf.grad) <= 5e-5, f"dual softmax dfeat {name}: {_rel(df.grad, cf.grad):.2e}"


def _pose64(a, b, w):
    R, t, _, _, _ = _procrustes64(a, b, w)
    return torch.cat([R, t[:, None]], 1)


@pytest.mark.parametrize("kind", ["off1e3", "wsum_tiny", "cube", "tetra"])
def test_procrustes_backward_geometries(device, kind):
    """Large offsets and weight sums below the clamp against float64 autograd; the isotropic sets (equal singular
    values: torch's SVD gradient is undefined there, the kernel's polar-factor formula is not) against central
    differences of the float64 solve."""
    g = torch.Generator().manual_seed(300)
    a, b, w, _ = _pcase(kind, g)
    if w is None:
        w = torch.ones(a.shape[0])
    if kind in ("cube", "tetra"):
        # noise-free, R and t do not depend on w (d w = 0 up to the float32 rounding of b): near-equal singular
        # values with a non-trivial d w need a little noise (1e-3: torch's SVD gradient would divide by ~1e-3)
        b = b + 1e-3 * torch.randn(b.shape, generator=g)
    go = synthetic.rand((1, 3, 4), 301)
    pc = torch.tensor([0, a.shape[0]], dtype=torch.int32, device=device)
    la, lb, lw = (t.clone().to(device).requires_grad_(True) for t in (a, b, w))
    ops.weighted_procrustes(la, lb, lw, pc).backward(go.to(device))
    if kind in ("cube", "tetra"):
        h = 1e-6
        refs = []
        for src in (a, b, w):
            base = src.to(F64)
            gr = torch.zeros_like(base)
            flat = gr.view(-1)
            for i in range(base.numel()):
                p, m_ = base.clone(), base.clone()
                p.view(-1)[i] += h
                m_.view(-1)[i] -= h
                args_p = [p if x is src else x.to(F64) for x in (a, b, w)]
                args_m = [m_ if x is src else x.to(F64) for x in (a, b, w)]
                flat[i] = float(((_pose64(*args_p) - _pose64(*args_m)) * go[0].double()).sum()) / (2 * h)
            refs.append(gr)
    else:
        ca, cb, cw = (t.double().requires_grad_(True) for t in (a, b, w))
        (_pose64(ca, cb, cw) * go[0].double()).sum().backward()
        refs = [ca.grad, cb.grad, cw.grad]
    for got, ref, nm in zip((la.grad, lb.grad, lw.grad), refs, "abw"):     # test_gpu_backward's Procrustes bound
        assert _rel(got, ref) <= 2e-5, f"procrustes {kind} d{nm}: {_rel(got, ref):.2e}"


# ---- 5. loss terms (forward) ------------------------------------------------------------------------------------ #
def _infonce_case(n, m, d, seed, r_p=0.2, r_n=0.4):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn((n, d), generator=g) * 0.3
    p = torch.randn((m, d), generator=g) * 0.3
    xt = torch.rand((m, 3), generator=g)
    xs = torch.rand((n, 3), generator=g)
    W = synthetic.rand((d, d), seed + 1, -0.05, 0.05)
    return a, p, xs, xt, W


def _infonce64(a, p, xs, xt, W, r_p, r_n):
    """oracle.torch_oracle.infonce with the nearest positive chosen as the LOWEST index among equal distances
    (argmin's documented order; topk leaves ties unspecified) and distances as direct differences."""
    w_triu = torch.triu(W)
    logits = a @ (w_triu + w_triu.t()) @ p.t()
    dist = (xs[:, None, :] - xt[None, :, :]).norm(dim=2)
    idx1 = dist.argmin(1, keepdim=True)
    mask = dist.gather(1, idx1)[:, 0] < r_p
    ignore = dist < r_n
    ignore.scatter_(1, idx1, False)
    logits = logits.masked_fill(ignore, -math.inf)
    loss = -logits.gather(1, idx1)[:, 0] + torch.logsumexp(logits, 1)
    return loss[mask].sum() / mask.sum()


def _infonce_check(device, a, p, xs, xt, W, r_p, r_n, what):
    pose = torch.tensor([[1.0, 0, 0, 0.0], [0, 1, 0, 0.0], [0, 0, 1, 0.0]])
    got = float(ops.infonce_pair(a.to(device), p.to(device), xs.to(device), pose.to(device), xt.to(device),
                                 W.to(device), r_p, r_n))
    ref = float(_infonce64(a.double(), p.double(), xs.double(), xt.double(), W.double(), r_p, r_n))
    if math.isnan(ref):
        assert math.isnan(got), f"{what}: {got} where the reference is NaN (no anchor has a positive)"
        return
    # logits: products of length d twice (a W_sym, then p): relative to sum |a||W||p|; the per-row log-sum-exp
    # moves by at most the largest logit error; the mean adds float64 sums of float32 terms
    d = a.shape[1]
    Ws = torch.triu(W.double()) + torch.triu(W.double()).t()
    mag = float((a.double().abs() @ Ws.abs() @ p.double().abs().t()).max())
    allow = 2 * (2 * _coef(d) * mag) + 8 * U * (abs(ref) + 1) + (max(a.shape[0], p.shape[0]) / 16 + 40) * U
    assert abs(got - ref) <= allow, f"{what}: {got:.9e} vs {ref:.9e} (allow {allow:.2e})"


@pytest.mark.parametrize("n,m", [(1, 1), (63, 65), (65, 63), (2000, 63), (63, 2000), (2000, 2000)])
@pytest.mark.parametrize("d", [32, 256])
def test_infonce_shapes(device, n, m, d):
    a, p, xs, xt, W = _infonce_case(n, m, d, 400 + n + m + d)
    if n == 1:
        xs = xt[:1] + 0.01                 # the one anchor has a positive
    _infonce_check(device, a, p, xs, xt, W, 0.2, 0.4, f"infonce {n}x{m} d={d}")


def test_infonce_edges(device):
    """No anchor with a positive (0 / 0 = NaN like the reference); anchors exactly at r_p and r_n from a target
    (strict comparisons: not a positive, not ignored); equal-distance nearest positives (the lowest index)."""
    d = 32
    a, p, xs, xt, W = _infonce_case(40, 50, d, 450)
    _infonce_check(device, a, p, xs + 100.0, xt, W, 0.2, 0.4, "infonce no positive")
    # exact distances: targets on the axes at 0.25 (binary fractions: |d| is exact in float32 and float64)
    xt2 = xt.clone() * 0 + 10.0
    xt2[0] = torch.tensor([0.25, 0.0, 0.0])
    xt2[1] = torch.tensor([-0.25, 0.0, 0.0])       # equidistant with target 0 from anchors on the y-z plane
    xt2[2] = torch.tensor([0.0, 0.5, 0.0])
    xs2 = torch.zeros((40, 3))                     # rows 0::3 at the origin: 0.25 from targets 0 and 1, 0.5 from 2
    xs2[1::3, 0] = 0.125                           # nearer to 0 only (1 is 0.375 away: ignored at r_n = 0.5)
    xs2[2::3, 2] = 0.125                           # equidistant from 0 and 1: the lowest index, 0
    # r_p = 0.25, r_n = 0.5: the origin anchors are exactly at r_p (no positive) and exactly at r_n from target 2
    # (not ignored)
    _infonce_check(device, a, p, xs2, xt2, W, 0.25, 0.5, "infonce at r_p / r_n")
    # r_p = 0.3: the origin and (0, 0, 0.125) anchors have two equidistant positives
    _infonce_check(device, a, p, xs2, xt2, W, 0.3, 0.5, "infonce equidistant positives")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100000])
def test_bce_logits_mean_edges(device, n):
    g = torch.Generator().manual_seed(500 + n)
    x = torch.randn(n, generator=g) * 10
    x[::3] = 100.0
    x[1::5] = -100.0
    y = (torch.rand(n, generator=g) > 0.5).float()
    got = float(ops.bce_logits_mean(x.to(device), y.to(device)))
    ref = float(torch.nn.functional.binary_cross_entropy_with_logits(x.double(), y.double()))
    # each term: 4 float32 roundings of max(x, 0) - x y + log1p(exp(-|x|)) (sizes up to |x|), float64 sums
    allow = 4 * U * float((x.abs().double() + 1).mean()) + 1e-12
    assert abs(got - ref) <= allow + 2 * U * abs(ref), f"bce n={n}: {got:.9e} vs {ref:.9e}"


@pytest.mark.parametrize("n", [1, 257, 100000])
def test_transform_l1_far_coordinates(device, n):
    g = torch.Generator().manual_seed(600 + n)
    xyz = torch.randn((n, 3), generator=g) * 5 + 1e3
    R = _rot(g)
    pg = torch.cat([R, torch.randn(3, 1, generator=g, dtype=F64)], 1).float()
    pp = (pg.double() + 1e-3 * torch.randn((3, 4), generator=g, dtype=F64)).float()
    got = float(ops.transform_l1_pair(pg.to(device), pp.to(device), xyz.to(device)))
    x64 = xyz.double()
    ref = float((O.se3_transform(pg.double(), x64) - O.se3_transform(pp.double(), x64)).abs().mean())
    # two float32 transforms of a 1e3 point (4 roundings of terms up to |x||R| + |t| each), their difference
    mag = float((x64.abs() @ pg.double()[:, :3].abs().t() + pg.double()[:, 3].abs()).mean())
    allow = 2 * 5 * U * mag + 2 * U * ref
    assert abs(got - ref) <= allow, f"transform_l1 n={n}: {got:.9e} vs {ref:.9e} (allow {allow:.2e})"


def test_overlap_pool_edges(device):
    """Rows of shadow indices only (0 / 0 = NaN, as the reference's mean of nothing), a pool width of 1, indices
    equal to ns (shadow) or above, values clamped to [0, 1]."""
    ns = 50
    g = torch.Generator().manual_seed(700)
    ov = torch.rand(ns, generator=g)
    ov[3] = 1.0
    for w in (1, 7):
        idx = torch.randint(0, ns + 1, (40, w), generator=g)
        idx[0] = ns
        idx[1] = ns
        idx[2, 0] = 3
        got = ops.overlap_pool(ov.to(device), idx.to(torch.int32).to(device), ns).cpu().to(F64)
        ext = torch.cat([ov.double(), torch.zeros(1, dtype=F64)])
        valid = (idx < ns).double()
        ref = (ext[idx] * valid).sum(1) / valid.sum(1)
        nan = torch.isnan(ref)
        assert bool(nan[:2].all()) and torch.equal(torch.isnan(got), nan), f"w={w}: NaN rows differ"
        err = (got[~nan] - ref[~nan].clamp(0, 1)).abs()
        assert bool((err <= (w + 2) * U * ref[~nan].abs() + 1e-30).all()), f"w={w}: err {float(err.max()):.3e}"
