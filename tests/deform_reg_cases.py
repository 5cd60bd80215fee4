"""The regulariser of deformable KPConv (include/spr.h, spr_deform_reg) restated in plain torch (any dtype; the tests
use float64) on the inputs of tests/deform_cases.py: all eight CASES, modulated off and on.

    reg_ref(...)        (value, fit, rep, m [nq, K]) of given offset features, differentiable in them
    ref64(case, ...)    float64 values and gradients of a case: at the offset features, and through the restated offset
                        convolution (kpconv_modes_cases.kpconv_ref + bias) at its weights, bias and input
    argmin_gap(case)    the input condition below, as a number;  check_gap(case) asserts it

Input condition (asserted by every test that compares a gradient, never worked around), float64: over the (row, kernel
point) entries of rows with at least two real neighbours, (second-smallest - smallest real d2) / e^2 >= GAP_MIN = 5e-5.
The minimum's gradient jumps where the argmin changes; float32 rounding of d2 / e^2 at these coordinates is about 1e-6,
so the condition leaves a 50 x margin.  The squared hinge of the repulsive term is C1 and needs no condition.  No row
or entry is excluded from any comparison.
"""
import torch

import deform_cases as dc
import kpconv_modes_cases as kc

GAP_MIN = 5e-5
R_DEFAULT = 1.2
MOD = [False, True]
mod_id = lambda m: "modulated" if m else "plain"
_cache = {}


def _geometry(q, s, idx, kp, extent, of):
    K, ns = kp.shape[0], s.shape[0]
    idx = idx.long()
    valid = (idx >= 0) & (idx < ns)
    safe = torch.where(valid, idx, torch.zeros_like(idx))
    D = kp + extent * of[:, :3 * K].reshape(-1, K, 3)                                  # [n, p, 3]
    y = s[safe] - q.unsqueeze(1)                                                       # [n, k, 3]
    d2 = ((y.unsqueeze(2) - D.unsqueeze(1)) ** 2).sum(3)                               # [n, k, p]
    d2 = torch.where(valid.unsqueeze(2), d2, torch.full_like(d2, float('inf')))        # a shadow never takes part
    return D, d2, valid


def reg_ref(q, s, idx, kp, extent, of, repulse_extent=R_DEFAULT):
    """(value, fit, rep, m): the contract of include/spr.h.  In the repulsive term the other kernel points are
    constants; a pair at distance 0 has the value R^2 and no gradient."""
    nq, K = q.shape[0], kp.shape[0]
    D, d2, valid = _geometry(q, s, idx, kp, extent, of)
    m = torch.where(valid.any(1, keepdim=True), d2.min(1)[0], torch.zeros_like(D[:, :, 0]))    # no real entry: 0
    fit = (m / extent ** 2).sum() / (nq * K)
    L = D / extent
    sq = ((L.unsqueeze(2) - L.detach().unsqueeze(1)) ** 2).sum(3)                      # [n, i, j]
    pos = sq > 0
    dist = torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))
    off_diag = ~torch.eye(K, dtype=torch.bool).unsqueeze(0)
    hinge = torch.clamp(dist - repulse_extent, max=0.0) * off_diag.to(sq.dtype)
    rep = (hinge ** 2).sum() / (nq * K)
    return 2 * fit + rep, fit, rep, m


def ref64(case, repulse_extent=R_DEFAULT, offset_features=None):
    """dict of float64 results.  offset_features given: value, fit, rep, m, d_of.  Otherwise the offsets are the
    restated offset convolution + bias, and d_off_w, d_off_b, dx (the gradient at the convolution's input) come too."""
    f = lambda k: case[k].double()
    if offset_features is not None:
        of = offset_features.double().clone().requires_grad_(True)
        leaves = {}
    else:
        leaves = {k: f(k).requires_grad_(True) for k in ("x", "off_w", "off_b")}
        of = kc.kpconv_ref(f('q'), f('s'), case['idx'], leaves["x"], leaves["off_w"], f('off_kp'), case['extent']) \
            + leaves["off_b"]
        of.retain_grad()
    value, fit, rep, m = reg_ref(f('q'), f('s'), case['idx'], f('kp'), case['extent'], of, repulse_extent)
    value.backward()
    out = dict(value=value.detach(), fit=fit.detach(), rep=rep.detach(), m=m.detach(), d_of=of.grad,
               offset_features=of.detach())
    if leaves:
        out.update(d_off_w=leaves["off_w"].grad, d_off_b=leaves["off_b"].grad, dx=leaves["x"].grad)
    return out


def argmin_gap(case, offset_features):
    """min over (row with >= 2 real neighbours, kernel point) of (second-smallest - smallest real d2) / e^2; inf when no
    row has two."""
    f = lambda k: case[k].double()
    _, d2, valid = _geometry(f('q'), f('s'), case['idx'], f('kp'), case['extent'], offset_features.double())
    rows = valid.sum(1) >= 2
    if not bool(rows.any()):
        return float('inf')
    two = torch.topk(d2[rows], 2, dim=1, largest=False)[0]                             # [rows, 2, p]
    return float(((two[:, 1] - two[:, 0]) / case['extent'] ** 2).min())


def check_gap(case, offset_features):
    gap = argmin_gap(case, offset_features)
    assert gap >= GAP_MIN, f"two neighbours within {gap:.2e} e^2 of the minimum: pick another offset seed"
    return gap


def case_of(name, modulated):
    """(case, ref) with ref = ref64 at the float32-rounded offsets of the float64 offset convolution (what the kernel
    under test is handed), computed once and left unchanged; the argmin gap is asserted."""
    key = (name, bool(modulated))
    if key not in _cache:
        case = dc.make_case(name, modulated)
        of = ref64(case)["offset_features"].float()
        check_gap(case, of)
        _cache[key] = (case, ref64(case, offset_features=of))
    return _cache[key]


COINCIDENT_SEED = 41


def coincident_case():
    """(case, of, ref): the seven-kernel-point case with hand-built offsets that put kernel points 1 and 2 of query 1 (a
    row with real neighbours) on one spot, exactly: kp[2] is set to kp[1] and the two points get the same offsets in
    that row alone (every other row draws them apart).  The pair then counts R^2 twice in the value and contributes
    nothing to the gradient."""
    if "coincident" not in _cache:
        import numpy as np
        case = dict(dc.make_case("simple 7 kernel points 32-32", False))
        kp = case["kp"].clone()
        kp[2] = kp[1]
        case["kp"] = kp
        rng = np.random.default_rng(COINCIDENT_SEED)
        of = torch.from_numpy(rng.uniform(-0.3, 0.3, (case["q"].shape[0], 3 * kp.shape[0])).astype(np.float32))
        of[1, 6:9] = of[1, 3:6]
        check_gap(case, of)
        _cache["coincident"] = (case, of, ref64(case, offset_features=of))
    return _cache["coincident"]


def chain_of(name, modulated):
    """(case, ref) with ref = ref64 through the restated offset convolution, computed once; the gap is asserted."""
    key = (name, bool(modulated), "chain")
    if key not in _cache:
        case = dc.make_case(name, modulated)
        ref = ref64(case)
        check_gap(case, ref["offset_features"])
        _cache[key] = (case, ref)
    return _cache[key]
