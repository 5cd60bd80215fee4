"""Deformable / modulated KPConv (linear influence, sum aggregation) restated in plain torch (any dtype; the tests use
float64), and the inputs of tests/test_deform_host.py, tests/test_gpu_deform.py and tests/test_gpu_deform_guarded.py.

    kpconv_deform_ref(...)   KPConv.forward with deformable=True (kpconv_blocks.py:309-412 of the reference);
                             differentiable in x, the weights, the offset convolution's weights and the offset bias (or
                             in given offset features)
    make_case(name, mod)     seeded inputs: kpconv_modes_cases.make_case at search radius R with kernel points of radius
                             R / 2 and extent 0.8 R / 2 -- rows twice as wide as the kernel, as in a deformable level
    conditions(...)          the input conditions below, as numbers;  check_conditions(...) asserts them

Input conditions (asserted by every test that uses a case, never worked around), float64:
    range gap       min over valid (n, k) of |min_p sqrt(d2) / e - 1| >= GAP_MIN: the in-range cut, hence the count,
                    depends on nothing finer
    distance floor  min sqrt(d2) / e >= DIST_MIN: the offset gradient divides by it
    row sums        kpconv_modes_cases.min_row_sum >= SUM_MIN
    in-range share  of the valid neighbours, in [SHARE_LO, SHARE_HI] for cases with more than two queries: the cut is
                    exercised
"""
import numpy as np
import torch

import kpconv_modes_cases as kc

GAP_MIN = 1e-4
DIST_MIN = 1e-3
SUM_MIN = kc.SUM_MIN
SHARE_LO, SHARE_HI = 0.2, 0.8
FAR = 1e6               # the reference's shadow point

# name -> (make_case arguments; radius is the SEARCH radius R), offset seed for modulated off / on
CASES = {
    "nq1 k1 32-32": (dict(seed=21, nq=1, kmax=1, cin=32, cout=32), (900, 900)),
    "nq37 k5 64-64": (dict(seed=22, nq=37, kmax=5, cin=64, cout=64), (900, 900)),
    "nq130 k33 128-128": (dict(seed=23, nq=130, kmax=33, cin=128, cout=128), (900, 901)),
    "nq130 k70 64-256 int64 unsorted": (dict(seed=24, nq=130, kmax=70, cin=64, cout=256, radius=0.35, shuffle=True,
                                             index_dtype=torch.int64), (901, 900)),
    "strided nq37 ns130 k33 32-64": (dict(seed=25, nq=37, ns=130, kmax=33, cin=32, cout=64, radius=0.3), (901, 900)),
    "simple 48-40": (dict(seed=27, nq=37, kmax=5, cin=48, cout=40), (900, 900)),
    "simple cin1 1-32": (dict(seed=26, nq=37, kmax=5, cin=1, cout=32), (900, 900)),
    "simple 7 kernel points 32-32": (dict(seed=28, nq=37, kmax=33, cin=32, cout=32, n_kp=7, radius=0.3), (900, 900)),
}
BACKWARD_CASES = ("nq37 k5 64-64", "simple 48-40", "nq130 k70 64-256 int64 unsorted")


def offset_dim(n_kp, modulated):
    return (4 if modulated else 3) * n_kp


def kpconv_deform_ref(q_pts, s_pts, neighb_inds, x, weights, kernel_points, kp_extent, modulated, off_w=None,
                      off_kp=None, off_b=None, offset_features=None):
    """(out [nq, cout], aux).  The offset features are given, or the rigid offset convolution (its own kernel points
    off_kp) plus bias.  aux: offset_features, deformed_KP [nq, K, 3], min_d2 [nq, K], in_range [nq, kmax], count [nq]."""
    K = kernel_points.shape[0]
    of = offset_features
    if of is None:
        of = kc.kpconv_ref(q_pts, s_pts, neighb_inds, x, off_w, off_kp, kp_extent) + off_b
    ns = s_pts.shape[0]
    idx = neighb_inds.long()
    valid = (idx >= 0) & (idx < ns)
    safe = torch.where(valid, idx, torch.zeros_like(idx))
    D = kernel_points + kp_extent * of[:, :3 * K].reshape(-1, K, 3)                     # [n, p, 3]
    m = 2 * torch.sigmoid(of[:, 3 * K:4 * K]) if modulated else torch.ones_like(of[:, :K])
    far = torch.full_like(s_pts[:1], FAR)
    y = torch.where(valid.unsqueeze(2), s_pts[safe], far) - q_pts.unsqueeze(1)          # [n, k, 3]
    d2 = ((y.unsqueeze(2) - D.unsqueeze(1)) ** 2).sum(3)                                # [n, k, p]
    in_range = (d2 < kp_extent ** 2).any(2) & valid
    h = torch.clamp(1 - torch.sqrt(d2) / kp_extent, min=0.0) * in_range.unsqueeze(2).to(d2.dtype)
    nx = x[safe] * valid.unsqueeze(2).to(x.dtype)
    wf = torch.einsum('nkp,nkc->npc', h, nx) * m.unsqueeze(2)
    out = torch.einsum('npc,pco->no', wf, weights)
    count = ((nx.sum(-1) > 0.0) & in_range).sum(-1).clamp(min=1)
    aux = dict(offset_features=of, deformed_KP=D, min_d2=d2.min(1)[0], in_range=in_range, count=count, d2=d2, valid=valid)
    return out / count.unsqueeze(1).to(out.dtype), aux


def make_case(name, modulated, offset_seed=None):
    """dict(q, s, idx, x, w, kp, extent, off_w, off_kp, off_b, modulated): float32 / index CPU tensors."""
    args, seeds = CASES[name]
    case = kc.make_case(**args)
    R = args.get('radius', 0.2)
    n_kp = args.get('n_kp', 15)
    cin = args['cin']
    case['kp'] = kc.kernel_points_15(R / 2, args['seed'] + 1000)[:n_kp].contiguous()
    case['off_kp'] = kc.kernel_points_15(R / 2, args['seed'] + 2000)[:n_kp].contiguous()
    case['extent'] = float(0.8 * R / 2)
    rng = np.random.default_rng(seeds[int(bool(modulated))] if offset_seed is None else offset_seed)
    od = offset_dim(n_kp, modulated)
    case['off_w'] = torch.from_numpy((rng.uniform(-1, 1, (n_kp, cin, od)) * 0.5 / np.sqrt(n_kp * cin)).astype(np.float32))
    case['off_b'] = torch.from_numpy(rng.uniform(-0.1, 0.1, (od,)).astype(np.float32))
    case['modulated'] = bool(modulated)
    return case


def ref64(case, go=None, offset_features=None):
    """float64 (out, aux) of a case; with go (the output gradient) also grads = dict(dx, dw, d_off_w, d_off_b, d_of) by
    autograd (d_of: the gradient at the offset features)."""
    f = lambda k: case[k].double()
    x, w, ow, ob = f('x'), f('w'), f('off_w'), f('off_b')
    if go is not None:
        for t in (x, w, ow, ob):
            t.requires_grad_(True)
    if offset_features is None:
        of = kc.kpconv_ref(f('q'), f('s'), case['idx'], x, ow, f('off_kp'), case['extent']) + ob
    else:
        of = offset_features.double()
    if go is not None and of.requires_grad:
        of.retain_grad()
    out, aux = kpconv_deform_ref(f('q'), f('s'), case['idx'], x, w, f('kp'), case['extent'], case['modulated'],
                                 offset_features=of)
    if go is None:
        return out, aux
    out.backward(go.double())
    grads = dict(dx=x.grad, dw=w.grad, d_off_w=ow.grad, d_off_b=ob.grad, d_of=of.grad)
    return out.detach(), {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in aux.items()}, grads


def conditions(case, aux=None):
    """dict(gap, floor, row_sum, share, n_valid) in float64 (see the module docstring)."""
    if aux is None:
        _, aux = ref64(case)
    d = torch.sqrt(aux['d2'].detach()) / case['extent']
    valid = aux['valid']
    if not bool(valid.any()):
        return dict(gap=float('inf'), floor=float('inf'), row_sum=kc.min_row_sum(case['x']), share=None, n_valid=0)
    dmin = d.min(2)[0][valid]
    return dict(gap=float((dmin - 1).abs().min()), floor=float(d[valid].min()), row_sum=kc.min_row_sum(case['x']),
                share=float(aux['in_range'][valid].double().mean()), n_valid=int(valid.sum()))


def check_conditions(case, aux=None):
    c = conditions(case, aux)
    assert c['gap'] >= GAP_MIN, f"a neighbour within {c['gap']:.2e} e of the range cut: pick another offset seed"
    assert c['floor'] >= DIST_MIN, f"a neighbour within {c['floor']:.2e} e of a kernel point: pick another offset seed"
    assert c['row_sum'] >= SUM_MIN, f"a feature row sums to {c['row_sum']:.2e}: pick another seed"
    if case['q'].shape[0] > 2:
        assert SHARE_LO <= c['share'] <= SHARE_HI, f"in-range share {c['share']:.2f}: the cut is not exercised"
    return c


# The reference fixture (tests/golden/kpconv_deform.npz, scripts/gen_kpconv_deform_golden.py): the golden shape of
# kpconv_modes_cases (96 points, rows of 20, 32 -> 64) at the deformable geometry above, modulated off / on; both
# convolutions' kernel points are the reference's own draws and are stored in the file.
GOLDEN_R = 0.2
GOLDEN_OFFSET_SEED = 900
GOLDEN_DW_STEP = kc.GOLDEN_DW_STEP


def golden_case(modulated, kp=None, off_kp=None):
    case = kc.golden_case()
    cin, n_kp = kc.GOLDEN['cin'], 15
    case['kp'] = kc.kernel_points_15(GOLDEN_R / 2, kc.GOLDEN['seed'] + 1000) if kp is None else kp
    case['off_kp'] = kc.kernel_points_15(GOLDEN_R / 2, kc.GOLDEN['seed'] + 2000) if off_kp is None else off_kp
    case['extent'] = float(0.8 * GOLDEN_R / 2)
    rng = np.random.default_rng(GOLDEN_OFFSET_SEED)
    od = offset_dim(n_kp, modulated)
    case['off_w'] = torch.from_numpy((rng.uniform(-1, 1, (n_kp, cin, od)) * 0.5 / np.sqrt(n_kp * cin)).astype(np.float32))
    case['off_b'] = torch.from_numpy(rng.uniform(-0.1, 0.1, (od,)).astype(np.float32))
    case['modulated'] = bool(modulated)
    return case


# ---- the encoder fixture (tests/golden/deform_encoder.npz, scripts/gen_kpconv_deform_golden.py) --------------------------
# name -> (architecture, modulated) on the 3DMatch config.  'last' / 'last modulated': the last level's conv search takes
# the deformable radius (a deformable block among its blocks other than the last).  'quirk': the only deformable conv
# block is the LAST of its level, so that level's conv radius stays normal (the reference's layer_blocks[:-1]), and a
# deformable strided block widens its level's pool (and up-sampling) radius.
ENCODER_SEED = 4
_HEAD = ['simple', 'resnetb', 'resnetb_strided', 'resnetb', 'resnetb']
ENCODER_ARCHS = {
    "last": (_HEAD + ['resnetb_strided', 'resnetb_deformable', 'resnetb_deformable', 'resnetb'], False),
    "last modulated": (_HEAD + ['resnetb_strided', 'resnetb_deformable', 'resnetb_deformable', 'resnetb'], True),
    "quirk": (_HEAD + ['resnetb_deformable_strided', 'resnetb', 'resnetb', 'resnetb_deformable'], False),
}


def encoder_clouds():
    """Two overlapping clouds of about a hundred points each (the fixture stores them)."""
    from superpoints_registration_amd import synthetic
    src, tgt, _ = synthetic.make_pair(110, seed=31, extent=0.24, jitter=0.002)
    return np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
