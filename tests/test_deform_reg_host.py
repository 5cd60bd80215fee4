"""Host: the regulariser of deformable KPConv without a GPU -- its three config keys, the C ABI of spr_deform_reg (header,
export, binding, size query, host-side refusals), the optimizer's parameter groups under deform_lr_factor, and the
float64 restatement of tests/deform_reg_cases.py against a plain-loop numpy version of the contract."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import deform_cases as dc
import deform_reg_cases as rc
from superpoints_registration_amd import _lib, get_config, synthetic
from superpoints_registration_amd.kpconv import KPFEncoder
from superpoints_registration_amd.training import configure_optimizers

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spr.h")


# ---- config --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["3dmatch", "kitti", "modelnet"])
def test_the_three_keys_and_their_defaults(tag):
    cfg = get_config(tag)
    assert cfg.deform_fitting_power == 0.0 and cfg.repulse_extent == 1.2 and cfg.deform_lr_factor == 1.0
    cfg = get_config(tag, deform_fitting_power=1.0, repulse_extent=0.9, deform_lr_factor=0.1)
    assert cfg.deform_fitting_power == 1.0 and cfg.repulse_extent == 0.9 and cfg.deform_lr_factor == 0.1


def _encoder_config(name, **kw):
    arch, modulated = dc.ENCODER_ARCHS[name]
    return get_config('3dmatch', deformable_kpconv=True, architecture=list(arch), modulated=modulated, **kw)


def test_the_encoder_sets_the_blocks_flag_only_under_a_positive_power():
    from superpoints_registration_amd import deformable
    for power, want in ((0.0, False), (1.0, True)):
        enc = KPFEncoder(_encoder_config("last", deform_fitting_power=power), 256)
        blocks = [m for m in enc.modules() if isinstance(m, deformable.KPConvDeformable)]
        assert len(blocks) == 2 and all(m.keep_reg_inputs is want and m.reg_inputs is None for m in blocks)


def test_no_block_with_a_forward_gives_none():
    from superpoints_registration_amd import deform_reg
    enc = KPFEncoder(_encoder_config("last", deform_fitting_power=1.0), 256)
    assert deform_reg.p2p_fitting_regularizer(enc, 1.0, 1.2) is None                   # no forward yet
    assert deform_reg.p2p_fitting_regularizer(KPFEncoder(get_config('3dmatch'), 256), 1.0, 1.2) is None


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def _declared_args(name):
    text = open(HEADER).read()
    m = re.search(rf"\b{name}\(([^;]*?)\);", text)
    assert m, f"{name} is not declared in include/spr.h"
    return [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]


@pytest.mark.parametrize("name", ["spr_deform_reg", "spr_deform_reg_workspace_size"])
def test_declared_exported_and_bound_with_one_argument_count(name):
    assert name in _lib.SIGNATURES
    assert len(_declared_args(name)) == len(_lib.SIGNATURES[name][1])
    assert callable(getattr(_lib.lib(), name))                                          # AttributeError if not exported


def test_the_version_stays():
    assert _lib.lib().spr_version() == 6


def test_the_size_query_is_monotone_and_zero_without_queries():
    from test_workspace_sizes_host import HUGE, INT_MAX, sweep_points
    fn = _lib.lib().spr_deform_reg_workspace_size
    assert fn(0) == 0 and fn(-1) == 0 and fn(-INT_MAX) == 0
    prev = 0
    for v in sweep_points(INT_MAX):
        r = fn(v)
        assert prev <= r < HUGE, (v, prev, r)
        prev = r
    assert fn(1) > 0 and fn(1 << 20) > fn(1)


def test_host_side_refusals():
    L = _lib.lib()
    one = torch.zeros(256)                          # a non-null offset pointer; nothing is read before the refusals
    of = ctypes.c_void_p(one.data_ptr())

    def call(nq=4, kmax=2, stride=2, n_kp=15, extent=0.1, offsets=of, of_stride=60, modulated=1, repulse=1.2):
        return L.spr_deform_reg(None, nq, None, 4, None, stride, kmax, None, n_kp, extent, offsets, of_stride, modulated,
                                repulse, None, None, None, 0, None)
    assert call(n_kp=17) == 2 and b"kernel points" in L.spr_last_error()
    assert call(offsets=None) == 2 and b"offset features" in L.spr_last_error()
    assert call(of_stride=59) == 2 and b"60 columns" in L.spr_last_error()
    assert call(of_stride=44, modulated=0) == 2 and b"45 columns" in L.spr_last_error()     # of_stride < 3 n_kp
    assert call(nq=0) == 2 and b"empty" in L.spr_last_error()
    assert call(kmax=3) == 2 and b"kmax" in L.spr_last_error()
    assert call(extent=0.0) == 2 and b"KP_extent" in L.spr_last_error()
    assert call(modulated=2) == 2 and b"modulated" in L.spr_last_error()
    assert call(repulse=-1.0) == 2 and b"repulse_extent" in L.spr_last_error()
    assert call() == 2 and b"workspace" in L.spr_last_error()                # valid arguments, no workspace


# ---- the optimizer -------------------------------------------------------------------------------------------------------
def _ids(params):
    return sorted(id(p) for p in params)


@pytest.mark.parametrize("optimizer", ["AdamW", "Adam"])
def test_parameter_groups_follow_deform_lr_factor(optimizer):
    one = _encoder_config("last modulated", optimizer=optimizer)
    model = KPFEncoder(one, 256)
    opt, _ = configure_optimizers(model, one)
    assert len(opt.param_groups) == 1 and _ids(opt.param_groups[0]['params']) == _ids(model.parameters())
    assert opt.param_groups[0]['lr'] == one.base_lr

    cfg = _encoder_config("last modulated", optimizer=optimizer, deform_lr_factor=0.1, scheduler_param=[2, 0.5])
    opt, sched = configure_optimizers(model, cfg)
    rest, slow = opt.param_groups
    assert len(opt.param_groups) == 2
    assert _ids(rest['params'] + slow['params']) == _ids(model.parameters())            # a partition: nothing twice
    want = [p for n, p in model.named_parameters() if n.endswith(("offset_conv.weights", "offset_bias"))]
    assert len(want) == 4 and _ids(slow['params']) == _ids(want)
    assert rest['weight_decay'] == slow['weight_decay'] == cfg.weight_decay
    for step in range(5):
        assert rest['lr'] == pytest.approx(cfg.base_lr * 0.5 ** (step // 2), rel=1e-12)
        assert slow['lr'] == pytest.approx(0.1 * rest['lr'], rel=1e-12)
        opt.step()
        sched.step()


# ---- the restatement -----------------------------------------------------------------------------------------------------
def _loops(case, of, R):
    """The contract of include/spr.h with one Python loop per index, float64: (fit, rep, d_of)."""
    q, s, kp, of = (t.double().numpy() for t in (case["q"], case["s"], case["kp"], of))
    idx, e = case["idx"].numpy(), case["extent"]
    nq, K, ns = q.shape[0], kp.shape[0], s.shape[0]
    fit = rep = 0.0
    d_of = np.zeros_like(of)
    for n in range(nq):
        D = np.array([kp[p] + e * of[n, 3 * p:3 * p + 3] for p in range(K)])
        L = D / e
        for p in range(K):
            best, at = None, None
            for k in range(idx.shape[1]):
                if 0 <= idx[n, k] < ns:
                    y = s[idx[n, k]] - q[n]
                    d2 = float(((y - D[p]) ** 2).sum())
                    if best is None or d2 < best:
                        best, at = d2, y
            g = np.zeros(3)
            if best is not None:
                fit += best / e ** 2
                g += 4 * (D[p] - at) / e
            for j in range(K):
                if j == p:
                    continue
                dist = float(np.sqrt(((L[p] - L[j]) ** 2).sum()))
                h = min(dist - R, 0.0)
                rep += h * h
                if dist > 0:
                    g += 2 * h * (L[p] - L[j]) / dist
            d_of[n, 3 * p:3 * p + 3] = g / (nq * K)
    return fit / (nq * K), rep / (nq * K), d_of


@pytest.mark.parametrize("modulated", rc.MOD, ids=rc.mod_id)
@pytest.mark.parametrize("name", ["nq1 k1 32-32", "simple 7 kernel points 32-32"])
def test_the_restatement_agrees_with_plain_loops(name, modulated):
    case, ref = rc.case_of(name, modulated)
    fit, rep, d_of = _loops(case, ref["offset_features"], rc.R_DEFAULT)
    assert abs(fit - float(ref["fit"])) <= 1e-12 * fit and abs(rep - float(ref["rep"])) <= 1e-12 * rep
    assert float(ref["value"]) == pytest.approx(2 * fit + rep, rel=1e-12)
    assert np.abs(d_of - ref["d_of"].numpy()).max() <= 1e-12 * np.abs(d_of).max()
    K = case["kp"].shape[0]
    assert not ref["d_of"][:, 3 * K:].any()                                             # modulation logits: no gradient
    if case["q"].shape[0] > 2:                                                          # row 0 is all shadow
        assert not ref["m"][0].any() and bool(ref["m"][1:].gt(0).all())


def test_the_restatement_at_a_coincident_pair():
    """Two kernel points of query 1 on one spot: the pair counts R^2 twice and contributes no gradient."""
    case, of, ref = rc.coincident_case()
    R, e, K, nq = rc.R_DEFAULT, case["extent"], case["kp"].shape[0], case["q"].shape[0]
    D = case["kp"] + e * of[:, :3 * K].view(-1, K, 3)                                   # float32, as the kernel forms it
    same = (D.unsqueeze(2) == D.unsqueeze(1)).all(3) & ~torch.eye(K, dtype=torch.bool)
    assert same.nonzero().tolist() == [[1, 1, 2], [1, 2, 1]]
    fit, rep, d_of = _loops(case, of, R)
    assert bool(torch.isfinite(ref["d_of"]).all()) and np.isfinite(d_of).all()
    assert float(ref["rep"]) == pytest.approx(rep, rel=1e-12) and float(ref["fit"]) == pytest.approx(fit, rel=1e-12)
    assert np.abs(d_of - ref["d_of"].numpy()).max() <= 1e-12 * np.abs(d_of).max()
    # the pair's share of row 1's repulsive sum is R^2, twice (the loops above skip its gradient: dist == 0)
    L = ((case["kp"].double() + e * of[:, :3 * K].double().view(-1, K, 3)) / e)[1]
    others = sum(min(float((L[i] - L[j]).norm()) - R, 0.0) ** 2 for i in range(K) for j in range(K)
                 if i != j and {i, j} != {1, 2})
    rest = (L.unsqueeze(1) - L.unsqueeze(0)).norm(dim=2)
    assert int((rest[~torch.eye(K, dtype=torch.bool)] < R).sum()) > 2                    # other pairs push as well
    assert ref64_row_rep(case, of, 1) - others == pytest.approx(2 * R * R, rel=1e-12)


def ref64_row_rep(case, of, n):
    """sum_i sum_{j != i} min(dist - R, 0)^2 of row n alone, from the restatement."""
    one = {k: (v[n:n + 1] if k in ("q", "idx") else v) for k, v in case.items()}
    return float(rc.ref64(one, offset_features=of[n:n + 1])["rep"]) * case["kp"].shape[0]


def test_every_case_holds_the_argmin_gap():
    for name in dc.CASES:
        for modulated in rc.MOD:
            case, ref = rc.case_of(name, modulated)
            assert rc.argmin_gap(case, ref["offset_features"]) >= rc.GAP_MIN
