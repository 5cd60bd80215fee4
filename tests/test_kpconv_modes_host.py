"""CPU: KPConv's influence functions and aggregation rules -- the float64 restatement (tests/kpconv_modes_cases.py)
against the reference's own results (tests/golden/kpconv_modes.npz) and against oracle.torch_oracle.kpconv, the
constructor behaviour of KPConv / KPFEncoder in every mode, and the C ABI of the new entry points."""
import re

import numpy as np
import pytest
import torch

import kpconv_modes_cases as kc
from conftest import load_golden
from oracle import torch_oracle as O
from superpoints_registration_amd import _lib, get_config, kpconv_modes
from superpoints_registration_amd.kpconv import KPFEncoder
from superpoints_registration_amd.kpconv_blocks import KPConv, SimpleBlock

T = torch.from_numpy


def _scale_err(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return float((got - ref).abs().max() / ref.abs().max())


def _golden_case():
    g = load_golden("kpconv_modes.npz")
    case = dict(kc.golden_case(), kp=T(g["kp"]))
    assert abs(case["extent"] - float(g["extent"])) == 0.0
    return g, case


def test_golden_inputs_meet_the_input_conditions():
    _, case = _golden_case()
    kc.check_conditions(case)
    idx, ns = case["idx"], case["s"].shape[0]
    assert bool((idx == ns).any()) and bool((idx[0] == ns).all()), "shadow entries and an all-shadow row"
    assert case["s"].shape[0] == 96 and idx.shape[1] == 20 and case["w"].shape == (15, 32, 64)


@pytest.mark.parametrize("influence,aggregation", kc.NEW_MODES)
def test_restatement_matches_the_reference(influence, aggregation):
    """Output within 1e-5 of its scale, gradients within 2e-5: the bounds tests/test_gpu_ops.py and
    tests/test_gpu_backward.py apply to KPConv (the golden is the reference's float32 CPU run)."""
    g, case = _golden_case()
    out, dx, dw = kc.ref64(case, influence, aggregation, kc.golden_go())
    tag = f"{influence}|{aggregation}|"
    assert _scale_err(out, g[tag + "out"]) <= 1e-5
    assert _scale_err(dx, g[tag + "dx"]) <= 2e-5
    samples = dw.reshape(-1)[::kc.GOLDEN_DW_STEP]
    assert float((samples - T(g[tag + "dw|samples"]).double()).abs().max() / dw.abs().max()) <= 2e-5
    assert abs(float(dw.norm()) - float(g[tag + "dw|norm"])) <= 2e-5 * float(g[tag + "dw|norm"])


def test_restatement_of_linear_sum_is_the_oracle():
    _, case = _golden_case()
    ours = kc.ref64(case, 'linear', 'sum')
    ref = O.kpconv(case["q"].double(), case["s"].double(), case["idx"].long(), case["x"].double(), case["w"].double(),
                   case["kp"].double(), case["extent"])
    assert _scale_err(ours, ref) <= 1e-14


def test_modes_differ_from_each_other():
    """Six different operators: no two combinations agree on the golden inputs (a mode switch that is ignored shows)."""
    _, case = _golden_case()
    outs = {m: kc.ref64(case, *m) for m in kc.MODES}
    for a in kc.MODES:
        for b in kc.MODES:
            if a < b:
                assert _scale_err(outs[a], outs[b]) > 1e-3, (a, b)


def test_closest_gap_and_row_sum_helpers():
    q = torch.zeros((1, 3))
    s = torch.tensor([[0.1, 0.0, 0.0], [0.0, 0.5, 0.0]])
    kp = torch.tensor([[0.0, 0.0, 0.0], [0.2, 0.0, 0.0], [0.0, 0.4, 0.0]])
    idx = torch.tensor([[0, 2]])                        # support 0, then a shadow entry
    # support 0: d2 = 0.01, 0.01, 0.17 -> a tie (float32 0.1 and 0.2: equal to rounding)
    assert kc.closest_gap(q, s, idx, kp) < 1e-6
    idx = torch.tensor([[1, 2]])                        # support 1: d2 = 0.25, 0.29, 0.01 -> (0.25 - 0.01) / 0.25
    assert abs(kc.closest_gap(q, s, idx, kp) - 0.96) < 1e-6
    assert kc.closest_gap(q, s, torch.tensor([[2, 5]]), kp) == float('inf')
    assert abs(kc.min_row_sum(torch.tensor([[1.0, -0.5], [0.25, -0.125]])) - 0.125) < 1e-12


# ---- constructors ------------------------------------------------------------------------------------------------------
def _conv(**kw):
    np.random.seed(0)
    return KPConv(15, 3, 32, 64, 0.06, 0.15, **kw)


def test_all_six_combinations_build_with_one_state_dict_layout():
    ref = None
    for influence, aggregation in kc.MODES:
        conv = _conv(KP_influence=influence, aggregation_mode=aggregation)
        assert (conv.KP_influence, conv.aggregation_mode) == (influence, aggregation)
        layout = {k: tuple(v.shape) for k, v in conv.state_dict().items()}
        assert layout == {"weights": (15, 32, 64), "kernel_points": (15, 3)}
        ref = ref or layout
        assert layout == ref


def test_deformable_and_modulated_still_raise():
    for kw in (dict(deformable=True), dict(modulated=True), dict(deformable=True, modulated=True)):
        with pytest.raises(NotImplementedError):
            _conv(**kw)
        with pytest.raises(NotImplementedError):
            _conv(KP_influence='gaussian', aggregation_mode='closest', **kw)


def test_unknown_strings_raise_value_error():
    with pytest.raises(ValueError, match="influence"):
        _conv(KP_influence='quadratic')
    with pytest.raises(ValueError, match="closest"):
        _conv(aggregation_mode='mean')
    with pytest.raises(ValueError):
        kpconv_modes.mode_codes('linear', 'max')
    assert kpconv_modes.mode_codes('gaussian', 'closest') == (2, 1)
    assert kpconv_modes.mode_codes('constant', 'sum') == (0, 0)
    assert kpconv_modes.is_default_mode('linear', 'sum') and not kpconv_modes.is_default_mode('linear', 'closest')


def test_config_keys_reach_every_kpconv_of_the_encoder():
    cfg = get_config('3dmatch', KP_influence='gaussian', aggregation_mode='closest')
    enc = KPFEncoder(cfg, cfg.d_embed)
    convs = [m for m in enc.modules() if isinstance(m, KPConv)]
    assert len(convs) == sum('simple' in b or 'resnetb' in b for b in cfg.architecture) > 0
    assert all((c.KP_influence, c.aggregation_mode) == ('gaussian', 'closest') for c in convs)
    default = KPFEncoder(get_config('3dmatch'), cfg.d_embed)
    assert list(enc.state_dict().keys()) == list(default.state_dict().keys())
    assert all(a.shape == b.shape for a, b in zip(enc.state_dict().values(), default.state_dict().values()))


def test_the_stem_route_is_for_the_default_mode_only(monkeypatch):
    """SimpleBlock.stem_route: stem.stem_route's answer in linear / sum, False in every other mode."""
    from superpoints_registration_amd import stem
    monkeypatch.setattr(stem, "stem_route", lambda x, w, use_bn: True)
    x = torch.ones((8, 1))
    for influence, aggregation in kc.MODES:
        cfg = get_config('3dmatch', KP_influence=influence, aggregation_mode=aggregation)
        block = SimpleBlock('simple', 1, 64, 0.0625, 0, cfg)
        assert block.stem_route(x) == ((influence, aggregation) == ('linear', 'sum'))


# ---- C ABI ---------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("spr_kpconv_modes_workspace_size", "spr_kpconv_modes_fwd",
               "spr_kpconv_modes_weighted_features_workspace_size", "spr_kpconv_modes_weighted_features",
               "spr_kpconv_modes_bwd_dx")


def test_new_symbols_are_declared_exported_and_bound():
    import ctypes
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spr.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(raw, name) and name in _lib.SIGNATURES, name
    for name, value in (("SPR_KP_CONSTANT", 0), ("SPR_KP_LINEAR", 1), ("SPR_KP_GAUSSIAN", 2), ("SPR_KP_SUM", 0),
                        ("SPR_KP_CLOSEST", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), hdr), name
    assert _lib.lib().spr_version() == 6


def test_size_queries_and_host_side_refusals_need_no_gpu():
    L = _lib.lib()
    # the forward keeps the weight planes of spr_kpconv_prep_weights for plane shapes only
    with_planes = L.spr_kpconv_modes_workspace_size(100, 100, 64, 64)
    without = L.spr_kpconv_modes_workspace_size(100, 100, 48, 40)
    assert with_planes - without == L.spr_kpconv_wplanes_bytes(64, 64)
    assert L.spr_kpconv_modes_weighted_features_workspace_size(1000) == L.spr_kpconv_weighted_features_workspace_bytes(1000)
    fwd = lambda infl, agg: L.spr_kpconv_modes_fwd(None, 4, None, 4, None, 2, 2, None, 32, None, 32, None, 15, 0.1, infl,
                                                   agg, None, 0, None, 0, None, 0, None, None, 0, None)
    assert fwd(3, 0) == 2 and b"influence" in L.spr_last_error()
    assert fwd(1, 2) == 2 and b"aggregation" in L.spr_last_error()
    assert fwd(2, 1) == 2 and b"workspace" in L.spr_last_error()          # valid mode, no workspace
    rc = L.spr_kpconv_modes_weighted_features(None, 4, None, 4, None, 2, 2, None, 32, None, 15, 0.1, 0, 7, None, None,
                                              None, 0, None)
    assert rc == 2 and b"aggregation" in L.spr_last_error()
    rc = L.spr_kpconv_modes_bwd_dx(None, 4, None, 4, None, 2, 2, 32, None, 15, 0.1, -1, 0, None, None, 0, None, None, 0,
                                   None)
    assert rc == 2 and b"influence" in L.spr_last_error()


@pytest.mark.parametrize("name,base", [("spr_kpconv_modes_workspace_size", [1000, 1000, 64, 64]),
                                       ("spr_kpconv_modes_weighted_features_workspace_size", [1000])])
def test_size_queries_are_monotone(name, base):
    """The sweep of tests/test_workspace_sizes_host.py; cout stops at 256, where the weight planes end (wider outputs
    take the one-thread-per-element kernel and keep no planes)."""
    from test_workspace_sizes_host import HUGE, INT_MAX, sweep_points
    fn = getattr(_lib.lib(), name)
    for i in range(len(base)):
        prev = None
        for v in sweep_points(256 if i == 3 else INT_MAX):
            if i in (2, 3) and v % 32:
                continue                                  # plane shapes: multiples of 32 (others keep no planes)
            args = list(base)
            args[i] = v
            r = fn(*args)
            assert r < HUGE and (prev is None or r >= prev), (name, args, prev, r)
            prev = r
    assert fn(*[-5] * len(base)) < (1 << 20)
