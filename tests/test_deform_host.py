"""Host: deformable / modulated KPConv without a GPU -- the float64 restatement of tests/deform_cases.py against the
reference's own float32 run (tests/golden/kpconv_deform.npz), the module's constructor and state-dict layout, the
opt-in of the block names, the level radii of the pyramid plan and the calibration, and the argument checks of the new
entry points."""
import ctypes

import numpy as np
import pytest
import torch

import deform_cases as dc
import kpconv_modes_cases as kc
from conftest import load_golden
from superpoints_registration_amd import _lib, calibration, deformable, get_config, kpconv_blocks, ops, synthetic
from superpoints_registration_amd.kpconv import KPFDecoder, KPFEncoder, plan_pyramid
from superpoints_registration_amd.kpconv_blocks import ResnetBottleneckBlock, SimpleBlock, block_decider

T = torch.from_numpy
DEFORMABLE_NAMES = ('simple_deformable', 'simple_deformable_strided', 'resnetb_deformable', 'resnetb_deformable_strided')


def _rel(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


# ---- the restatement is the reference's behaviour ------------------------------------------------------------------------
@pytest.mark.parametrize("modulated", [False, True], ids=["plain", "modulated"])
def test_the_restatement_matches_the_reference(modulated):
    g = load_golden("kpconv_deform.npz")
    case = dc.golden_case(modulated, kp=T(g["kp"]), off_kp=T(g["off_kp"]))
    assert not np.array_equal(g["kp"], g["off_kp"]), "the offset convolution has its own kernel points"
    assert abs(case["extent"] - float(g["extent"])) <= 1e-15
    dc.check_conditions(case)
    out, aux, grads = dc.ref64(case, kc.golden_go())
    tag = "mod|" if modulated else "plain|"
    assert _rel(T(g[tag + "out"]), out) <= 1e-5
    assert _rel(T(g[tag + "dx"]), grads["dx"]) <= 2e-5
    assert _rel(T(g[tag + "d_off_b"]), grads["d_off_b"]) <= 2e-5
    for name in ("dw", "d_off_w"):
        flat = grads[name].reshape(-1)
        assert float((flat[::dc.GOLDEN_DW_STEP] - T(g[tag + name + "|samples"]).double()).abs().max() / flat.abs().max()) <= 2e-5
        assert abs(float(flat.norm()) - float(g[tag + name + "|norm"])) <= 2e-5 * float(g[tag + name + "|norm"])
    assert float(((T(g[tag + "min_d2"]).double() - aux["min_d2"]).abs() / aux["min_d2"]).max()) <= 1e-5
    assert _rel(T(g[tag + "deformed_KP"]), aux["deformed_KP"]) <= 1e-5


def test_every_case_meets_its_input_conditions():
    for name in dc.CASES:
        for modulated in (False, True):
            c = dc.check_conditions(dc.make_case(name, modulated))
            assert c["n_valid"] > 0


def test_the_restated_gradient_skips_nothing_at_these_inputs():
    """The one stated deviation (an item with d2 == 0 contributes 0 to the offset gradient; the reference's sqrt gives
    NaN) is not exercised by a case: the distance floor keeps every item away from it, so the float64 autograd values
    are finite and are the reference's."""
    case = dc.make_case("nq37 k5 64-64", True)
    _, _, grads = dc.ref64(case, synthetic.rand((37, 64), 77))
    assert all(bool(torch.isfinite(v).all()) for v in grads.values())


# ---- the module ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("modulated", [False, True], ids=["plain", "modulated"])
def test_constructor_and_state_dict_layout(modulated):
    np.random.seed(3)
    m = deformable.KPConvDeformable(15, 3, 32, 64, 0.08, 0.1, modulated=modulated)
    od = 60 if modulated else 45
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes == {"weights": (15, 32, 64), "offset_bias": (od,), "kernel_points": (15, 3),
                      "offset_conv.weights": (15, 32, od), "offset_conv.kernel_points": (15, 3)}
    assert list(shapes) == ["weights", "offset_bias", "kernel_points", "offset_conv.weights", "offset_conv.kernel_points"]
    assert isinstance(m.offset_conv, kpconv_blocks.KPConv) and not m.offset_conv.deformable
    assert m.offset_conv.KP_extent == m.KP_extent and m.offset_conv.radius == m.radius and m.offset_dim == od
    assert float(m.offset_bias.detach().abs().max()) == 0.0 and float(m.weights.detach().abs().max()) > 0
    assert not torch.equal(m.kernel_points, m.offset_conv.kernel_points), "the offset convolution draws its own kernel points"
    assert not m.kernel_points.requires_grad and not m.offset_conv.kernel_points.requires_grad
    assert {n for n, _ in m.named_parameters() if _.requires_grad} == {"weights", "offset_bias", "offset_conv.weights"}
    assert m.deformable and m.modulated == modulated and m.min_d2 is None and m.deformed_KP is None and m.offset_features is None
    assert (m.K, m.p_dim, m.in_channels, m.out_channels, m.KP_influence, m.aggregation_mode) == (15, 3, 32, 64, 'linear', 'sum')


@pytest.mark.parametrize("mode", kc.NEW_MODES, ids=lambda m: "-".join(m))
def test_other_modes_are_refused_by_name(mode):
    with pytest.raises(NotImplementedError, match=f"{mode[0]}.*{mode[1]}"):
        deformable.KPConvDeformable(15, 3, 32, 64, 0.08, 0.1, KP_influence=mode[0], aggregation_mode=mode[1])
    cfg = get_config('3dmatch', deformable_kpconv=True, KP_influence=mode[0], aggregation_mode=mode[1])
    with pytest.raises(NotImplementedError):
        block_decider('resnetb_deformable', 0.1, 128, 128, 1, cfg)
    with pytest.raises(ValueError):
        deformable.KPConvDeformable(15, 3, 32, 64, 0.08, 0.1, KP_influence='quadratic')


# ---- the opt-in ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DEFORMABLE_NAMES)
def test_block_names_build_only_with_the_key(name):
    assert get_config('3dmatch').deformable_kpconv is False
    with pytest.raises((ValueError, NotImplementedError)):
        block_decider(name, 0.1, 128, 128, 1, get_config('3dmatch'))
    with pytest.raises((ValueError, NotImplementedError)):
        block_decider(name, 0.1, 128, 128, 1, get_config('3dmatch', modulated=True))
    for modulated in (False, True):
        cfg = get_config('3dmatch', deformable_kpconv=True, modulated=modulated)
        b = block_decider(name, 0.1, 128, 128, 1, cfg)
        assert isinstance(b, SimpleBlock if name.startswith('simple') else ResnetBottleneckBlock) and b.block_name == name
        assert isinstance(b.KPConv, deformable.KPConvDeformable) and b.KPConv.modulated == modulated
        assert b.KPConv.offset_dim == (60 if modulated else 45)
        rigid = block_decider(name.replace('_deformable', ''), 0.1, 128, 128, 1, cfg)
        assert type(rigid.KPConv) is kpconv_blocks.KPConv and rigid.KPConv.modulated is False
    # the pinned refusals do not depend on the key
    for kw in (dict(deformable=True), dict(modulated=True)):
        with pytest.raises(NotImplementedError):
            kpconv_blocks.KPConv(15, 3, 32, 64, 0.08, 0.1, **kw)


def test_a_deformable_first_block_never_takes_the_stem_route(monkeypatch):
    from superpoints_registration_amd import stem
    cfg = get_config('3dmatch', deformable_kpconv=True)
    b = block_decider('simple_deformable', 0.0625, 1, 128, 0, cfg)
    rigid = block_decider('simple', 0.0625, 1, 128, 0, cfg)
    monkeypatch.setattr(stem, "stem_route", lambda *a, **k: True)    # whatever the stem's own rule says
    x = torch.ones((8, 1))
    assert rigid.stem_route(x) and not b.stem_route(x)


def test_a_reference_state_dict_loads_into_the_encoder():
    arch, _ = dc.ENCODER_ARCHS["last modulated"]
    cfg = get_config('3dmatch', deformable_kpconv=True, architecture=list(arch), modulated=True)
    enc = KPFEncoder(cfg, cfg.d_embed)
    names = set(enc.state_dict())
    for i in (6, 7):
        for leaf in ("weights", "kernel_points", "offset_conv.weights", "offset_conv.kernel_points", "offset_bias"):
            assert f"encoder_blocks.{i}.KPConv.{leaf}" in names
    assert not any("offset" in n for n in names if n.startswith("encoder_blocks.8."))
    sd = {k: torch.full_like(v, 0.25) for k, v in enc.state_dict().items()}
    enc.load_state_dict(sd, strict=True)
    assert float(enc.encoder_blocks[6].KPConv.offset_conv.weights.detach().min()) == 0.25
    assert enc.encoder_blocks[6].KPConv.offset_conv.weights.shape == (15, 128, 60)
    with pytest.raises(ValueError):
        KPFEncoder(get_config('3dmatch', architecture=list(arch)), 256)


# ---- level radii ---------------------------------------------------------------------------------------------------------
def reference_radii(cfg):
    """[(conv radius or None, pool radius or None, up radius or None)] per level: Preprocessor.forward of the reference
    (kpconv.py:319-408) restated -- layer_blocks holds the level's non-strided blocks, the conv search widens when a
    deformable name is among layer_blocks[:-1], the pool search when the strided block itself is deformable."""
    r_normal = cfg.first_subsampling_dl * cfg.conv_radius
    layer_blocks, out = [], []
    arch = list(cfg.architecture)
    for i, block in enumerate(arch):
        if 'global' in block or 'upsample' in block:
            break
        if not ('pool' in block or 'strided' in block):
            layer_blocks.append(block)
            if i < len(arch) - 1 and 'upsample' not in arch[i + 1]:
                continue
        conv = pool = up = None
        if layer_blocks:
            conv = r_normal * cfg.deform_radius / cfg.conv_radius if any('deformable' in b for b in layer_blocks[:-1]) \
                else r_normal
        if 'pool' in block or 'strided' in block:
            pool = r_normal * cfg.deform_radius / cfg.conv_radius if 'deformable' in block else r_normal
            up = 2 * pool
        out.append((conv, pool, up))
        r_normal *= 2
        layer_blocks = []
    return out


def _plan_radii(cfg):
    _, levels, _ = plan_pyramid(cfg)
    return [(lv.conv_radius if lv.has_conv else None, lv.pool_radius if lv.down else None,
             2 * lv.pool_radius if lv.down else None) for lv in levels]


def _shipped_variants():
    import decoder_cases
    out = []
    for tag in ('3dmatch', 'kitti', 'modelnet'):
        out.append(get_config(tag))
        out.append(decoder_cases.with_decoder(get_config(tag)))
    return out


def test_without_deformable_names_every_radius_is_todays():
    for cfg in _shipped_variants():
        _, levels, _ = plan_pyramid(cfg)
        r = cfg.first_subsampling_dl * cfg.conv_radius
        for lv in levels:
            assert lv.radius == r and lv.conv_radius == r and lv.pool_radius == r      # the very numbers, not close ones
            r *= 2
        assert _plan_radii(cfg) == reference_radii(cfg)


HEAD = ['simple', 'resnetb', 'resnetb_strided']
RADIUS_ARCHS = [
    HEAD + ['resnetb_deformable', 'resnetb_deformable', 'resnetb'],                # widened conv
    HEAD + ['resnetb', 'resnetb', 'resnetb_deformable'],                           # the quirk: the last block alone
    HEAD + ['resnetb_deformable'],                                                 # a level of one block
    HEAD + ['resnetb_deformable', 'resnetb_deformable_strided', 'resnetb'],        # pool widened; the level's one conv block is its last
    HEAD + ['resnetb', 'resnetb_deformable_strided', 'resnetb_deformable', 'resnetb'],
    ['simple_deformable', 'resnetb', 'resnetb_deformable_strided', 'resnetb', 'nearest_upsample', 'unary'],
] + [list(a) for a, _ in dc.ENCODER_ARCHS.values()]


@pytest.mark.parametrize("arch", RADIUS_ARCHS, ids=lambda a: ",".join(a[2:]))
def test_level_radii_follow_the_reference(arch):
    for tag in ('3dmatch', 'kitti'):
        cfg = get_config(tag, deformable_kpconv=True, architecture=list(arch), neighborhood_limits=[40] * 6)
        assert _plan_radii(cfg) == reference_radii(cfg)
    cfg = get_config('3dmatch', deformable_kpconv=True, architecture=list(arch))
    got = _plan_radii(cfg)
    if arch == RADIUS_ARCHS[1]:
        assert got[1][0] == 0.125, "the last block of a level does not widen its conv search"
    if arch == RADIUS_ARCHS[0]:
        assert got[1][0] == 0.25
    if arch == RADIUS_ARCHS[3]:
        assert got[1] == (0.125, 0.25, 0.5), "one conv block: layer_blocks[:-1] is empty"


@pytest.mark.parametrize("arch", RADIUS_ARCHS[:5], ids=lambda a: ",".join(a[2:]))
def test_calibration_counts_at_the_conv_radius(monkeypatch, arch):
    """calibration._chunk_hists builds each level's table at the conv search's radius; the subsampling cell stays
    2 r_normal / conv_radius."""
    cfg = get_config('3dmatch', deformable_kpconv=True, architecture=list(arch))
    _, levels, _ = plan_pyramid(cfg)
    seen = []

    class Table:
        def __init__(self, supports, s_cu, radius):
            self.supports, self.s_cu = supports, s_cu
            seen.append(("conv", radius))

        def count(self, q, q_cu, hist_n, counts=False):
            return None, torch.zeros((1, hist_n), dtype=torch.int64)

    def subsample(points, cu, dl):
        seen.append(("dl", dl))
        return points, torch.tensor([points.shape[0]])
    monkeypatch.setattr(ops, "RadiusTable", Table)
    monkeypatch.setattr(ops, "grid_subsample", subsample)
    monkeypatch.setattr(ops, "lengths_to_cu", lambda lens, device: None)
    calibration._chunk_hists([torch.zeros((5, 3))], levels, cfg, 8)
    want = []
    for (conv, pool, _), lv in zip(reference_radii(cfg), levels):
        if conv is not None:
            want.append(("conv", conv))
        if pool is not None:
            want.append(("dl", 2 * lv.radius / cfg.conv_radius))
    assert seen == want


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------------------
def test_size_queries_and_host_side_refusals_need_no_gpu():
    L = _lib.lib()
    assert L.spr_version() == 6
    with_planes = L.spr_kpconv_deform_workspace_size(100, 100, 64, 64)
    without = L.spr_kpconv_deform_workspace_size(100, 100, 48, 40)
    assert with_planes - without == L.spr_kpconv_wplanes_bytes(64, 64)
    assert L.spr_kpconv_deform_workspace_size(100, 100, 64, 64) == L.spr_kpconv_modes_workspace_size(100, 100, 64, 64)
    assert L.spr_kpconv_deform_weighted_features_workspace_size(1000) == L.spr_kpconv_weighted_features_workspace_bytes(1000)
    one = torch.zeros(256)                          # a non-null offset pointer; nothing is read before the refusals
    of = ctypes.c_void_p(one.data_ptr())

    def fwd(nq=4, kmax=2, stride=2, n_kp=15, extent=0.1, offsets=of, of_stride=60, modulated=1, impl=0, cin=32):
        return L.spr_kpconv_deform_fwd(None, nq, None, 4, None, stride, kmax, None, cin, None, 32, None, n_kp, extent,
                                       offsets, of_stride, modulated, None, None, impl, None, 0, None, 0, None, None, 0, None)
    assert fwd(nq=0) == 2 and b"empty" in L.spr_last_error()
    assert fwd(kmax=3) == 2 and b"kmax" in L.spr_last_error()
    assert fwd(n_kp=17) == 2 and b"kernel points" in L.spr_last_error()
    assert fwd(extent=0.0) == 2 and b"KP_extent" in L.spr_last_error()
    assert fwd(modulated=2) == 2 and b"modulated" in L.spr_last_error()
    assert fwd(offsets=None) == 2 and b"offset features" in L.spr_last_error()
    assert fwd(of_stride=59) == 2 and b"60 columns" in L.spr_last_error()
    assert fwd(of_stride=45, modulated=0, impl=2) == 2 and b"impl" in L.spr_last_error()
    assert fwd() == 2 and b"workspace" in L.spr_last_error()              # valid arguments, no workspace
    rc = L.spr_kpconv_deform_weighted_features(None, 4, None, 4, None, 2, 2, None, 32, None, 15, 0.1, of, 44, None, None,
                                               None, 0, None)
    assert rc == 2 and b"45 columns" in L.spr_last_error()
    rc = L.spr_kpconv_deform_weighted_features(None, 4, None, 4, None, 2, 2, None, 32, None, 15, 0.1, of, 45, None, None,
                                               None, 0, None)
    assert rc == 2 and b"workspace" in L.spr_last_error()
    rc = L.spr_kpconv_deform_bwd_dx(None, 4, None, 4, None, 2, 2, 32, None, 15, 0.1, of, 60, 1, None, of, 0, None, None,
                                    0, None)
    assert rc == 2 and b"range" in L.spr_last_error()
    rc = L.spr_kpconv_deform_bwd_dx(None, 4, None, 4, None, 2, 2, 32, None, 15, 0.1, of, 60, 1, None, None, 0, None, None,
                                    0, None)
    assert rc == 2 and b"workspace" in L.spr_last_error()
    rc = L.spr_kpconv_deform_bwd_offsets(None, 4, None, 4, None, 2, 2, None, 32, None, 16, 0.1, of, 63, 1, None, None, None)
    assert rc == 2 and b"64 columns" in L.spr_last_error()
    rc = L.spr_kpconv_deform_bwd_offsets(None, 4, None, 4, None, 2, 2, None, 32, None, 15, 0.1, of, 60, 1, None, None, None)
    assert rc == 2 and b"null gradient" in L.spr_last_error()


@pytest.mark.parametrize("name,base", [("spr_kpconv_deform_workspace_size", [1000, 1000, 64, 64]),
                                       ("spr_kpconv_deform_weighted_features_workspace_size", [1000])])
def test_size_queries_are_monotone(name, base):
    """The sweep of tests/test_workspace_sizes_host.py; cout stops at 256, where the weight planes end."""
    from test_workspace_sizes_host import HUGE, INT_MAX, sweep_points
    fn = getattr(_lib.lib(), name)
    for i in range(len(base)):
        prev = None
        for v in sweep_points(256 if i == 3 else INT_MAX):
            if i in (2, 3) and v % 32:
                continue
            args = list(base)
            args[i] = v
            r = fn(*args)
            assert r < HUGE and (prev is None or r >= prev), (name, args, prev, r)
            prev = r
    assert fn(*[-5] * len(base)) < (1 << 20)
