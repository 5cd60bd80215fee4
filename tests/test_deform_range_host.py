"""CPU: the inputs of tests/test_gpu_deform_range.py (tests/deform_range_cases.py).  Every case meets its input
conditions in float64 -- range gap, distance floor (or "exactly 0 or >= DIST_MIN" in the d2 == 0 cases), row sums; the
argmin gap for the regulariser -- and holds what it is meant to hold; the guarded float64 restatement equals
deform_cases.kpconv_deform_ref; the forward dispatch and the tile kernel's LDS formula are restated as the source has
them."""
import os

import numpy as np
import pytest
import torch

import deform_cases as dc
import deform_range_cases as drc
import deform_reg_cases as rc
import kpconv_modes_cases as kc

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "superpoints_registration_amd", "csrc")


def _source(name):
    with open(os.path.join(SRC, name)) as f:
        return f.read()


def test_routes_are_what_they_name():
    for name, (impl, cin, cout, n_kp) in drc.ROUTES.items():
        assert drc.deform_route(impl, cin, cout, n_kp) == drc.ROUTE_KERNEL[name], name
    src = _source("kpconv_deform.hip")
    assert "if (impl == 0 && n_kp == kKP && plane_shape(cin, cout))" in src and "constexpr int kKP = 15;" in src
    assert "cin > 0 && cin % 32 == 0 && cout > 0 && cout % 32 == 0 && cout <= 256" in src
    assert "return cin % 64 == 0\n               ? launch_deform_tile<64>" in src


def test_the_lds_formula_and_the_grid_cap_are_the_sources():
    src = _source("kpconv_deform.hip")
    assert "constexpr int kTQ = 32, kWaves = 8;" in src and "constexpr int kSlot = 16;" in _source("kpconv_walk.h")
    assert ("return 2 * sizeof(_Float16) * (size_t)kTQ * (kKP * cc + 16) + sizeof(float4) * kWaves * kKPmax +\n"
            "         sizeof(float) * kWaves * 64 * kSlot + sizeof(int) * kWaves * 64 + sizeof(int) * kTQ;") in src
    assert "const int per_cu = (int)((160 * 1024) / lds);" in src
    assert "const int cap = device_cu_count() * (per_cu > 0 ? per_cu : 1);" in src
    f16, f4, f, i = 2, 16, 4, 4
    for cc in (32, 64):
        want = 2 * f16 * 32 * (15 * cc + 16) + f4 * 8 * 16 + f * 8 * 64 * 16 + i * 8 * 64 + i * 32
        assert drc.deform_lds_bytes(cc) == want <= drc.LDS_BUDGET
        assert drc.residency(cc) == (160 * 1024) // want == 1
        nq = drc.grid_nq(drc.HOST_CU, cc)
        tiles, cap = -(-nq // 32), drc.HOST_CU * drc.residency(cc)
        assert tiles == cap + 2 and nq % 32 == 1            # a full second-trip tile, then a tile of one row
    assert "for (int b = threadIdx.x; b < nblocks; b += 256)" in _source("deform_reg.hip")
    assert -(-drc.REG_BIG_NQ // 16) > 256 and -(-drc.REG_BIG_NQ // 16) <= 512


# ---- the guarded restatement ---------------------------------------------------------------------------------------------
def _both(name, modulated, go=None):
    case = dc.make_case(name, modulated)
    of = dc.ref64(case)[1]["offset_features"].float()
    outs = []
    for fn in (dc.kpconv_deform_ref, drc.guarded_ref):
        f = lambda k: case[k].double()
        x, w, o = f('x'), f('w'), of.double()
        if go is not None:
            for t in (x, w, o):
                t.requires_grad_(True)
        out, aux = fn(f('q'), f('s'), case['idx'], x, w, f('kp'), case['extent'], modulated, offset_features=o)
        if go is not None:
            out.backward(go.double())
        outs.append((out.detach(), aux, (x.grad, w.grad, o.grad)))
    return outs


@pytest.mark.parametrize("modulated", drc.MOD, ids=drc.mod_id)
@pytest.mark.parametrize("name", list(dc.CASES))
def test_the_guarded_restatement_is_the_reference_bit_for_bit(name, modulated):
    (out, aux, _), (gout, gaux, _) = _both(name, modulated)
    assert torch.equal(out, gout) and float(out.abs().max()) > 0
    for k in ("min_d2", "in_range", "count", "d2"):
        assert torch.equal(aux[k], gaux[k]), k


@pytest.mark.parametrize("modulated", drc.MOD, ids=drc.mod_id)
@pytest.mark.parametrize("name", dc.BACKWARD_CASES)
def test_the_guarded_restatement_has_the_references_gradient(name, modulated):
    from superpoints_registration_amd import synthetic
    case = dc.make_case(name, modulated)
    go = synthetic.rand((case["q"].shape[0], case["w"].shape[2]), 77)
    (_, aux, grads), (_, _, ggrads) = _both(name, modulated, go)
    assert float(aux["d2"].detach()[aux["valid"]].min()) > 0          # none of them holds a zero
    for a, b in zip(grads, ggrads):
        assert float(a.abs().max()) > 0 and float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())


# ---- every case meets its conditions ---------------------------------------------------------------------------------------
def _checked(name):
    spec = drc.CASES[name]
    case = drc.get(name)
    out, aux, _ = drc.ref64(case, guarded=spec.zeros)
    c = drc.check_conditions(case, aux, spec.zeros)
    return case, out, aux, c


def _contract(case):
    """include/spr.h: legal strides (contiguous tensors), n_kp <= 16, float32 / int32; finite inputs."""
    K, nq = case["kp"].shape[0], case["q"].shape[0]
    assert 1 <= K <= drc.KP_MAX and case["idx"].dtype == torch.int32 and case["idx"].shape[0] == nq
    assert case["of"].shape == (nq, dc.offset_dim(K, case["modulated"])) and case["of"].dtype == torch.float32
    for k in ("q", "s", "x", "w", "kp", "of"):
        assert case[k].is_contiguous() and bool(torch.isfinite(case[k]).all()), k
    assert case["x"].shape[0] == case["s"].shape[0] and case["w"].shape[:2] == (K, case["x"].shape[1])


@pytest.mark.parametrize("name", list(drc.CASES))
def test_every_case_meets_the_conditions_in_float64(name):
    case, out, aux, c = _checked(name)
    _contract(case)
    assert drc._SEEDS[name] < drc.OFFSET_SEED0 + drc.MAX_SEEDS
    assert c["n_valid"] > 0 and bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
    if not drc.CASES[name].zeros:
        assert c["zeros"] == 0


@pytest.mark.parametrize("route", drc.TILE_ROUTES)
def test_the_grid_case_meets_the_conditions_in_float64(route):
    name, spec = drc.grid_case(route, drc.HOST_CU)
    case = drc.get_grid(route, drc.HOST_CU)
    _contract(case)
    out, aux, _ = drc.ref64(case)
    c = drc.check_conditions(case, aux)
    nq = case["q"].shape[0]
    assert nq == 32 * drc.HOST_CU + 33 and case["idx"].shape[1] == 5 and case["w"].shape[2] == 32 and case["modulated"]
    assert drc.deform_route(*drc.ROUTES[route][:2], 32, 15) == drc.ROUTE_KERNEL[route]
    # the second trip's rows and the last tile's row are live and differ from the first trip's
    live = aux["in_range"].any(1)
    assert bool(live[32 * drc.HOST_CU:32 * drc.HOST_CU + 32].any()) and float(out[-1].abs().max()) > 0
    assert not torch.equal(aux["count"][:32], aux["count"][32 * drc.HOST_CU:32 * drc.HOST_CU + 32])
    print(f"{name}: seed {drc._SEEDS[name]}, share {c['share']:.2f}, gap {c['gap']:.2e}")


@pytest.mark.parametrize("name", list(drc.REG_CASES))
def test_every_regulariser_case_meets_the_argmin_gap(name):
    case = drc.get(name, drc.REG_CASES)
    _contract(case)
    assert rc.check_gap(case, case["of"]) >= rc.GAP_MIN
    ref = rc.ref64(case, offset_features=case["of"])
    assert all(bool(torch.isfinite(ref[k]).all()) for k in ("value", "fit", "rep", "d_of"))


# ---- every case holds what it is meant to hold ---------------------------------------------------------------------------
def _cut_rows(aux):
    return aux["valid"].any(1) & ~aux["in_range"].any(1)


@pytest.mark.parametrize("route", drc.FWD_ROUTES)
def test_offset_cases_cut_and_keep(route):
    for offset, ext in kc.OFFSETS:
        for srt in (True, False):
            case, _, aux, c = _checked(drc.offset_name(route, offset, ext, srt, True))
            assert 0.1 <= c["share"] <= 0.9, c["share"]
            assert float(case["q"].abs().max()) >= offset
            idx, ns = case["idx"].long(), case["s"].shape[0]
            if not srt:
                assert bool((idx[:, 0] == ns).any()) and bool(((idx[:, :-1] == ns) & (idx[:, 1:] < ns)).any())


@pytest.mark.parametrize("route", ("tile32", "tile64", "simple48"))
def test_width_cases_reach_every_staging_chunk(route):
    for mod in drc.MOD:
        for kmax in drc.DEFORM_WIDTHS:
            case, _, aux, _ = _checked(drc.width_name(route, kmax, "unsorted", mod))
            assert case["idx"].shape[1] == kmax
            inr = aux["in_range"]
            if kmax > 64:
                assert int(inr[:, 64:].any(1).sum()) >= (5 if kmax == 65 else 30), "no in-range item behind column 64"
            if kmax > 128:
                assert bool(inr[:, 128].any()) and bool(aux["valid"][:, 128].any())
            assert bool(aux["valid"][:, kmax - 1].any())
        # the first 64 columns hold only valid, out-of-range neighbours; what is in range comes later
        case, _, aux, _ = _checked(drc.width_name(route, 129, "late chunk", mod))
        inr, valid = aux["in_range"], aux["valid"]
        late = ~inr[:, :64].any(1) & valid[:, :64].all(1) & inr[:, 64:].any(1)
        print(f"late chunk {route}: {int(late.sum())} rows, {int((late & inr[:, 64:128].any(1)).sum())} with items in the "
              f"second chunk, {int((late & inr[:, 128]).sum())} in the third")
        assert int(late.sum()) >= 40 and int((late & inr[:, 64:128].any(1)).sum()) >= 20 and int((late & inr[:, 128]).sum()) >= 20
        # one chunk with all 64 lanes in range
        case, _, aux, _ = _checked(drc.width_name(route, 129, "full chunk", mod))
        full = aux["in_range"][:, :64].all(1) | aux["in_range"][:, 64:128].all(1)
        assert int(full.sum()) >= 10


def test_in_range_edge_cases_hold_their_rows():
    for route in drc.FWD_ROUTES:
        for mod in drc.MOD:
            case, out, aux, _ = _checked(drc.edge_name("cut", route, mod))
            cut = _cut_rows(aux)
            assert bool(cut[drc.CUT_ROWS].all()) and bool(aux["valid"][drc.CUT_ROWS].any(1).all())
            assert float(out[drc.CUT_ROWS].abs().max()) == 0.0 and int((~cut & aux["valid"].any(1)).sum()) >= 20
            case, _, aux, _ = _checked(drc.edge_name("odd", route, mod))
            n_in = aux["in_range"].sum(1).tolist()
            assert all(n_in.count(c) >= 5 for c in drc.ODD_COUNTS), [n_in.count(c) for c in drc.ODD_COUNTS]
            case, out, aux, _ = _checked(drc.edge_name("edges", route, mod))
            idx, ns = case["idx"].long(), case["s"].shape[0]
            neg = [r for r in drc.NEG_ROWS if bool(aux["in_range"][r].any())]
            assert len(neg) >= 8 and sum(int(aux["in_range"][r].sum()) >= 2 for r in neg) >= 5
            for r in neg:
                sums = case["x"].double().sum(1)[idx[r][aux["in_range"][r]]]
                assert bool((sums < 0).all()) and int(aux["count"][r]) == 1 and float(out[r].abs().max()) > 0
            dup = [r for r in drc.DUP_ROWS if bool(aux["in_range"][r, :3].all())]
            assert all(int(idx[r, 0]) == int(idx[r, 1]) == int(idx[r, 2]) < ns for r in drc.DUP_ROWS) and len(dup) >= 5
            for v in (-1, ns, ns + 5):
                assert int((idx == v).sum()) >= 10, v
            assert int(idx.min()) == -1 and int(idx.max()) == ns + 5


def test_offset_magnitudes_and_logits():
    for route in drc.FWD_ROUTES:
        for mod in drc.MOD:
            shares = []
            for sc in drc.OF_SCALES:
                case, _, aux, c = _checked(drc.edge_name(f"of*{sc:g}", route, mod))
                live = aux["valid"].any(1)
                shares.append(int(_cut_rows(aux).sum()) / int(live.sum()))
            K = case["kp"].shape[0]
            print(f"of scales {route} {drc.mod_id(mod)}: fully cut rows {shares}")
            assert 0.05 <= shares[3] < 1.0 and shares[2] <= shares[3] and shares[0] == shares[1] == 0.0
            tiny = drc.get(drc.edge_name(f"of*{drc.OF_SCALES[0]:g}", route, mod))["of"]
            assert 0 < float(tiny[:, :3 * K].abs().max()) < 1e-5
        case, _, aux, _ = _checked(drc.edge_name("logits", route, True))
        K = case["kp"].shape[0]
        lg = case["of"][:, 3 * K:].numpy()
        assert set(np.unique(lg).tolist()) == set(drc.LOGITS)
        with np.errstate(over="ignore"):
            m32 = np.float32(2) / (np.float32(1) + np.exp(-lg, dtype=np.float32))
        assert bool(np.isfinite(m32).all())
        assert bool((m32[lg == 90] == 2).all()) and bool((m32[lg == -90] == 0).all()) and bool((m32[lg == 20] == 2).all())
        assert bool((m32[lg == 0] == 1).all()) and bool((m32[lg == -20] > 0).all())
        assert bool((m32[np.abs(lg) == 90] * (1 - np.float32(0.5) * m32[np.abs(lg) == 90]) == 0).all())


@pytest.mark.parametrize("route", ("tile32", "tile64", "simple48"))
def test_the_zero_case_sits_on_kernel_point_zero(route):
    for mod in drc.MOD:
        case, _, aux, c = _checked(drc.edge_name("zero", route, mod))
        nq = case["q"].shape[0]
        assert torch.equal(case["q"], case["s"]) and bool((case["idx"][:, 0].long() == torch.arange(nq)).all())
        assert float(case["kp"][0].abs().max()) == 0.0 and float(case["of"][:, :3].abs().max()) == 0.0
        assert bool((aux["d2"][:, 0, 0] == 0).all()) and c["zeros"] == nq and c["floor_nz"] >= dc.DIST_MIN
        assert float(case["of"][:, 3:].abs().min()) > 0
        # float32 sees the same zeros
        d2, _ = kc.d2_float32(dict(case, kp=case["kp"] + case["extent"] * case["of"][0, :45].view(15, 3)))
        assert d2[0, 0, 0] == 0.0


def test_kernel_point_counts():
    for mod in drc.MOD:
        for route, n in (("kp1", 1), ("kp7", 7), ("kp16", 16)):
            case, _, aux, c = _checked(drc.edge_name("points", route, mod))
            assert case["kp"].shape[0] == n and case["w"].shape[0] == n and 0.05 < c["share"] < 0.95
        assert drc.KP_MAX == kc.AUX_KP_MAX == 16


@pytest.mark.parametrize("route", drc.TILE_ROUTES)
def test_magnitude_cases(route):
    for mod in drc.MOD:
        case, _, aux, _ = _checked(drc.edge_name("mag", route, mod))
        assert case["idx"].shape[1] == kc.MAG_KMAX == 16 and float(case["x"].abs().max()) < 1.0
        for edge in kc.POW2_EDGES:
            x = kc.pow2_edge_x(case["x"], edge)
            bound = np.float32(2 * kc.MAG_KMAX) * np.float32(x.abs().max())
            exp = np.frexp(bound)[1]
            assert {"below": exp == 7 and bound < 128, "at": bound == 128, "above": exp == 8 and bound > 128}[edge]
            edged = dict(case, x=x)
            drc.check_conditions(edged, drc.ref64(edged)[1])
        mixed = dict(case, x=kc.mixed_x(case["x"]))
        drc.check_conditions(mixed, drc.ref64(mixed)[1])
        for sx in kc.X_SCALES:
            scaled = dict(case, x=case["x"] * sx)
            assert torch.equal(scaled["x"].double(), case["x"].double() * sx)
            drc.check_conditions(scaled, drc.ref64(scaled)[1], x_scale=sx)
    for edge in kc.POW2_EDGES:
        case, _, aux, c = _checked(f"saturating {route} {edge}")
        v = float(case["x"][0, 0])
        bound = 2.0 * kc.MAG_KMAX * float(case["x"].abs().max())
        assert bool((aux["wf"][:, 0, :] == bound).all()) and bound == 2 * 16 * v, "the saturating sum is not the bound"
        assert float(aux["wf"].abs().max()) == bound and c["zeros"] == 65 * kc.MAG_KMAX
        assert bool((case["idx"].long() == torch.arange(65).unsqueeze(1)).all())


def test_regulariser_cases_hold_their_rows():
    for mod in drc.MOD:
        case = drc.get(f"reg rows {drc.mod_id(mod)}", drc.REG_CASES)
        real = ((case["idx"].long() >= 0) & (case["idx"].long() < case["s"].shape[0])).sum(1)
        assert bool((real[8:16] == 0).all()) and bool((real[16:24] == 1).all()) and int((real >= 2).sum()) >= 20
        for route, n in (("kp1", 1), ("kp16", 16)):
            case = drc.get(f"reg points {route} {drc.mod_id(mod)}", drc.REG_CASES)
            assert case["kp"].shape[0] == n
            ref = rc.ref64(case, offset_features=case["of"])
            assert (float(ref["rep"]) == 0.0) == (n == 1)
        # repulse_extent 50: every pair of every query active; 0: none
        case = drc.get(f"reg of*8 {drc.mod_id(mod)}", drc.REG_CASES)
        K = case["kp"].shape[0]
        L = (case["kp"].double() + case["extent"] * case["of"].double()[:, :3 * K].reshape(-1, K, 3)) / case["extent"]
        dist = (L.unsqueeze(2) - L.unsqueeze(1)).norm(dim=3)
        assert float(dist.max()) < 50.0 and float(dist[:, ~torch.eye(K, dtype=torch.bool)].min()) > 0
        assert float(rc.ref64(case, 0.0, offset_features=case["of"])["rep"]) == 0.0
    for kmax in drc.REG_WIDTHS:
        assert drc.get(f"reg width {kmax} plain", drc.REG_CASES)["idx"].shape[1] == kmax
    for nq in drc.REG_COUNTS:
        assert drc.get(f"reg count {nq} plain", drc.REG_CASES)["q"].shape[0] == nq
    assert drc.get("reg many workgroups", drc.REG_CASES)["q"].shape[0] == 16 * 256 + 17
