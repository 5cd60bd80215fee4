"""CPU: the case builders of tests/test_gpu_kpconv_modes_range.py (tests/kpconv_modes_cases.py) hold what they claim --
the route table against the dispatch text of csrc/kpconv_modes.hip, the exact float32 equalities of the arg-min tie
case, the 10 % cap on rows that leave the strict comparison in `closest`, odd valid counts, power-of-two maxima,
influence underflow -- and the float64 mode reference on these builders' inputs agrees with itself where the modes
coincide, next to its check against tests/golden/kpconv_modes.npz."""
import os
import re

import numpy as np
import pytest
import torch

import forward_cases as fc
import kpconv_modes_cases as kc
from conftest import load_golden

T = torch.from_numpy
HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "superpoints_registration_amd", "csrc",
                   "kpconv_modes.hip")


def _source():
    return re.sub(r"\s+", " ", open(HIP).read())


def test_modes_route_restates_the_dispatch_text():
    """The conditions modes_route restates, as they stand in spr_kpconv_modes_fwd; a change of the dispatch fails here
    until the table follows."""
    src = _source()
    assert "constexpr int kKP = %d;" % kc.TILE_KP in src and "constexpr int kKPmax = %d;" % kc.AUX_KP_MAX in src
    assert "if (impl == 0 && n_kp == kKP && modes_plane_shape(cin, cout)) {" in src
    assert ("inline bool modes_plane_shape(int cin, int cout) { return cin > 0 && cin % 32 == 0 && cout > 0 && "
            "cout % 32 == 0 && cout <= 256; }") in src
    assert "cin % 64 == 0 ? 64 : 32" in src
    assert "n_kp >= 1 && n_kp <= %d, \"kpconv_modes: bad dims\"" % kc.FWD_KP_MAX in src
    assert src.count("n_kp >= 1 && n_kp <= kKPmax") == 2          # weighted features and d x
    for name, (impl, cin, cout, n_kp) in kc.ROUTES.items():
        assert kc.modes_route(impl, cin, cout, n_kp) == kc.ROUTE_KERNEL[name], name
    assert kc.modes_route(0, 32, 288, 15) == "simple" and kc.modes_route(0, 96, 32, 15) == "tile32"
    assert kc.modes_route(0, 64, 256, 15) == "tile64" and kc.modes_route(0, 64, 64, 16) == "simple"
    assert set(kc.ROUTE_KERNEL.values()) == {"tile32", "tile64", "simple"}


def test_the_restatement_matches_the_reference_fixture():
    """kpconv_ref on the golden inputs against the reference's own float32 results, every new mode (forward; the
    gradients are held by tests/test_kpconv_modes_host.py): the reference of every range test."""
    g = load_golden("kpconv_modes.npz")
    case = dict(kc.golden_case(), kp=T(g["kp"]))
    for influence, aggregation in kc.NEW_MODES:
        out = kc.ref64(case, influence, aggregation)
        ref = T(g[f"{influence}|{aggregation}|out"]).double()
        assert float((out - ref).abs().max() / ref.abs().max()) <= 1e-5, (influence, aggregation)


def _closest_cases():
    """Every case the GPU module runs in a closest mode, once per geometry (the geometry does not depend on the
    channel counts; the kernel points depend on n_kp)."""
    for route in ("tile32", "kp7", "kp16"):
        for offset, ext in kc.OFFSETS:
            for srt in (True, False):
                yield f"offset {route} {offset:g} {ext:g} {srt}", kc.offset_case(route, offset, ext, srt)
        for kmax in kc.ROW_WIDTHS:
            for srt in (True, False):
                yield f"width {route} {kmax} {srt}", kc.width_case(route, kmax, srt)
        for nq in kc.QUERY_COUNTS:
            for srt in (True, False):
                yield f"count {route} {nq} {srt}", kc.count_case(route, nq, srt)
        yield f"odd {route}", kc.odd_valid_case(route)
        yield f"edges {route}", kc.count_edge_case(route)
        yield f"tie {route}", kc.tie_case(route)
        for offset, ext in ((0.0, 0.0625), (1e2, 0.0625), (1e3, 0.25)):
            yield f"exact {route} {offset:g}", kc.exact_case(route, offset, ext)[0]
    yield "magnitude", kc.magnitude_case("tile32")
    yield "kp17", kc.cloud_case("impl1", 33, 120, 12, 1e2, 0.125, 49, n_kp=17)


def test_near_ties_stay_under_the_cap():
    """At most 10 % of a case's live rows hold an item whose two lowest d2 are within GAP_MIN (float64 values alone)."""
    worst = (0.0, "")
    for name, case in _closest_cases():
        out, live = kc.near_tie_share(case)
        assert live > 0 and out <= kc.NEAR_TIE_CAP * live, f"{name}: {out} of {live} live rows near a tie"
        worst = max(worst, (out / live, f"{name}: {out} of {live}"))
    print("worst share of near-tie rows:", worst)


def test_near_tie_rows_helper():
    q = torch.zeros((3, 3))
    kp = torch.tensor([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]])
    s = torch.tensor([[0.25, 0.0, 0.0], [0.25 + 1e-6, 0.0, 0.0], [0.1, 0.0, 0.0]])
    case = dict(q=q, s=s, kp=kp, idx=torch.tensor([[0, 3], [1, 3], [2, 3]]))
    # row 0: an exact tie (not a near-tie), row 1: a gap of ~8e-6 relative, row 2: clear
    assert kc.near_tie_rows(case).tolist() == [False, True, False]
    assert kc.near_tie_share(case) == (1, 3)


@pytest.mark.parametrize("route", list(kc.ROUTES))
def test_tie_case_is_an_exact_float32_tie(route):
    """The float32 d2 of every real item: the minimum is taken by kernel point 0 and by at least two others with the
    SAME float32 value, which is also the float64 value (nothing rounded anywhere)."""
    case = kc.tie_case(route)
    d2, valid = kc.d2_float32(case)
    d2_64, _ = kc._d2_64(case)
    n_kp = case["kp"].shape[0]
    expect = np.float32(18.0 / 64.0 * kc.TIE_EXT ** 2)
    assert valid.any(1).all() and int(valid.sum()) > 3 * valid.shape[0]
    items = d2[valid]                                             # [items, p]
    assert np.array_equal(items.astype(np.float64), d2_64.numpy()[valid])
    assert np.all(items.min(1) == expect) and np.all(items[:, 0] == expect)
    ties = (items == expect).sum(1)
    assert np.all(ties >= (5 if n_kp >= 15 else 3)), ties.min()
    assert np.all(np.argmin(items, 1) == 0) and bool((torch.argmin(d2_64, 2)[T(valid)] == 0).all())
    # a kernel that took the LAST minimum would pick another point for every item
    assert np.all((items.shape[1] - 1 - np.argmin(items[:, ::-1], 1)) > 0)
    w = case["w"].double()
    assert float((w[1:].mean((1, 2)) - w[:-1].mean((1, 2))).min()) > 0.2      # clearly different per kernel point
    assert float(case["x"].min()) >= 0.5
    assert kc.near_tie_share(case)[0] == 0


def test_tie_positions_on_the_plain_lattice():
    """(3/8, 3/8, 0) ext: the centre, the +x and +y axis points and the (+, +, +-) corners, indices 0, 1, 3, 7, 8."""
    kp = fc.lattice_kernel_points(1.0).astype(np.float64)
    d2 = ((np.array([0.375, 0.375, 0.0]) - kp) ** 2).sum(1)
    assert np.flatnonzero(d2 == d2.min()).tolist() == [0, 1, 3, 7, 8] and d2.min() == 18.0 / 64.0


@pytest.mark.parametrize("route", ["tile32", "tile64", "simple48"])
def test_odd_valid_counts(route):
    case = kc.odd_valid_case(route)
    counts = kc.valid_counts(case).tolist()
    assert set(counts) == {0, 1, 3, 7, 9} and counts[3] == 0 and counts.count(0) == 1
    idx, ns = case["idx"].long(), case["s"].shape[0]
    for r, c in enumerate(counts):
        assert bool((idx[r, :c] < ns).all()) and bool((idx[r, c:] == ns).all())      # leading, then shadow


def test_shape_edges_of_the_builders():
    """Row widths around the 64-column staging chunk with real neighbours behind column 64 / 128; the last tile of
    nq 33 / 65 holds one live row; unsorted rows carry shadow entries in front."""
    for kmax in (65, 129):
        idx = kc.width_case("tile32", kmax, False)["idx"].long()
        assert idx.shape == (150, kmax) and int((idx[:, 64 * ((kmax - 1) // 64):] < 200).sum()) > 50
    assert int((kc.width_case("tile32", 129)["idx"][:, 64:128] < 200).sum()) > 1000        # sorted: the second pass
    assert kc.count_case("tile32", 33, True)["q"].shape[0] == 33 == 32 + 1
    uns = kc.count_case("tile32", 33, False)["idx"].long()
    assert bool((uns[:, 0] == 120).any()) and bool((uns[:, 1:] < 120).any())
    off = kc.offset_case("tile64", 1e3, 0.03, True)
    assert float(off["q"].abs().max()) > 900 and off["x"].shape == (350, 64) and off["w"].shape == (15, 64, 64)
    assert kc.cloud_case("kp16", 5, 20, 4, 0.0, 0.1, 1)["kp"].shape == (16, 3)
    assert kc.cloud_case("kp7", 5, 20, 4, 0.0, 0.1, 1)["w"].shape == (7, 32, 32)
    assert np.array_equal(fc.kp_weights(3, 5, 9), fc.kp_weights(3, 5, 9, 15))
    assert np.array_equal(fc.random_kernel_points(0.1, 9), fc.random_kernel_points(0.1, 9, 15))
    assert fc.kp_weights(3, 5, 9, 16).shape == (16, 3, 5) and fc.random_kernel_points(0.1, 9, 1).shape == (1, 3)


@pytest.mark.parametrize("route", ["tile32", "simple48", "cin1"])
def test_exact_and_count_edge_inputs(route):
    case, names = kc.exact_case(route, 1e2, 0.0625)
    w = kc.influences_64(case, 'linear')
    for p in range(1, 15):
        assert float(w[names["on_kp"][p - 1], 0, p]) == 1.0
    assert float(w[names["coincident"], 0, 0]) == 1.0 and float(w[names["at_extent"], 0, 0]) == 0.0
    assert float(w[names["inside"], 0, 0]) > 0.0 and float(w[names["outside"], 0, 0]) == 0.0
    edge = kc.count_edge_case(route)
    x = edge["x"].double()
    assert bool((x[:40].sum(1) == 0).all()) and bool((x[40:80].sum(1) == -1).all()) and float(x.abs().max()) < 2 ** 10
    assert bool((x == x.round()).all())
    cnt = kc.ref_counts(edge)
    idx = edge["idx"].long()
    assert bool((idx[3] == 160).all()) and bool((cnt[5:25] == 1).all()) and int(cnt.max()) > 1
    assert bool(((idx[5:25] < 80) | (idx[5:25] == 160)).all())


def test_underflow_inputs():
    """Every Gaussian influence is below half the smallest float32 denormal (it rounds to 0 or to the denormal, never
    further), every linear influence is exactly 0, rows keep real neighbours, and the counts are not all 1."""
    for route in ("tile32", "simple48"):
        case = kc.underflow_case(route)
        assert float(kc.influences_64(case, 'gaussian').max()) < 2.0 ** -150
        assert float(kc.influences_64(case, 'linear').max()) == 0.0
        assert int((kc.valid_counts(case) > 3).sum()) > 20 and int(kc.ref_counts(case).max()) > 3
        for mode in kc.MODES:
            if mode[0] != 'constant':
                assert float(kc.ref64(case, *mode).abs().max()) <= 1e-300
        # every neighbour is 16 extents or more from its query, so all kernel points are nearly equidistant from it:
        # this geometry is over the near-tie cap by construction, and the GPU module compares NO closest mode
        # strictly on it (constant / closest must be finite; the other closest modes must be 0, whatever the pick)
        out, live = kc.near_tie_share(case)
        assert out > kc.NEAR_TIE_CAP * live


@pytest.mark.parametrize("route", kc.MAG_ROUTES)
def test_magnitude_inputs(route):
    """kmax * max|x| in float32 is exactly 2^6, or one float32 step below / above it; the scales are powers of two (the
    float64 reference of a scaled input is the scaled reference, exactly); the mixed tensor's halves differ by 2^12."""
    case = kc.magnitude_case(route)
    x = case["x"]
    assert case["idx"].shape == (65, kc.MAG_KMAX) and float(x.abs().max()) < 1.0
    prod = {e: np.float32(kc.MAG_KMAX) * np.float32(float(kc.pow2_edge_x(x, e).abs().max())) for e in kc.POW2_EDGES}
    assert prod["at"] == np.float32(64.0)
    assert prod["below"] == np.nextafter(np.float32(64), np.float32(0)) and prod["above"] == np.nextafter(np.float32(64), np.float32(128))
    exps = {e: int(np.frexp(prod[e])[1]) - 1 for e in kc.POW2_EDGES}           # floor(log2)
    assert exps == {"below": 5, "at": 6, "above": 6}
    for e in kc.POW2_EDGES:
        assert int((kc.pow2_edge_x(x, e) != x).sum()) == 1
    for sc in kc.X_SCALES + kc.W_SCALES:
        assert np.frexp(sc)[0] == 0.5
    ref = kc.ref64(case, 'gaussian', 'sum')
    scaled = kc.ref64(dict(case, x=x * kc.X_SCALES[0], w=case["w"] * kc.W_SCALES[2]), 'gaussian', 'sum')
    assert torch.equal(scaled, ref * (kc.X_SCALES[0] * kc.W_SCALES[2]))
    mx = kc.mixed_x(x)
    h = x.shape[0] // 2
    assert torch.equal(mx[:h], x[:h]) and torch.equal(mx[h:], x[h:] * 4096.0)
    assert kc.min_row_sum(x) >= kc.SUM_MIN
    # the variants the GPU module runs: the count flag is a float32 row sum's sign there as well (a power-of-two
    # scale of x keeps every sign)
    for variant in [mx] + [kc.pow2_edge_x(x, e) for e in kc.POW2_EDGES]:
        assert kc.min_row_sum(variant) >= kc.SUM_MIN, "a variant's row sum is near the count threshold"
    for e in kc.POW2_EDGES:
        sat = kc.saturating_case(route, e)
        bound = np.float32(kc.MAG_KMAX) * np.float32(float(sat["x"].abs().max()))
        assert bound == prod[e]
        counts = kc.valid_counts(sat)
        assert int((counts == kc.MAG_KMAX).sum()) == 64 and int(counts[3]) == 0
        idx = sat["idx"].long()
        wf = sat["x"].double()[idx.clamp(max=119)][:, :, 0] * (idx < 120)             # constant / sum, channel 0
        assert float(wf.sum(1).max()) == float(bound), "the weighted-feature sums reach kmax * max|x| exactly"


def test_row_sums_are_clear_of_the_count_threshold():
    """The count flag is a float32 row sum's sign: the features of every non-integer case keep |sum| >= SUM_MIN."""
    for route in kc.ROUTES:
        if kc.ROUTES[route][1] == 1:
            continue                                   # one channel: the "sum" is the value itself, in any order
        for case in (kc.offset_case(route, 1e2, 0.03, True), kc.width_case(route, 64), kc.count_case(route, 33, True),
                     kc.odd_valid_case(route), kc.tie_case(route)):
            assert kc.min_row_sum(case["x"]) >= kc.SUM_MIN, route
