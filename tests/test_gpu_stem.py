"""GPU: the encoder stem's Cin = 1 KPConv (k_kpconv_cin1: index rows staged in LDS, the wave's stop taken from the
staged rows, records gathered in batches) and the sine position embedding (k_posemb: one thread per sin / cos pair,
dim_t from LDS), at the shapes where their loops change path: query counts around the 16-query wave and the
64-query workgroup, row widths around the record batch (8) and the staged chunk (64 columns), strided rows, rows of
only shadow entries, unsorted rows with shadow and negative entries in the middle, sorted rows whose valid counts
differ inside one wave; token counts around the embedding's 16-token workgroup and both widths' zero tails.  Then the
stem operator spr_kpconv_stem (the first block in inference without its raw tensor) against the operator route
ops.kpconv -> ops.instnorm(slope=0.1) on a ragged batch: statistics, output bits, published range, batch invariance,
its workspace, and the shapes it refuses.

Bounds: KPConv against the float64 restatement of tests/forward_cases.py at 1e-5 of the output scale, the embedding
at 2e-6 of the scale or four times the float32 expression's own error (the rule of test_gpu_forward_range.py), zero
tails and repeated launches bit for bit."""
import numpy as np
import pytest
import torch

import forward_cases as fc
from superpoints_registration_amd import _lib, ops, stem
from workspace_arena import Arena

pytestmark = pytest.mark.gpu
T = torch.from_numpy
F64 = torch.float64
EXT = 0.125


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _features(ns, kind, seed):
    """[ns, 1]: the stem's column of ones, or random features of which about a third are exactly zero (the count
    takes features > 0 only)."""
    if kind == "ones":
        return np.ones((ns, 1), np.float32)
    r = fc.rng_of(701, seed, ns)
    x = (r.random((ns, 1)) * (r.random((ns, 1)) > 0.35)).astype(np.float32)
    x[0] = 0.75                      # query 0 coincides with support 0: the one-query, one-neighbour case stays live
    return x


def _run(device, q, s, nb, x, w, kp, srt, pad):
    """The neighbour rows as the kernel sees them: `pad` further columns behind kmax hold VALID indices the kernel
    must not read (nbr_stride = kmax + pad)."""
    nq, kmax = nb.shape
    wide = np.concatenate([nb, fc.rng_of(702, nq, kmax).integers(0, s.shape[0], (nq, pad))], 1).astype(np.int32)
    nbt = T(wide).to(device)[:, :kmax]
    assert nbt.stride(0) == kmax + pad
    args = (T(q).to(device), T(s).to(device), nbt, T(x).to(device), T(w).to(device), T(kp).to(device), EXT)
    y = ops.kpconv_raw(*args, rows_sorted=srt)
    assert torch.equal(_bits(y), _bits(ops.kpconv_raw(*args, rows_sorted=srt))), "two launches differ"
    return y


def _check(device, q, s, nb, x, w, kp, srt, pad, what):
    ref = fc.kpconv_f64(q, s, nb, x, w, kp, EXT)
    y = _run(device, q, s, nb, x, w, kp, srt, pad).cpu()
    assert torch.isfinite(y).all(), what
    scale = float(np.abs(ref).max())
    err = float(np.abs(y.double().numpy() - ref).max())
    print(f"{what}: err {err:.3e} scale {scale:.3e} ratio {err / max(1e-5 * scale, 1e-300):.3f}")
    assert scale > 0 and err <= 1e-5 * scale, f"{what}: {err:.3e} > 1e-5 * {scale:.3e}"
    return y, ref


@pytest.mark.parametrize("kmax", [1, 5, 40, 41])
@pytest.mark.parametrize("nq", [1, 15, 16, 17, 63, 65, 1000])
def test_cin1_gather_shapes(device, nq, kmax):
    """Every query count and row width, each with contiguous and strided rows, sorted (differing valid counts inside
    the 16-query groups: fill 0.7) and unsorted rows, ones and random positive / zero features; ns != nq."""
    ns = nq + 37
    w, kp = fc.kp_weights(1, 64, 71), fc.random_kernel_points(EXT, 72)
    for srt in (True, False):
        q, s, nb = fc.kp_cloud_case(nq, ns, kmax, 1e2, EXT, 73, rows_sorted=srt)
        if srt and nq >= 16 and kmax >= 5:
            assert len(set(((nb[:16] < ns).sum(1)).tolist())) > 1      # the wave's stop is not every query's count
        for pad in (0, 3):
            for kind in ("ones", "random"):
                _check(device, q, s, nb, _features(ns, kind, 74), w, kp, srt, pad,
                       f"cin1 nq {nq} kmax {kmax} srt={srt} stride {kmax + pad} x={kind}")


@pytest.mark.parametrize("kmax", [64, 65, 70, 130])
def test_cin1_gather_staged_chunks(device, kmax):
    """Rows wider than one staged chunk of 64 columns: waves whose rows end inside the first chunk sit out the later
    ones, the others go on (sorted); every chunk is walked whole (unsorted)."""
    nq, ns = 85, 200
    w, kp = fc.kp_weights(1, 64, 75), fc.random_kernel_points(EXT, 76)
    for srt in (True, False):
        q, s, nb = fc.kp_cloud_case(nq, ns, kmax, 1e2, EXT, 77, rows_sorted=srt, fill=0.6)
        if srt:
            nb[16:32, 20:] = ns                                          # a whole wave done after the first chunk
            nb[40, :] = np.argsort(np.linalg.norm(s.astype(np.float64) - q[40].astype(np.float64), axis=1))[:kmax]
        for pad in (0, 3):
            _check(device, q, s, nb, _features(ns, "random", 78), w, kp, srt, pad,
                   f"cin1 chunks kmax {kmax} srt={srt} stride {kmax + pad}")


@pytest.mark.parametrize("srt", [True, False])
def test_cin1_gather_shadow_rows_and_holes(device, srt):
    """Rows of only shadow entries give cnt = 0 and an exactly zero output row, in a wave of their own (queries
    16..31), among live rows and as the last rows; unsorted rows carry shadow (= ns, > ns) and negative entries in
    the middle, which contribute nothing."""
    nq, ns, kmax = 70, 120, 40
    q, s, nb = fc.kp_cloud_case(nq, ns, kmax, 1e2, EXT, 79, rows_sorted=srt)
    nb[16:32] = ns
    nb[[2, 37, 69]] = ns
    if not srt:
        r = fc.rng_of(703, 1)
        hole = r.random(nb.shape) < 0.2
        hole[:, 0] = False
        nb = np.where(hole, r.choice(np.array([-1, -7, ns, ns + 5]), nb.shape), nb)
        assert (nb[:, 1:-1] < 0).any() and (nb[:, 1:-1] > ns).any()
    w, kp = fc.kp_weights(1, 64, 80), fc.random_kernel_points(EXT, 81)
    for kind in ("ones", "random"):
        y, _ = _check(device, q, s, nb, _features(ns, kind, 82), w, kp, srt, 3, f"cin1 shadow rows srt={srt} x={kind}")
        dead = ~((nb >= 0) & (nb < ns)).any(1)
        assert dead[16:32].all() and dead[[2, 37, 69]].all()
        assert torch.equal(y[T(dead)], torch.zeros(int(dead.sum()), 64))


@pytest.mark.parametrize("cout", [16, 40, 64])
def test_cin1_gather_widths(device, cout):
    """Output widths: one and four 16-channel MFMA tiles, and 40 channels (the last tile half masked)."""
    nq, ns, kmax = 65, 90, 12
    w, kp = fc.kp_weights(1, cout, 83), fc.random_kernel_points(EXT, 84)
    for srt in (True, False):
        q, s, nb = fc.kp_cloud_case(nq, ns, kmax, 1e2, EXT, 85, rows_sorted=srt)
        y, _ = _check(device, q, s, nb, _features(ns, "random", 86), w, kp, srt, 0, f"cin1 cout {cout} srt={srt}")
        assert y.shape == (nq, cout)


# ---- the sine position embedding ------------------------------------------------------------------------------------
def _pe_xyz(n, seed):
    """Coordinates of every class in one tensor: exact zeros, negatives, O(1) values and magnitudes around 1e3 (the
    large-argument path of sinf / cosf: arguments of several thousand)."""
    r = fc.rng_of(704, seed, n)
    xyz = r.uniform(-1.0, 1.0, (n, 3)) * r.choice(np.array([0.0, 1.0, 30.0, 1e3]), (n, 3))
    xyz[0] = (0.0, -1e3, 977.25)
    return T(xyz.astype(np.float32))


@pytest.mark.parametrize("d_model", [256, 128])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_posemb_sine_pairs(device, n, d_model):
    """Token counts around the 16-token workgroup and the 64-lane wave; d_model 256 (npf 84, 4 zero channels) and 128
    (npf 42: the y and z blocks start at an odd pair of the row, 2 zero channels)."""
    xyz = _pe_xyz(n, 87)
    assert (xyz == 0).any() and (xyz < 0).any() and float(xyz.abs().max()) > 900.0
    npf = d_model // 3 // 2 * 2
    y = ops.posemb_sine(xyz.to(device), d_model, 1.0)
    assert y.shape == (n, d_model) and d_model - 3 * npf > 0
    ref64, base32 = fc.posemb_f64(xyz, d_model), fc.posemb_f32(xyz, d_model)
    got = y.cpu().to(F64)
    assert torch.isfinite(got).all()
    scale = float(ref64.abs().max())
    err, err32 = float((got - ref64).abs().max()), float((base32.to(F64) - ref64).abs().max())
    lim = max(2e-6 * scale, 4 * err32)
    print(f"posemb n={n} d={d_model}: err {err:.3e} scale {scale:.3e} err32 {err32:.3e} ratio {err / lim:.3f}")
    assert scale > 0 and err <= lim
    assert torch.equal(y[:, 3 * npf:].cpu(), torch.zeros(n, d_model - 3 * npf))
    assert torch.equal(_bits(y), _bits(ops.posemb_sine(xyz.to(device), d_model, 1.0)))
    # a token's row does not depend on its position in the workgroup or on its batch mates
    k = min(n, 21)
    assert torch.equal(_bits(ops.posemb_sine(xyz[n - k:].to(device), d_model, 1.0)), _bits(y[n - k:]))


# ---- the stem operator: KPConv (Cin = 1) + InstanceNorm + LeakyReLU without the raw tensor --------------------------
# cloud lengths around the 16-row MFMA group and the 512-row statistics slice, one empty cloud among them
STEM_LENGTHS = [1, 15, 16, 0, 17, 511, 512, 513, 1030]
STEM_KMAX = 20
_STEM = {}


def _stem_case(device, cout, kind):
    """One ragged batch per (cout, features), computed once: the inputs on the device, the operator route's raw
    tensor, statistics and output, and the fused call's output and statistics.  Seeds 91..94; with them the
    statistics of every cloud agree bit for bit at both widths and both feature kinds (printed by
    test_stem_statistics)."""
    key = (cout, kind)
    if key not in _STEM:
        nq, ns = sum(STEM_LENGTHS), sum(STEM_LENGTHS) + 85
        q, s, nb = fc.kp_cloud_case(nq, ns, STEM_KMAX, 1e2, EXT, 91, rows_sorted=True)
        wide = np.concatenate([nb, fc.rng_of(705, nq).integers(0, ns, (nq, 3))], 1).astype(np.int32)
        d = dict(q=T(q).to(device), s=T(s).to(device), nb=T(wide).to(device)[:, :STEM_KMAX],
                 x=T(_features(ns, kind, 92)).to(device), w=T(fc.kp_weights(1, cout, 93)).to(device),
                 kp=T(fc.random_kernel_points(EXT, 94)).to(device), cu=ops.lengths_to_cu(STEM_LENGTHS, device))
        d["ml"] = max(STEM_LENGTHS)
        d["raw"] = ops.kpconv_raw(d["q"], d["s"], d["nb"], d["x"], d["w"], d["kp"], EXT, rows_sorted=True)
        d["mean"], d["rstd"] = ops.instnorm_stats(d["raw"], d["cu"], max_len=d["ml"])
        d["ref"] = ops.instnorm(d["raw"], d["cu"], slope=0.1, max_len=d["ml"])
        d["out"], d["smean"], d["srstd"] = _stem_run(d, return_stats=True)
        _STEM[key] = d
    return _STEM[key]


def _stem_run(d, rows=None, **kw):
    """The fused call on the whole batch, or on the rows [a, b) as a batch of one cloud."""
    if rows is None:
        return stem.kpconv_stem(d["q"], d["s"], d["nb"], d["x"], d["w"], d["kp"], EXT, d["cu"], slope=0.1,
                                rows_sorted=True, max_len=d["ml"], **kw)
    a, b = rows
    cu = ops.lengths_to_cu([b - a], d["q"].device)
    return stem.kpconv_stem(d["q"][a:b], d["s"], d["nb"][a:b], d["x"], d["w"], d["kp"], EXT, cu, slope=0.1,
                            rows_sorted=True, max_len=b - a, **kw)


def _ulp_apart(a, b):
    """Per element: 0 = same bits, 1 = adjacent float32 (same sign), 2 = further apart."""
    ia, ib = _bits(a).to(torch.int64), _bits(b).to(torch.int64)
    dist = (ia - ib).abs()
    return torch.where(dist == 0, 0, torch.where((dist == 1) & ((ia < 0) == (ib < 0)), 1, 2))


@pytest.mark.parametrize("kind", ["ones", "random"])
@pytest.mark.parametrize("cout", [16, 64])
def test_stem_statistics(device, cout, kind):
    """k_stem_stats + k_in_final against ops.instnorm_stats of the materialised ops.kpconv output: every mean and
    rstd equal or the adjacent float32 (the two sum the same float64 terms in another order: at most 1e-10 relative,
    also through var = E[y^2] - m^2 on this data), at most 1 % adjacent; the empty cloud included."""
    d = _stem_case(device, cout, kind)
    for name, got, ref in (("mean", d["smean"], d["mean"]), ("rstd", d["srstd"], d["rstd"])):
        apart = _ulp_apart(got, ref)
        adjacent = int((apart == 1).sum())
        print(f"stem statistics cout {cout} x={kind} {name}: {adjacent} of {apart.numel()} entries adjacent")
        assert int((apart == 2).sum()) == 0, f"{name}: entries further than one float32 apart"
        assert adjacent <= 0.01 * apart.numel()


@pytest.mark.parametrize("kind", ["ones", "random"])
@pytest.mark.parametrize("cout", [16, 64])
def test_stem_output_and_range(device, cout, kind):
    """For every cloud whose statistics match bitwise the rows equal ops.kpconv -> ops.instnorm(slope=0.1) bit for
    bit; for the others within what one float32 step of the mean and of rstd moves the normalised value
    (ulp(mean) * rstd + 2^-22 |ref|).  The published range equals the operator route's."""
    d = _stem_case(device, cout, kind)
    out, ref = d["out"].cpu(), d["ref"].cpu()
    assert out.shape == ref.shape and torch.isfinite(out).all()
    exact = ((_ulp_apart(d["smean"], d["mean"]) == 0) & (_ulp_apart(d["srstd"], d["rstd"]) == 0)).all(1)
    off = 0
    for c, l in enumerate(STEM_LENGTHS):
        a, b = off, off + l
        off = b
        if exact[c]:
            assert torch.equal(_bits(out[a:b]), _bits(ref[a:b])), f"cloud {c} ({l} rows) differs from the operator route"
        else:
            m, r = d["mean"][c].cpu().double(), d["rstd"][c].cpu().double()
            lim = 1.01 * (torch.abs(m) * 2.0 ** -23 * r + ref[a:b].double().abs() * 2.0 ** -22)
            assert bool(((out[a:b].double() - ref[a:b].double()).abs() <= lim).all()), f"cloud {c} ({l} rows)"
    print(f"stem output cout {cout} x={kind}: {int(exact.sum())} of {len(STEM_LENGTHS)} clouds with bitwise statistics")
    (pa, na), (pb, nb_) = ops._get_range(d["out"]), ops._get_range(d["ref"])
    assert pa is not None and float(pa[:na].max()) == float(pb[:nb_].max()) == float(ref.abs().max())
    assert torch.equal(_bits(_stem_run(d)), _bits(d["out"])), "two launches differ"


@pytest.mark.parametrize("cout", [16, 64])
def test_stem_batch_invariance(device, cout):
    """A cloud's output rows and statistics have the same bits alone and among its batch mates: the statistics
    slices start at the cloud's first row, and a row's product does not depend on its 16-row group."""
    d = _stem_case(device, cout, "random")
    off = 0
    for c, l in enumerate(STEM_LENGTHS):
        a, b = off, off + l
        off = b
        if l == 0:
            continue
        alone, m, r = _stem_run(d, rows=(a, b), return_stats=True)
        assert torch.equal(_bits(alone), _bits(d["out"][a:b])), f"cloud {c} ({l} rows) differs inside the batch"
        assert torch.equal(_bits(m[0]), _bits(d["smean"][c])) and torch.equal(_bits(r[0]), _bits(d["srstd"][c]))


@pytest.mark.parametrize("poison", [0xFF, 0x00])
def test_stem_inside_exactly_its_workspace(device, monkeypatch, poison):
    """The call inside exactly spr_kpconv_stem_workspace_size bytes, poisoned (NaN / -1, or zeros) and between guard
    bands: production's bits, no guard byte touched; one byte less is refused before any launch."""
    d = _stem_case(device, 64, "random")
    arena = Arena(poison)
    monkeypatch.setattr(ops, "_workspace", arena)
    out = _stem_run(d)
    assert arena.calls == 1 and arena.records[0][1] == _lib.lib().spr_kpconv_stem_workspace_size(
        sum(STEM_LENGTHS), d["s"].shape[0], len(STEM_LENGTHS), d["ml"], 64)
    arena.verify()
    assert torch.equal(_bits(out), _bits(d["out"]))
    monkeypatch.setattr(ops, "_workspace", lambda n, dev: arena(n - 1, dev))
    with pytest.raises(RuntimeError, match="workspace too small"):
        _stem_run(d)
    arena.verify()


def test_stem_refuses_what_it_has_no_kernel_for(device):
    """cout = 40 stays on the operator route: the routing rule says no, the wrapper and the library refuse."""
    d = dict(_stem_case(device, 64, "ones"))
    d["w"] = T(fc.kp_weights(1, 40, 95)).to(device)
    with torch.no_grad():
        assert stem.stem_route(d["x"], d["w"], True) is False and stem.stem_route(d["x"], _STEM[(64, "ones")]["w"], True)
    with pytest.raises(RuntimeError, match="no kernel"):
        _stem_run(d)
    L = _lib.lib()
    nq, ns = sum(STEM_LENGTHS), d["s"].shape[0]
    ws = torch.empty(L.spr_kpconv_stem_workspace_size(nq, ns, len(STEM_LENGTHS), d["ml"], 40), dtype=torch.uint8, device=device)
    out = torch.empty((nq, 40), device=device)
    rc = L.spr_kpconv_stem(ops._ptr(d["q"]), nq, ops._ptr(d["s"]), ns, ops._ptr(d["nb"]), STEM_KMAX + 3, STEM_KMAX, 1,
                           ops._ptr(d["x"]), ops._ptr(d["w"]), 40, ops._ptr(d["kp"]), 15, EXT, ops._ptr(d["cu"]),
                           len(STEM_LENGTHS), d["ml"], 1e-5, 0.1, ops._ptr(out), None, 0, None, None, ops._ptr(ws),
                           ws.numel(), ops._stream(out))
    assert rc != 0 and b"no kernel" in L.spr_last_error()
    y = ops.instnorm(ops.kpconv_raw(d["q"], d["s"], d["nb"], d["x"], d["w"], d["kp"], EXT, rows_sorted=True), d["cu"],
                     slope=0.1, max_len=d["ml"])
    assert y.shape == (nq, 40) and torch.isfinite(y).all()
