"""GPU: the training augmentation operator (csrc/augment.hip, include/spr.h "8f-6") against the numpy float64
statement of its contract (tests/augment_replica.py).  Comparisons are exact unless a bound is named."""
import math

import numpy as np
import pytest
import torch

import augment_replica as ar
from conftest import load_golden
from superpoints_registration_amd import augment, get_config, ops, overlap, synthetic

pytestmark = pytest.mark.gpu
T = torch.from_numpy
U = 2.0 ** -24
R_MAX = math.sqrt(-2.0 * math.log(0.5 * 2.0 ** -23))      # the largest Box-Muller radius the uniform mapping can give


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(device, pairs, psrc, swap, perturb, mode, scale, max_pts=30000, seed=0, pair_keys=None, masks=None, corrs=None,
        noise=None, keys=None):
    """pairs: [(src, tgt, pose)] numpy; masks: [(src_mask, tgt_mask)] or None; corrs: [corr [2,K]] or None;
    noise / keys: per-pair [(noise_src, noise_tgt)] / [(keys_src, keys_tgt)] or None.  Returns per-pair dicts."""
    nb = len(pairs)
    sl, tl = [p[0].shape[0] for p in pairs], [p[1].shape[0] for p in pairs]
    cat = lambda xs, w, dt: T(np.concatenate([np.asarray(x, dt).reshape(-1, w) if w else np.asarray(x, dt).reshape(-1)
                                              for x in xs]) if xs else np.zeros((0, w) if w else (0,), dt)).to(device)
    kw = {}
    if masks is not None:
        kw["src_mask"], kw["tgt_mask"] = cat([m[0] for m in masks], 0, np.uint8), cat([m[1] for m in masks], 0, np.uint8)
    if corrs is not None:
        counts = [c.shape[1] for c in corrs]
        kw["corr"] = T(np.concatenate([np.asarray(c, np.int32).reshape(2, -1) for c in corrs], axis=1)).to(device)
        kw["corr_off"] = np.concatenate([[0], np.cumsum(counts)])[:nb]
        kw["corr_count"] = counts
    if noise is not None:
        kw["noise"] = cat([n[0] for n in noise] + [n[1] for n in noise], 3, np.float32)
    if keys is not None:
        kw["keys"] = T(np.concatenate([np.asarray(k[0], np.uint32) for k in keys]
                                      + [np.asarray(k[1], np.uint32) for k in keys]).view(np.int32)).to(device)
    out_s, out_t = augment.output_lengths(sl, tl, swap, max_pts)
    r = ops.augment_pairs(cat([p[0] for p in pairs], 3, np.float32), ops.lengths_to_cu(sl, device),
                          cat([p[1] for p in pairs], 3, np.float32), ops.lengths_to_cu(tl, device),
                          T(np.stack([p[2] for p in pairs]).astype(np.float32)).to(device), psrc, swap, perturb, mode,
                          scale, max_pts=max_pts, seed=seed, pair_keys=pair_keys, out_lens=(out_s, out_t), **kw)
    torch.cuda.synchronize()
    assert r["src_cu"].cpu().tolist() == np.concatenate([[0], np.cumsum(out_s)]).tolist()
    assert r["tgt_cu"].cpu().tolist() == np.concatenate([[0], np.cumsum(out_t)]).tolist()
    h = {k: v.cpu().numpy() for k, v in r.items()}
    res, bs, bt = [], 0, 0
    for b in range(nb):
        d = {"src_xyz": h["src_xyz"][bs:bs + out_s[b]], "tgt_xyz": h["tgt_xyz"][bt:bt + out_t[b]], "pose": h["pose"][b],
             "src_perm": h["src_perm"][bs:bs + out_s[b]], "tgt_perm": h["tgt_perm"][bt:bt + out_t[b]],
             "status": int(h["status"][b])}
        if masks is not None:
            d["src_mask"], d["tgt_mask"] = h["src_mask"][bs:bs + out_s[b]], h["tgt_mask"][bt:bt + out_t[b]]
        if corrs is not None:
            o, k = int(kw["corr_off"][b]), int(h["corr_count"][b])
            d["corr"] = h["corr"][:, o:o + k]
        res.append(d)
        bs, bt = bs + out_s[b], bt + out_t[b]
    return res


def assert_same(got, want, what, fields=("src_xyz", "tgt_xyz", "pose")):
    for f in fields:
        assert got[f].shape == want[f].shape, (what, f, got[f].shape, want[f].shape)
        assert np.array_equal(_bits(got[f]), _bits(want[f])), (what, f)
    for f in ("src_perm", "tgt_perm", "src_mask", "tgt_mask", "corr"):
        if want.get(f) is not None and f in got:
            assert np.array_equal(np.asarray(got[f]).astype(np.int64), np.asarray(want[f]).astype(np.int64)), (what, f)


def _case(g, name):
    return {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + ".")}


def _keys_from_perm(perm):
    k = np.empty(perm.shape[0], dtype=np.uint32)
    k[perm] = np.arange(perm.shape[0], dtype=np.uint32) * np.uint32(1000) + np.uint32(17)
    return k


# ---- 1. fixture ----------------------------------------------------------------------------------------------------
def test_fixture_bit_exact_against_the_float64_contract(device):
    g = load_golden("augment_ops.npz")
    max_pts = int(g["max_pts"])
    for mode in ("small", "large"):
        names = [str(n) for n in g["cases"] if str(g[f"{n}.mode"]) == mode]
        assert len(names) == 2
        cs = [_case(g, n) for n in names]
        for c in cs:                       # exact float64 centroid sums in any order
            for pts in (c["src"], c["tgt"]):
                p = pts.astype(np.float64)
                for d in range(3):
                    assert sum(p[:, d].tolist()) == sum(p[::-1, d].tolist()) == math.fsum(p[:, d])
        # one jitter scale per call: every case of a mode shares it in the fixture
        assert len({float(c["scale"]) for c in cs}) == 1
        scale = float(cs[0]["scale"])
        keys = [(_keys_from_perm(c["perm_src"]), _keys_from_perm(c["perm_tgt"])) for c in cs]
        got = run(device, [(c["src"], c["tgt"], c["pose"]) for c in cs], [bool(c["perturb_src"]) for c in cs],
                  [bool(c["swap"]) for c in cs], np.stack([c["perturb"] for c in cs]), mode, scale, max_pts=max_pts,
                  masks=[(c["src_overlap"], c["tgt_overlap"]) for c in cs], corrs=[c["corr"] for c in cs],
                  noise=[(c["noise_src"], c["noise_tgt"]) for c in cs], keys=keys)
        for c, k, gp, name in zip(cs, keys, got, names):
            want = ar.apply_pair(c["src"], c["tgt"], c["pose"], c["perturb"], bool(c["perturb_src"]), bool(c["swap"]),
                                 mode, scale, max_pts, c["noise_src"], c["noise_tgt"], k[0], k[1], c["src_overlap"],
                                 c["tgt_overlap"], c["corr"])
            assert gp["status"] == 0
            assert_same(gp, want, name)
            # the integer outputs are the reference's own
            assert np.array_equal(gp["src_mask"].astype(bool), c["ref_src_overlap"])
            assert np.array_equal(gp["tgt_mask"].astype(bool), c["ref_tgt_overlap"])
            assert np.array_equal(gp["corr"].astype(np.int64), c["ref_corr"])
            perms = [c["perm_src"][:max_pts], c["perm_tgt"][:max_pts]]
            perms = perms[::-1] if bool(c["swap"]) else perms
            assert np.array_equal(gp["src_perm"], perms[0]) and np.array_equal(gp["tgt_perm"], perms[1])


# ---- 2. draws ------------------------------------------------------------------------------------------------------
def test_draw_buffers_against_the_numpy_philox(device):
    seed, pair_keys = 0xC0FFEE1234, [5, 2 ** 33 + 1, 77]
    sl, tl = [60001, 0, 70000], [50000, 65537, 110000]
    ns, nt = sum(sl), sum(tl)
    _, _, _, noise, keys = ops.augment_draw(seed, pair_keys, "small", ops.lengths_to_cu(sl, device),
                                            ops.lengths_to_cu(tl, device), ns, nt)
    torch.cuda.synchronize()
    noise, keys = noise.cpu().numpy().astype(np.float64), keys.cpu().numpy().view(np.uint32)
    want_k, want_n, want_r = [], [], []
    for side, lens in ((0, sl), (1, tl)):
        for pk, n in zip(pair_keys, lens):
            want_k.append(ar.keys(seed, pk, side, n))
            nz, r = ar.noise64(seed, pk, side, n)
            want_n.append(nz)
            want_r.append(r)
    assert np.array_equal(keys, np.concatenate(want_k))
    want_n, want_r = np.concatenate(want_n), np.concatenate(want_r)
    # three float32 roundings of factors (<= 3 * 2^-24 relative), the rounding of the angle 2 pi u (<= 2 pi 2^-24
    # absolute in the cosine), <= 2 ulp per library function: together below 2e-6 * r
    err = np.abs(noise - want_n)
    print("noise: max err / r =", float((err / want_r).max()))
    assert np.all(err <= 2e-6 * want_r)
    v = noise.reshape(-1)
    n = v.size
    assert n >= 10 ** 6
    k = 5.0                                                       # 5 sigma of each estimator
    assert abs(v.mean()) <= k / math.sqrt(n)
    assert abs(v.var() - 1.0) <= k * math.sqrt(2.0 / n)
    # lag-1 over consecutive values (x|y of one point share a radius but are uncorrelated; y|z and z|x' independent)
    assert abs(np.mean(v[:-1] * v[1:])) <= k / math.sqrt(n)
    assert abs(np.mean(noise[:-1] * noise[1:])) <= k / math.sqrt(n)   # the same component of consecutive points


# ---- helpers for the synthetic cases ---------------------------------------------------------------------------------
def decisions(seed, pair_keys, mode):
    return ops.augment_draw(seed, pair_keys, mode)


# ---- 3. inline equals explicit -------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["small", "large"])
def test_inline_draws_equal_explicit_buffers(device, mode):
    seed, pair_keys = 31337, [9, 10, 2 ** 35]
    pairs = [synthetic.make_pair(n, seed=s) for n, s in ((3000, 1), (1, 2), (4097, 3))]
    pairs[1] = (pairs[1][0], pairs[2][1][:130], pairs[1][2])
    sl, tl = [p[0].shape[0] for p in pairs], [p[1].shape[0] for p in pairs]
    psrc, swap, P, noise, keys = ops.augment_draw(seed, pair_keys, mode, ops.lengths_to_cu(sl, device),
                                                  ops.lengths_to_cu(tl, device), sum(sl), sum(tl))
    noise, keys = noise.cpu().numpy(), keys.cpu().numpy().view(np.uint32)
    so, to = np.concatenate([[0], np.cumsum(sl)]), sum(sl) + np.concatenate([[0], np.cumsum(tl)])
    nz = [(noise[so[b]:so[b + 1]], noise[to[b]:to[b + 1]]) for b in range(3)]
    ky = [(keys[so[b]:so[b + 1]], keys[to[b]:to[b + 1]]) for b in range(3)]
    rng = np.random.default_rng(0)
    masks = [(rng.random(a) > 0.5, rng.random(b) > 0.5) for a, b in zip(sl, tl)]
    corrs = [np.stack([rng.integers(0, a, 500), rng.integers(0, b, 500)]) for a, b in zip(sl, tl)]
    inline = run(device, pairs, psrc, swap, P, mode, 0.01, max_pts=2500, seed=seed, pair_keys=pair_keys, masks=masks,
                 corrs=corrs)
    explicit = run(device, pairs, psrc, swap, P, mode, 0.01, max_pts=2500, masks=masks, corrs=corrs, noise=nz, keys=ky)
    for b in range(3):
        assert_same(inline[b], explicit[b], f"pair {b}")
        want = ar.apply_pair(*pairs[b], P[b], psrc[b], swap[b], mode, 0.01, 2500, nz[b][0], nz[b][1], ky[b][0], ky[b][1],
                             masks[b][0], masks[b][1], corrs[b])
        if mode == "large":
            assert_same(inline[b], want, f"pair {b} vs contract")
            continue
        # small: the float64 centroid sum of a real (unquantised) cloud depends on the summation order by n * 2^-53
        # relative -- far below a float32 ulp, but able to flip the centroid's rounding: integers exact, coordinates
        # and pose within what one ulp of the centroid (|c| < 4) moves them by, (|R| + 1) * 2^-23 * 4 < 8 * 2^-24 * 8
        assert_same(inline[b], want, f"pair {b} vs contract", fields=())
        for f in ("src_xyz", "tgt_xyz", "pose"):
            assert np.abs(inline[b][f].astype(np.float64) - want[f].astype(np.float64)).max() <= 8 * U * 8.0


# ---- 4. batch independence -----------------------------------------------------------------------------------------
def test_a_pair_is_augmented_identically_in_any_batch_and_stream(device):
    seed, key, mode = 4242, 987654321, "small"
    pair = synthetic.make_pair(5000, seed=11)
    rng = np.random.default_rng(3)
    mask = (rng.random(5000) > 0.5, rng.random(5000) > 0.3)
    corr = np.stack([rng.integers(0, 5000, 1200), rng.integers(0, 5000, 1200)])
    psrc, swap, P = decisions(seed, [key], mode)
    alone = run(device, [pair], psrc, swap, P, mode, 0.005, max_pts=4000, seed=seed, pair_keys=[key], masks=[mask],
                corrs=[corr])[0]
    others = [synthetic.make_pair(1000 + 37 * i, seed=50 + i) for i in range(16)]
    pairs, keys16 = list(others), [1000 + i for i in range(16)]
    pairs[11], keys16[11] = pair, key
    masks = [(rng.random(p[0].shape[0]) > 0.5, rng.random(p[1].shape[0]) > 0.5) for p in pairs]
    corrs = [np.stack([rng.integers(0, p[0].shape[0], 300), rng.integers(0, p[1].shape[0], 300)]) for p in pairs]
    masks[11], corrs[11] = mask, corr
    psrc16, swap16, P16 = decisions(seed, keys16, mode)
    batch = run(device, pairs, psrc16, swap16, P16, mode, 0.005, max_pts=4000, seed=seed, pair_keys=keys16, masks=masks,
                corrs=corrs)[11]
    assert_same(batch, alone, "position 11 of 16")
    assert batch["corr"].shape[1] > 0 and batch["src_xyz"].shape[0] == 4000
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        again = run(device, [pair], psrc, swap, P, mode, 0.005, max_pts=4000, seed=seed, pair_keys=[key], masks=[mask],
                    corrs=[corr])[0]
    assert_same(again, alone, "second stream")


# ---- 5. label consistency ------------------------------------------------------------------------------------------
def _nearest_d2(a, b):
    """nearest squared distance of every row of a to b, float64 (expansion form: error ~1e-15, far below the margin)."""
    out = np.empty(a.shape[0])
    bb = (b * b).sum(axis=1)
    for i in range(0, a.shape[0], 4096):
        x = a[i:i + 4096]
        out[i:i + 4096] = ((x * x).sum(axis=1)[:, None] + bb[None] - 2.0 * (x @ b.T)).min(axis=1)
    return out


# Partially overlapping 16 384-point pairs: random two thirds of each side of a 24 576-point synthetic pair.  The
# seeds are chosen (on the CPU, from the numpy computation asserted below) so that no point's nearest squared distance
# lies within 1e-4 (relative) of r^2: the closest are 3.6e-4 and 2.2e-4 away, above what the float32 rounding of the
# augmented coordinates and pose can move a distance by (<= 6e-5 at |x| < 5, r = 0.0375).
LABEL_SEEDS = (20, 26)


def label_pairs():
    out = []
    for s in LABEL_SEEDS:
        src, tgt, pose = synthetic.make_pair(24576, seed=s, extent=4.0)
        out.append((src[:16384].copy(), tgt[:16384].copy(), pose))
    return out


def test_masks_survive_augmentation_and_relabelling(device):
    cfg = get_config("3dmatch")
    radius = cfg.overlap_radius
    pairs = label_pairs()
    for src, tgt, pose in pairs:                                  # no point sits within 1e-4 (relative) of r^2
        moved = src.astype(np.float64) @ pose[:, :3].astype(np.float64).T + pose[:, 3].astype(np.float64)
        for d2 in (_nearest_d2(moved, tgt.astype(np.float64)), _nearest_d2(tgt.astype(np.float64), moved)):
            assert np.all(np.abs(d2 / radius ** 2 - 1.0) > 1e-4), float(np.abs(d2 / radius ** 2 - 1.0).min())
    batch = {"src_xyz": [T(p[0]).to(device) for p in pairs], "tgt_xyz": [T(p[1]).to(device) for p in pairs],
             "pose": T(np.stack([p[2] for p in pairs])).to(device), "src_path": ["s0", "s1"], "tgt_path": ["t0", "t1"]}
    overlap.label_batch(batch, radius)
    frac = float(torch.cat(batch["src_overlap"]).float().mean())
    assert 0.5 < frac < 0.99, frac
    cfg0 = get_config("3dmatch")
    cfg0.augment_noise = 0.0
    keys = [3, 4]
    aug = augment.augment_batch(batch, cfg0, 77, keys)
    assert aug is not batch and aug["src_xyz"][0] is not batch["src_xyz"][0]
    psrc, swap, _ = ops.augment_draw(77, keys, cfg.perturb_pose)
    for b in range(2):
        assert aug["src_path"][b] == ("t%d" % b if swap[b] else "s%d" % b)
    relabelled = overlap.label_batch({"src_xyz": aug["src_xyz"], "tgt_xyz": aug["tgt_xyz"], "pose": aug["pose"]}, radius)
    for b in range(2):                                            # every point is compared
        assert aug["src_overlap"][b].shape[0] == 16384
        assert torch.equal(relabelled["src_overlap"][b], aug["src_overlap"][b])
        assert torch.equal(relabelled["tgt_overlap"][b], aug["tgt_overlap"][b])
        # the carried correspondences still point at each other's partners: both ends are masked points
        c = aug["correspondences"][b]
        assert c.shape[1] == batch["correspondences"][b].shape[1] > 0
        assert bool(aug["src_overlap"][b][c[0]].all()) and bool(aug["tgt_overlap"][b][c[1]].all())


def test_jitter_stays_within_its_bound_and_the_pose_still_registers(device):
    mode, seed, keys, scale = "large", 5, [100, 101, 102, 103], 0.01
    pairs = []
    for s in range(4):
        src, _, pose = synthetic.make_pair(16384, seed=30 + s, jitter=0.0)
        tgt = (src.astype(np.float64) @ pose[:, :3].astype(np.float64).T + pose[:, 3].astype(np.float64)).astype(np.float32)
        pairs.append((src, tgt, pose))
    psrc, swap, P = decisions(seed, keys, mode)
    clean = run(device, pairs, psrc, swap, P, mode, 0.0, seed=seed, pair_keys=keys)
    noisy = run(device, pairs, psrc, swap, P, mode, scale, seed=seed, pair_keys=keys)
    for b in range(4):
        for f in ("src_xyz", "tgt_xyz"):
            d = np.abs(noisy[b][f].astype(np.float64) - clean[b][f].astype(np.float64))
            assert d.max() > 0.5 * scale
            # |noise| <= r_max per coordinate; one rounding of the product and one of the sum
            assert np.all(d <= scale * R_MAX * (1 + 2 * U) + U * (np.abs(clean[b][f]) + scale * R_MAX))
        assert np.array_equal(noisy[b]["src_perm"], clean[b]["src_perm"])
        # pose' maps the un-jittered source onto the un-jittered target (same original index), to float32 rounding:
        # the target's own rounding, the perturbation's and the composed pose's entries, <= 32 u (|x|_1 + |t|_1 + 1)
        G = clean[b]["pose"].astype(np.float64)
        x = clean[b]["src_xyz"].astype(np.float64)
        back = np.empty(16384, dtype=np.int64)
        back[clean[b]["tgt_perm"]] = np.arange(16384)
        y = clean[b]["tgt_xyz"].astype(np.float64)[back[clean[b]["src_perm"]]]
        err = np.abs(x @ G[:, :3].T + G[:, 3] - y)
        bound = 32 * U * (np.abs(x).sum(axis=1, keepdims=True) + np.abs(G[:, 3]).sum() + np.abs(P[b][:, 3]).sum() + 1.0)
        assert np.all(err <= bound), float((err / bound).max())


# ---- 6. edges ------------------------------------------------------------------------------------------------------
def _check_against_contract(device, pairs, mode, scale, max_pts, seed, keys, masks=None, corrs=None):
    psrc, swap, P = decisions(seed, keys, mode)
    got = run(device, pairs, psrc, swap, P, mode, scale, max_pts=max_pts, seed=seed, pair_keys=keys, masks=masks,
              corrs=corrs)
    for b, (src, tgt, pose) in enumerate(pairs):
        nz = [np.zeros((c.shape[0], 3), np.float32) for c in (src, tgt)]
        ky = [ar.keys(seed, keys[b], s, c.shape[0]) for s, c in enumerate((src, tgt))]
        want = ar.apply_pair(src, tgt, pose, P[b], psrc[b], swap[b], mode, 0.0, max_pts, nz[0], nz[1], ky[0], ky[1],
                             None if masks is None else masks[b][0], None if masks is None else masks[b][1],
                             None if corrs is None else corrs[b])
        assert got[b]["status"] == 0
        assert_same(got[b], want, f"pair {b}")
    return got


def _quantised_pair(n, m, seed):
    src, tgt, pose = synthetic.make_pair(max(n, m, 1), seed=seed)
    q = lambda x: (np.round(x.astype(np.float64) * 4096.0) / 4096.0).astype(np.float32)
    return q(src[:n]), q(tgt[:m]), pose


def test_edges_empty_clouds_single_pair_and_modes(device):
    rng = np.random.default_rng(9)
    pairs = [_quantised_pair(0, 40, 1), _quantised_pair(50, 0, 2), _quantised_pair(33, 21, 3), _quantised_pair(0, 0, 4)]
    masks = [(rng.random(p[0].shape[0]) > 0.5, rng.random(p[1].shape[0]) > 0.5) for p in pairs]
    corrs = [np.zeros((2, 0), np.int64), np.zeros((2, 0), np.int64),
             np.stack([rng.integers(0, 33, 15), rng.integers(0, 21, 15)]), np.zeros((2, 0), np.int64)]
    for mode in ("none", "small", "large"):                       # scale = 0 throughout: exact against the contract
        _check_against_contract(device, pairs, mode, 0.0, 30000, 8, [1, 2, 3, 4], masks, corrs)
        _check_against_contract(device, pairs[2:3], mode, 0.0, 30000, 8, [3], masks[2:3], corrs[2:3])   # nb = 1
        _check_against_contract(device, pairs, mode, 0.0, 30000, 8, [1, 2, 3, 4])                       # no masks at all
    got = _check_against_contract(device, pairs[2:3], "none", 0.0, 30000, 8, [3], masks[2:3], corrs[2:3])[0]
    # mode none, scale 0: a pure shuffle (and swap) of the inputs
    swap = ops.augment_draw(8, [3], "none")[1][0]
    a, b = (pairs[2][1], pairs[2][0]) if swap else (pairs[2][0], pairs[2][1])
    assert np.array_equal(got["src_xyz"], a[got["src_perm"]]) and np.array_equal(got["tgt_xyz"], b[got["tgt_perm"]])


@pytest.mark.parametrize("max_pts", [1, 32, 33, 34])
def test_edges_max_pts_around_the_length(device, max_pts):
    rng = np.random.default_rng(10)
    pair = _quantised_pair(33, 33, 5)
    mask = (rng.random(33) > 0.5, rng.random(33) > 0.5)
    corr = np.stack([rng.integers(0, 33, 40), rng.integers(0, 33, 40)])
    for mode in ("small", "large"):
        got = _check_against_contract(device, [pair], mode, 0.0, max_pts, 12, [6], [mask], [corr])[0]
        assert got["src_xyz"].shape[0] == min(33, max_pts)


def test_edges_nan_in_one_pair_flags_that_pair_only(device):
    pairs = [_quantised_pair(40, 30, 1), _quantised_pair(35, 45, 2), _quantised_pair(20, 25, 3)]
    keys, seed = [1, 2, 3], 3
    psrc, swap, P = decisions(seed, keys, "small")
    clean = run(device, pairs, psrc, swap, P, "small", 0.005, seed=seed, pair_keys=keys)
    bad = list(pairs)
    tg = pairs[1][1].copy()
    tg[7, 1] = np.nan
    bad[1] = (pairs[1][0], tg, pairs[1][2])
    got = run(device, bad, psrc, swap, P, "small", 0.005, seed=seed, pair_keys=keys)
    assert [g["status"] for g in got] == [0, 1, 0]
    for b in (0, 2):
        assert_same(got[b], clean[b], f"pair {b} beside a NaN pair")
    inf_pose = list(pairs)
    ps = pairs[2][2].copy()
    ps[0, 3] = np.inf
    inf_pose[2] = (pairs[2][0], pairs[2][1], ps)
    assert [g["status"] for g in run(device, inf_pose, psrc, swap, P, "small", 0.005, seed=seed, pair_keys=keys)] == [0, 0, 1]
    batch = {"src_xyz": [T(p[0]).to(device) for p in bad], "tgt_xyz": [T(p[1]).to(device) for p in bad],
             "pose": T(np.stack([p[2] for p in bad])).to(device)}
    with pytest.raises(RuntimeError, match=r"non-finite.*\[1\]"):
        augment.augment_batch(batch, get_config("3dmatch"), seed, keys)


def test_edges_duplicate_shuffle_keys_keep_a_stable_order(device):
    pair = _quantised_pair(64, 48, 6)
    ks = (np.arange(64, dtype=np.uint32)[::-1] // 8).astype(np.uint32)       # eight runs of eight equal keys
    kt = np.zeros(48, dtype=np.uint32)                                       # all equal: the identity
    nz = (np.zeros((64, 3), np.float32), np.zeros((48, 3), np.float32))
    P = np.eye(3, 4, dtype=np.float32)[None]
    got = run(device, [pair], [True], [False], P, "none", 0.0, noise=[nz], keys=[(ks, kt)])[0]
    assert np.array_equal(got["src_perm"], np.argsort(ks, kind="stable"))
    assert np.array_equal(got["tgt_perm"], np.arange(48))
    assert np.array_equal(got["src_xyz"], pair[0][got["src_perm"]]) and np.array_equal(got["tgt_xyz"], pair[1])


# ---- 7. trainer ----------------------------------------------------------------------------------------------------
def test_trainer_augments_reproducibly_and_leaves_the_batch_alone(device):
    from superpoints_registration_amd.regtr import RegTR
    from superpoints_registration_amd.training import Trainer
    cfg = get_config("3dmatch")
    raw = [synthetic.make_pair(2048, seed=3 + i, extent=0.6, jitter=0.002) for i in range(2)]

    def fresh():
        return {"src_xyz": [T(p[0]).to(device) for p in raw], "tgt_xyz": [T(p[1]).to(device) for p in raw],
                "pose": T(np.stack([p[2] for p in raw])).to(device)}

    def two_steps(**kw):
        model = RegTR(cfg)
        synthetic.fill_parameters(model, seed=0)
        model = model.to(device)
        tr = Trainer(cfg, **kw).setup(model)
        batch = fresh()
        keep = {"src": [t.clone() for t in batch["src_xyz"]], "pose": batch["pose"].clone(), "keys": sorted(batch)}
        out = [tr.train_step(model, batch), tr.train_step(model, batch)]
        return out, batch, keep

    a, batch, keep = two_steps(augment=True, seed=17)
    assert sorted(batch) == keep["keys"]                           # no labels, nothing added
    assert all(torch.equal(x, y) for x, y in zip(batch["src_xyz"], keep["src"])) and torch.equal(batch["pose"], keep["pose"])
    for losses in a:
        assert all(bool(torch.isfinite(v).all()) for v in losses.values()), losses
    b, _, _ = two_steps(augment=True, seed=17)
    for la, lb in zip(a, b):
        assert sorted(la) == sorted(lb)
        for k in la:
            assert torch.equal(la[k], lb[k]), k                    # bit-reproducible across fresh runs
    c, _, _ = two_steps(augment=True, seed=18)
    assert any(not torch.equal(a[0][k], c[0][k]) for k in a[0])    # another seed, another augmentation
    off, _, _ = two_steps(augment=False)
    plain, _, _ = two_steps()
    for lo, lp in zip(off, plain):
        for k in lo:
            assert torch.equal(lo[k], lp[k]), k
    assert any(not torch.equal(a[0][k], plain[0][k]) for k in a[0])
