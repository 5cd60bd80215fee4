"""GPU: the ModelNet pair generator (csrc/modelnet_pairs.hip, include/spr.h "8f-7") against the numpy float64
statement of its contract (tests/modelnet_replica.py).  Comparisons are exact unless a bound is named."""
import numpy as np
import pytest
import torch

import modelnet_replica as mr
from conftest import load_golden
from superpoints_registration_amd import _lib, get_config, modelnet, ops
from tensor_arena import TensorArena
from workspace_arena import GUARD, Arena

pytestmark = pytest.mark.gpu
T = torch.from_numpy
U = 2.0 ** -24
P07 = (0.7, 0.7)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _i32(a):
    return T(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32))


def shape_cloud(n, seed):
    """An unquantised lumpy shell of n float32 points inside the unit ball."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True) * (0.5 + 0.4 * rng.random((n, 1)))).astype(np.float32)


def run(device, clouds, k, dirs, tf, p=P07, scale=0.01, clip=0.05, seed=0, keys=None, draws=None, put=lambda t: t):
    """clouds: list of [n_b,3] float32 arrays; dirs [nb,2,3], tf [nb,3,4]; draws: per-pair list of dicts with rkeys
    [2,n_b], extra [2,k], noise [2,k,3], skeys [2,k] (explicit buffers) or None (inline from seed / keys).
    Returns (per-pair dicts of numpy arrays, the raw result)."""
    nb, lens = len(clouds), [c.shape[0] for c in clouds]
    xyz = T(np.concatenate(clouds).astype(np.float32).reshape(-1, 3)).to(device)
    kw = {}
    if draws is not None:
        cat = lambda f: np.concatenate([d[f] for d in draws], axis=1)
        kw = {"rkeys": put(_i32(cat("rkeys")).to(device)), "extra": put(_i32(cat("extra")).to(device)),
              "noise": put(T(cat("noise").astype(np.float32)).to(device)), "skeys": put(_i32(cat("skeys")).to(device))}
    r = modelnet.modelnet_pairs(put(xyz), put(ops.lengths_to_cu(lens, device)), max(lens), p, k,
                                put(T(np.asarray(tf, np.float32)).to(device)), put(T(np.asarray(dirs, np.float64)).to(device)),
                                scale=scale, clip=clip, seed=seed, pair_keys=keys, **kw)
    torch.cuda.synchronize()
    h = {f: v.cpu().numpy() for f, v in r.items()}
    out = []
    for b in range(nb):
        sl = slice(b * k, (b + 1) * k)
        cnt = int(h["corr_count"][b])
        out.append({"src_xyz": h["src_xyz"][sl], "tgt_xyz": h["tgt_xyz"][sl], "pose": h["pose"][b],
                    "src_overlap": h["src_overlap"][sl], "tgt_overlap": h["tgt_overlap"][sl],
                    "src_index": h["src_index"][sl], "tgt_index": h["tgt_index"][sl],
                    "corr": h["corr"][:, b * k:b * k + cnt], "status": int(h["status"][b])})
    return out, r


FLOATS, INTS = ("src_xyz", "tgt_xyz", "pose"), ("src_overlap", "tgt_overlap", "src_index", "tgt_index", "corr")


def assert_same(got, want, what):
    assert got["status"] == want["status"], (what, got["status"], want["status"])
    for f in FLOATS:
        assert got[f].shape == want[f].shape, (what, f)
        assert np.array_equal(_bits(got[f]), _bits(want[f])), (what, f)
    for f in INTS:
        assert np.array_equal(np.asarray(got[f]).astype(np.int64), np.asarray(want[f]).astype(np.int64)), (what, f)


def contract_draws(seed, key, n, k, noise=None):
    """The per-point draws of one pair from the numpy Philox; noise (device float32 arithmetic) must be handed in."""
    return {"rkeys": np.stack([mr.resample_keys(seed, key, s, n) for s in range(2)]),
            "extra": np.stack([mr.extra_words(seed, key, s, k) for s in range(2)]),
            "skeys": np.stack([mr.shuffle_keys(seed, key, s, k) for s in range(2)]),
            "noise": np.zeros((2, k, 3), np.float32) if noise is None else noise}


def replica(cloud, k, dirs, tf, d, p=P07, scale=0.01, clip=0.05):
    q = tuple(mr.percentile_q(x) for x in p)
    return mr.make_pair(cloud, p, q, k, scale, clip, tf, dirs, d["rkeys"], d["extra"], d["noise"], d["skeys"])


def device_draws(device, seed, keys, lens, k, rot=45.0, trans=0.5):
    """(dirs, tf, per-pair explicit draw dicts) through spr_modelnet_draw."""
    nb, n_total = len(lens), sum(lens)
    dirs, tf, rk, ex, nz, sk = modelnet.modelnet_draw(seed, keys, rot, trans, ops.lengths_to_cu(lens, device), n_total, k)
    torch.cuda.synchronize()
    rk, ex, sk = (t.cpu().numpy().view(np.uint32) for t in (rk, ex, sk))
    nz = nz.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(lens)])
    draws = [{"rkeys": rk[:, off[b]:off[b + 1]], "extra": ex[:, b * k:(b + 1) * k], "noise": nz[:, b * k:(b + 1) * k],
              "skeys": sk[:, b * k:(b + 1) * k]} for b in range(nb)]
    return dirs, tf, draws


# ---- 1. explicit draws: bit-equal to the contract --------------------------------------------------------------------
def _case(g, name):
    return {f[len(name) + 1:]: v for f, v in g.items() if f.startswith(name + ".")}


def test_fixture_cases_bit_exact_against_the_float64_contract(device):
    g = load_golden("modelnet_pairs.npz")
    scale, clip = float(g["scale"]), float(g["clip"])
    for names in (("down_64_32", "opposed_200_32"), ("up_300_717",)):          # one call per output size
        cs = [_case(g, n) for n in names]
        k = int(cs[0]["k"])
        got, _ = run(device, [c["xyz"] for c in cs], k, np.stack([c["dirs"] for c in cs]),
                     np.stack([c["transform"] for c in cs]), scale=scale, clip=clip, draws=cs)
        for name, c, gp in zip(names, cs, got):
            assert_same(gp, replica(c["xyz"], k, c["dirs"], c["transform"], c, scale=scale, clip=clip), name)
            # the integer outputs are the reference's own
            assert np.array_equal(gp["src_overlap"].astype(bool), c["ref_src_overlap"])
            assert np.array_equal(gp["tgt_overlap"].astype(bool), c["ref_tgt_overlap"])
            assert np.array_equal(gp["src_index"], c["ref_src_index"]) and np.array_equal(gp["tgt_index"], c["ref_tgt_index"])
            assert np.array_equal(gp["corr"].astype(np.int64), c["ref_corr"])


def test_real_shape_four_clouds_of_2048_to_717(device):
    seed, keys, lens, k = 99, [11, 12, 13, 2 ** 40 + 5], [2048] * 4, 717
    clouds = [shape_cloud(2048, 40 + b) for b in range(4)]
    dirs, tf, draws = device_draws(device, seed, keys, lens, k)
    got, _ = run(device, clouds, k, dirs, tf, draws=draws)
    for b in range(4):
        want = replica(clouds[b], k, dirs[b], tf[b], draws[b])
        assert_same(got[b], want, f"shape {b}")
        assert 100 < got[b]["corr"].shape[1] < 717 and 0.2 < got[b]["src_overlap"].mean() < 0.95


# ---- 2. draws ----------------------------------------------------------------------------------------------------------
def test_inline_draws_equal_explicit_buffers_and_the_numpy_philox(device):
    seed, keys, lens, k = 31337, [9, 10, 2 ** 35], [300, 2048, 1000], 717     # pair 0 up-samples: its extras are used
    clouds = [shape_cloud(n, 7 + b) for b, n in enumerate(lens)]
    dirs, tf, draws = device_draws(device, seed, keys, lens, k)
    for b, (key, n) in enumerate(zip(keys, lens)):
        want = contract_draws(seed, key, n, k)
        for f in ("rkeys", "extra", "skeys"):
            assert np.array_equal(draws[b][f], want[f]), (b, f)
        for s in range(2):
            nz, r = mr.noise64(seed, key, s, k)
            # the bound of tests/test_gpu_augment.py:141-145: three float32 roundings of factors, the rounding of the
            # angle, <= 2 ulp per library function: together below 2e-6 * r
            assert np.all(np.abs(draws[b]["noise"][s].astype(np.float64) - nz) <= 2e-6 * r), (b, s)
    inline, _ = run(device, clouds, k, dirs, tf, seed=seed, keys=keys)
    explicit, _ = run(device, clouds, k, dirs, tf, draws=draws)
    for b in range(3):
        assert_same(inline[b], explicit[b], f"pair {b}")
        assert_same(inline[b], replica(clouds[b], k, dirs[b], tf[b], draws[b]), f"pair {b} vs contract")
    assert np.unique(inline[0]["src_index"]).size < k


# ---- 3. batch independence ---------------------------------------------------------------------------------------------
def test_a_pair_is_generated_identically_in_any_batch_position_and_stream(device):
    seed, key, k = 4242, 987654321, 717
    cloud = shape_cloud(2048, 3)
    d1, t1 = modelnet.modelnet_draw(seed, [key], 45.0, 0.5)
    alone = run(device, [cloud], k, d1, t1, seed=seed, keys=[key])[0][0]
    assert alone["status"] == 0 and alone["corr"].shape[1] > 0
    lens = [2048, 777, 1500, 64, 2048]
    for pos in (0, 4):
        keys5 = [1000 + i for i in range(5)]
        clouds = [shape_cloud(n, 60 + i) for i, n in enumerate(lens)]
        clouds[pos], keys5[pos] = cloud, key
        d5, t5 = modelnet.modelnet_draw(seed, keys5, 45.0, 0.5)
        batch = run(device, clouds, k, d5, t5, seed=seed, keys=keys5)[0]
        assert_same(batch[pos], alone, f"position {pos} of 5")
        assert all(g["status"] == 0 for g in batch)
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        again = run(device, [cloud], k, d1, t1, seed=seed, keys=[key])[0][0]
    assert_same(again, alone, "second stream")


# ---- 4. edges ------------------------------------------------------------------------------------------------------------
def _check(device, clouds, k, seed, keys, p=P07, draws=None, scale=0.0):
    """inline (or explicit) draws with zero jitter against the contract"""
    dirs, tf = modelnet.modelnet_draw(seed, keys, 45.0, 0.5)
    got, _ = run(device, clouds, k, dirs, tf, p=p, scale=scale, seed=seed, keys=keys, draws=draws)
    for b, c in enumerate(clouds):
        d = draws[b] if draws is not None else contract_draws(seed, keys[b], c.shape[0], k)
        assert_same(got[b], replica(c, k, dirs[b], tf[b], d, p=p, scale=scale), f"pair {b}")
    return got


@pytest.mark.parametrize("p", [(0.5, 0.5), (1.0, 1.0), (0.7, 1.0), (0.5, 0.3)])
def test_edges_half_space_and_no_crop(device, p):
    got = _check(device, [shape_cloud(500, 1), shape_cloud(33, 2)], 64, 5, [1, 2], p=p)
    if p == (1.0, 1.0):          # nothing cropped: every point overlaps, every selected-on-both-sides index corresponds
        assert got[0]["src_overlap"].all() and got[0]["tgt_overlap"].all()


def test_edges_duplicated_points_tie_at_the_threshold(device):
    """Every point four times: equal d around the threshold; the strict > drops all copies of the threshold point."""
    base = shape_cloud(50, 4)
    cloud = np.concatenate([base] * 4)[np.random.default_rng(0).permutation(200)]
    got = _check(device, [cloud], 64, 6, [3])[0]
    assert got["status"] == 0
    same = np.concatenate([base[:1]] * 40)                 # one point forty times: every d equal, nothing is > thr
    got = _check(device, [same, cloud], 16, 6, [4, 3])
    assert [g["status"] for g in got] == [2, 0] and got[0]["corr"].shape[1] == 0 and not got[0]["src_xyz"].any()


@pytest.mark.parametrize("n", [11, 21])
def test_edges_integral_h(device, n):
    """(n - 1) * 0.3: with q = 30.000001907348633 h sits just above 3 / 6: t is tiny, thr = a + (b - a) t"""
    _check(device, [shape_cloud(n, n)], 8, 7, [n])
    _check(device, [shape_cloud(n, n + 1)], 32, 7, [n + 100])            # and up-sampled


def test_edges_duplicate_resample_and_shuffle_keys_keep_the_stable_order(device):
    n, k = 96, 40
    cloud = shape_cloud(n, 8)
    d = contract_draws(1, 1, n, k)
    d["rkeys"] = np.stack([(np.arange(n, dtype=np.uint32)[::-1] // 8).astype(np.uint32), np.zeros(n, np.uint32)])
    d["skeys"] = np.stack([np.zeros(k, np.uint32), (np.arange(k, dtype=np.uint32)[::-1] // 4).astype(np.uint32)])
    got = _check(device, [cloud], k, 1, [1], draws=[d])[0]
    # all-equal shuffle keys: the source leaves in resample order; all-equal resample keys: the reference cloud is
    # resampled in ascending raw order
    want = replica(cloud, k, *[x[0] for x in modelnet.modelnet_draw(1, [1], 45.0, 0.5)], d, scale=0.0)
    assert np.array_equal(got["src_index"], want["src_resampled"])
    assert np.array_equal(np.sort(got["tgt_index"]), np.nonzero(want["crop_masks"][1])[0][:k])


def test_edges_the_longest_cloud(device):
    got = _check(device, [shape_cloud(8192, 9), shape_cloud(8191, 10)], 717, 8, [1, 2])
    assert all(g["status"] == 0 for g in got)
    _check(device, [shape_cloud(4097, 11)], 8192, 8, [3])                  # the largest k, up-sampled
    with pytest.raises(RuntimeError, match="8193"):
        run(device, [shape_cloud(8193, 12)], 717, *modelnet.modelnet_draw(8, [4], 45.0, 0.5), seed=8, keys=[4])


def test_edges_nan_in_one_pair_flags_that_pair_only_and_one_point_keeps_nothing(device):
    seed, keys, k = 3, [1, 2, 3, 4], 48
    clouds = [shape_cloud(100, 1), shape_cloud(80, 2), shape_cloud(1, 3), shape_cloud(120, 4)]
    dirs, tf = modelnet.modelnet_draw(seed, keys, 45.0, 0.5)
    clean, _ = run(device, clouds, k, dirs, tf, seed=seed, keys=keys)
    assert [g["status"] for g in clean] == [0, 0, 2, 0]
    assert not clean[2]["src_xyz"].any() and not clean[2]["tgt_index"].any() and clean[2]["corr"].shape[1] == 0
    bad = list(clouds)
    bad[1] = clouds[1].copy()
    bad[1][7, 1] = np.nan
    got, _ = run(device, bad, k, dirs, tf, seed=seed, keys=keys)
    assert [g["status"] for g in got] == [0, 1, 2, 0]
    for b in (0, 3):
        assert_same(got[b], clean[b], f"pair {b} beside a NaN pair")
    for g in got:
        assert g["src_index"].min() >= 0 and g["tgt_index"].min() >= 0
    assert got[1]["src_index"].max() < 80 and got[1]["corr"].shape[1] == 0
    inf_tf = tf.copy()
    inf_tf[3, 0, 3] = np.inf
    assert [g["status"] for g in run(device, clouds, k, dirs, inf_tf, seed=seed, keys=keys)[0]] == [0, 0, 2, 1]
    with pytest.raises(RuntimeError, match="without points"):
        modelnet.make_pairs([T(c).to(device) for c in bad], get_config("modelnet"), seed, keys)


# ---- 5. guard bands --------------------------------------------------------------------------------------------------------
def test_every_tensor_and_the_workspace_between_poisoned_guard_bands(device, monkeypatch):
    seed, keys, lens, k = 77, [5, 6, 7], [700, 2048, 333], 717           # pairs 0 and 2 up-sample
    clouds = [shape_cloud(n, 20 + b) for b, n in enumerate(lens)]
    dirs, tf, draws = device_draws(device, seed, keys, lens, k)
    for explicit in (False, True):
        kw = {"draws": draws} if explicit else {"seed": seed, "keys": keys}
        production = run(device, clouds, k, dirs, tf, **kw)[1]
        for flavour, poison in ((1, 0xFF), (2, 0x00)):
            arena, tensors = Arena(poison, GUARD), TensorArena(flavour, GUARD)
            with monkeypatch.context() as m:
                m.setattr(ops, "_workspace", arena)
                tensors.install(m)
                guarded = run(device, clouds, k, dirs, tf, put=tensors.put, **kw)[1]
            arena.verify()
            tensors.verify()
            assert arena.calls == 1 and tensors.calls > 10               # the ten outputs and the placed inputs
            cnt = production["corr_count"].tolist()
            for f in production:                                        # complete with exactly the queried size
                a, b = production[f], guarded[f]
                if f == "corr":                                         # columns past a pair's count are not written
                    cols = torch.cat([torch.arange(i * k, i * k + c) for i, c in enumerate(cnt)]).to(device)
                    a, b = a[:, cols], b[:, cols]
                assert torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8)), \
                    (f, explicit, hex(poison))


def test_the_call_is_refused_with_the_workspace_one_byte_short(device):
    L = _lib.lib()
    n, nb, k = 2048, 1, 717
    need = L.spr_modelnet_pairs_workspace_size(n, nb, k)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=device)
    dummy = torch.zeros(4 * nb * k * 3 + 64, dtype=torch.float64, device=device)   # never reached: the carve fails first
    p = lambda t: ops._ptr(t)
    args = lambda nbytes: (p(dummy), p(dummy), n, nb, n, 0.7, 0.7, 30.0, 30.0, k, 0.01, 0.05, p(dummy), p(dummy), 0, p(dummy),
                           None, None, None, None, p(dummy), p(dummy), p(dummy), p(dummy), p(dummy), p(dummy), p(dummy),
                           p(dummy), p(dummy), p(dummy), p(ws), nbytes, None)
    rc = L.spr_modelnet_pairs(*args(need - 1))
    assert rc != 0 and b"workspace too small" in L.spr_last_error()


# ---- 6. invariants ---------------------------------------------------------------------------------------------------------
def test_invariants_on_32_random_pairs(device):
    seed, nb, n, k = 2024, 32, 2048, 717
    keys = [500 + 3 * b for b in range(nb)]
    clouds = [shape_cloud(n, 100 + b) for b in range(nb)]
    dirs, tf = modelnet.modelnet_draw(seed, keys, 45.0, 0.5)
    got, _ = run(device, clouds, k, dirs, tf, scale=0.0, seed=seed, keys=keys)
    q = mr.percentile_q(0.7)
    for b in range(nb):
        g, x = got[b], clouds[b].astype(np.float64)
        assert g["status"] == 0
        c = mr._f32(mr.cloud_sum(x) / n)
        kept = [mr.crop(x, c, dirs[b, s], 0.7, q)[0] for s in range(2)]
        # every output point is a kept point of its own side; overlap iff kept on the other side as well
        assert kept[0][g["src_index"]].all() and kept[1][g["tgt_index"]].all()
        assert np.array_equal(g["src_overlap"].astype(bool), kept[1][g["src_index"]])
        assert np.array_equal(g["tgt_overlap"].astype(bool), kept[0][g["tgt_index"]])
        # no repeats when down-sampling; every correspondence joins the same raw index, in ascending raw order, and
        # they are all there: the raw indices present on both sides
        assert np.unique(g["src_index"]).size == k and np.unique(g["tgt_index"]).size == k
        cs, ct = g["src_index"][g["corr"][0]], g["tgt_index"][g["corr"][1]]
        assert np.array_equal(cs, ct) and np.all(np.diff(cs) > 0)
        assert np.array_equal(cs, np.intersect1d(g["src_index"], g["tgt_index"]))
        assert g["src_overlap"][g["corr"][0]].all() and g["tgt_overlap"][g["corr"][1]].all()
        # scale = 0: the reference cloud is the raw points, and the pose maps the source back onto them.  x' = R x + t
        # rounded once (<= U (|x|_1 + |t|_inf)), R^T R = I + E with |E_ij| <= 2 sqrt(3) U from the float32 rounding of R,
        # the pose's translation rounded once (<= sqrt(3) U |t|_inf): together below 8 U (|x|_1 + |t|_1)
        assert np.array_equal(g["tgt_xyz"], clouds[b][g["tgt_index"]])
        P, raw = g["pose"].astype(np.float64), x[g["src_index"]]
        back = g["src_xyz"].astype(np.float64) @ P[:, :3].T + P[:, 3]
        bound = 8 * U * (np.abs(raw).sum(axis=1, keepdims=True) + np.abs(tf[b][:, 3].astype(np.float64)).sum())
        assert np.all(np.abs(back - raw) <= bound), float((np.abs(back - raw) / bound).max())
        assert np.array_equal(_bits(g["pose"]), _bits(replica(clouds[b], k, dirs[b], tf[b],
                                                           contract_draws(seed, keys[b], n, k), scale=0.0)["pose"]))


# ---- 7. trainer --------------------------------------------------------------------------------------------------------------
def test_trainer_takes_a_step_on_generated_pairs(device):
    from superpoints_registration_amd import synthetic
    from superpoints_registration_amd.regtr import RegTR
    from superpoints_registration_amd.training import Trainer
    cfg = get_config("modelnet")
    shapes = torch.stack([T(np.concatenate([shape_cloud(2048, 70 + b), np.zeros((2048, 3), np.float32)], axis=1)) for b in range(2)])

    def step():
        model = RegTR(cfg)
        synthetic.fill_parameters(model, seed=0)
        model = model.to(device)
        batch = modelnet.make_pairs(shapes.to(device), cfg, 17, [3, 4])
        assert sorted(batch) == ["correspondences", "idx", "pose", "src_index", "src_overlap", "src_xyz", "tgt_index",
                                 "tgt_overlap", "tgt_xyz"]
        assert all(t.shape == (717, 3) for t in batch["src_xyz"] + batch["tgt_xyz"]) and batch["pose"].shape == (2, 3, 4)
        assert all(m.dtype == torch.bool for m in batch["src_overlap"]) and batch["correspondences"][0].dtype == torch.int64
        masks = [m.clone() for m in batch["src_overlap"]]
        losses = Trainer(cfg).setup(model).train_step(model, batch)
        assert all(torch.equal(a, b) for a, b in zip(masks, batch["src_overlap"]))     # the batch's own masks are used
        return losses
    a, b = step(), step()
    assert sorted(a) == sorted(b) and len(a) > 0
    for f in a:
        assert bool(torch.isfinite(a[f]).all()), (f, a[f])
        assert torch.equal(a[f], b[f]), f
