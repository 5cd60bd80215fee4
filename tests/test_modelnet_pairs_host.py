"""CPU: the ModelNet pair contract (include/spr.h "8f-7").  The numpy replica (tests/modelnet_replica.py) against the
reference's own transforms (golden modelnet_pairs.npz, written by scripts/gen_modelnet_pairs_golden.py), the library's
host-side draws against the replica, and the host-side argument checks.  No GPU."""
import numpy as np
import pytest

import modelnet_replica as mr
from conftest import load_golden
from superpoints_registration_amd import _lib, get_config, modelnet

U = 2.0 ** -24


def case(g, name):
    return {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + ".")}


def replica_of(g, c):
    p, q = float(g["p_keep"]), mr.percentile_q(float(g["p_keep"]))
    return mr.make_pair(c["xyz"], (p, p), (q, q), int(c["k"]), float(g["scale"]), float(g["clip"]), c["transform"],
                        c["dirs"], c["rkeys"], c["extra"], c["noise"], c["skeys"])


@pytest.fixture(scope="module")
def golden():
    g = load_golden("modelnet_pairs.npz")
    return g, {str(n): case(g, str(n)) for n in g["cases"]}


def test_fixture_holds_the_cases_and_the_contracts_own_draws(golden):
    g, cases = golden
    assert {(c["xyz"].shape[0], int(c["k"])) for c in cases.values()} == {(64, 32), (300, 717), (200, 32)}
    seed = int(g["seed"])
    for name, c in cases.items():
        key, n, k = int(c["key"]), c["xyz"].shape[0], int(c["k"])
        x = c["xyz"].astype(np.float64) * 4096.0
        assert np.array_equal(x, np.round(x)) and np.abs(c["xyz"]).max() < 1.0           # multiples of 2^-12 in (-1, 1)
        dirs, tf = mr.decide(seed, key, float(g["rot_mag"]), float(g["trans_mag"]))
        assert np.array_equal(dirs, c["dirs"]) and np.array_equal(tf, c["transform"])
        for s in range(2):
            assert np.array_equal(c["rkeys"][s], mr.resample_keys(seed, key, s, n))
            assert np.array_equal(c["extra"][s], mr.extra_words(seed, key, s, k))
            assert np.array_equal(c["skeys"][s], mr.shuffle_keys(seed, key, s, k))
            want = mr.noise64(seed, key, s, k)[0].astype(np.float32)
            assert (c["noise"][s] != want).sum() <= 1                                     # one planted value beyond the clip
    assert float(cases["opposed_200_32"]["dirs"][0] @ cases["opposed_200_32"]["dirs"][1]) < -0.97
    assert cases["opposed_200_32"]["ref_corr"].shape[1] <= 8
    assert np.abs(cases["down_64_32"]["noise"]).max() * float(g["scale"]) > float(g["clip"])


def test_replica_against_the_reference_transforms(golden):
    g, cases = golden
    for name, c in cases.items():
        r = replica_of(g, c)
        assert r["status"] == 0, name
        # every integer output is the reference's own
        assert np.array_equal(r["crop_masks"][0], c["ref_crop_src"]) and np.array_equal(r["crop_masks"][1], c["ref_crop_tgt"])
        assert np.array_equal(r["src_overlap"].astype(bool), c["ref_src_overlap"]), name
        assert np.array_equal(r["tgt_overlap"].astype(bool), c["ref_tgt_overlap"]), name
        assert np.array_equal(r["src_index"], c["ref_src_index"]) and np.array_equal(r["tgt_index"], c["ref_tgt_index"])
        assert np.array_equal(r["corr"], c["ref_corr"]), name
        # coordinates: the reference evaluates R x + t in float32 (and with its own numpy cos / sin / matmul): four
        # roundings of magnitude sum_j |R_ij| |x_j| + |t_i|, plus one float32 ulp of the result for the jitter add
        T = c["transform"].astype(np.float64)
        for nm, A, t in (("src", np.abs(T[:, :3]), np.abs(T[:, 3])), ("tgt", np.eye(3), np.zeros(3))):
            raw = np.abs(c["xyz"].astype(np.float64))[r[nm + "_index"]]
            got, ref = r[nm + "_xyz"].astype(np.float64), c["ref_" + nm].astype(np.float64)
            bound = 4 * U * (raw @ A.T + t) + np.spacing(np.abs(c["ref_" + nm])).astype(np.float64)
            err = np.abs(got - ref)
            print(name, nm, "max err / bound =", float((err / bound).max()))
            assert np.all(err <= bound), (name, nm)
        # pose = [R^T | -(R^T t)]: the same bound with x = a unit vector (rotation) and x = t (translation)
        P, Pr = r["pose"].astype(np.float64), c["ref_pose"].astype(np.float64)
        assert Pr.shape == (3, 4)
        bound = 4 * U * np.concatenate([np.abs(T[:, :3].T), (np.abs(T[:, :3].T) @ np.abs(T[:, 3]))[:, None]], axis=1)
        assert np.all(np.abs(P - Pr) <= bound), name
    up = replica_of(g, cases["up_300_717"])
    assert np.unique(up["src_index"]).size < 717                    # repeats: the up-sampling path


@pytest.mark.parametrize("n", [2, 11, 21, 64, 200, 2048])
def test_replica_threshold_is_numpys_linear_percentile(n):
    """integral h at n = 11, 21 (h = 3, 6 exactly for q = 30) and the float32-born q of p_keep = 0.7"""
    rng = np.random.default_rng(n)
    d = rng.standard_normal(n)
    d[n // 2] = d[0]                                                 # a tie
    for q in (30.0, mr.percentile_q(0.7), mr.percentile_q(0.3), mr.percentile_q(0.9)):
        assert mr.crop_threshold(d, q) == np.percentile(d, q), (n, q)
    assert mr.percentile_q(0.7) == modelnet.percentile_q(0.7) == 30.000001907348633


def test_cloud_sum_order_is_exact_on_quantised_points_and_fixed_otherwise():
    rng = np.random.default_rng(0)
    q = np.round(rng.uniform(-1, 1, (3000, 3)) * 4096.0) / 4096.0
    assert np.array_equal(mr.cloud_sum(q), np.array([float(sum(q[:, d].tolist())) for d in range(3)]))
    x = rng.standard_normal((2500, 3)).astype(np.float32)
    assert np.allclose(mr.cloud_sum(x), x.astype(np.float64).sum(axis=0), rtol=1e-12, atol=1e-12)


def test_host_draws_equal_the_replica_bit_for_bit():
    seed, keys = 0xC0FFEE1234, [0, 5, 2 ** 33 + 1, 2 ** 62 + 7]
    for rot, trans in ((45.0, 0.5), (180.0, 1.0), (0.0, 0.0)):
        dirs, tf = modelnet.modelnet_draw(seed, keys, rot, trans)
        assert dirs.shape == (4, 2, 3) and dirs.dtype == np.float64 and tf.shape == (4, 3, 4) and tf.dtype == np.float32
        for b, key in enumerate(keys):
            d, t = mr.decide(seed, key, rot, trans)
            assert np.array_equal(dirs[b].view(np.uint64), d.view(np.uint64)), (rot, key)
            assert np.array_equal(tf[b].view(np.uint32), t.view(np.uint32)), (rot, key)
            R = tf[b, :, :3].astype(np.float64)
            assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(R) - 1.0) <= 1e-6
            assert np.abs(np.linalg.norm(dirs[b], axis=1) - 1.0).max() <= 1e-15
            assert np.all(np.abs(tf[b, :, 3]) <= trans)
    a = modelnet.modelnet_draw(seed, [5], 45.0, 0.5)
    b = modelnet.modelnet_draw(seed + 1, [5], 45.0, 0.5)
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0][0, 0], a[0][0, 1])               # the two sides draw their own directions
    with pytest.raises(RuntimeError, match="2\\^63"):
        modelnet.modelnet_draw(seed, [2 ** 63], 45.0, 0.5)


def _pairs_rc(max_len=2048, p=(0.7, 0.7), k=717, nb=1, n_total=2048):
    """spr_modelnet_pairs with null tensors: only the host-side checks in front of the first HIP call can answer."""
    L = _lib.lib()
    q = [modelnet.percentile_q(x) if 0.0 < x <= 1.0 else 30.0 for x in p]
    rc = L.spr_modelnet_pairs(None, None, n_total, nb, max_len, p[0], p[1], q[0], q[1], k, 0.01, 0.05, None, None, 0,
                              None, None, None, None, None, None, None, None, None, None, None, None, None, None, None,
                              None, 0, None)
    return rc, L.spr_last_error()


def test_host_side_argument_validation_needs_no_gpu():
    rc, msg = _pairs_rc(max_len=8193)
    assert rc != 0 and b"8193" in msg and b"8192" in msg
    for k in (0, -1, 8193):
        rc, msg = _pairs_rc(k=k)
        assert rc != 0 and b"k must be" in msg, k
    for p in ((0.0, 0.7), (0.7, 0.0), (-0.1, 0.7), (0.7, 1.5), (float("nan"), 0.7)):
        rc, msg = _pairs_rc(p=p)
        assert rc != 0 and b"p_keep" in msg, p
    rc, msg = _pairs_rc()                                            # legal sizes: the first complaint is a null pointer
    assert rc != 0 and b"null" in msg
    assert _pairs_rc(nb=0, n_total=0)[0] == 0                        # nothing to do


def test_workspace_query_is_monotone_and_rejects_negative_sizes():
    f = _lib.lib().spr_modelnet_pairs_workspace_size
    assert f(-1, 1, 1) == 0 and f(1, -1, 1) == 0 and f(1, 1, -1) == 0
    base = (8192, 4, 717)
    for i, limit in enumerate((1 << 26, 1 << 13, 8192)):
        prev = 0
        for v in (0, 1, 2, 255, 256, 257, limit - 1, limit):
            args = list(base)
            args[i] = v
            r = f(*args)
            assert prev <= r < (1 << 40), (i, v, r)
            prev = r
    assert f(4 * 2048, 4, 717) >= 2 * 4 * 2048 + 16 * 4 * 717


def test_config_and_the_unbuilt_noise_types():
    cfg = get_config("modelnet")
    assert (list(cfg.partial), cfg.num_points, cfg.noise_type, cfg.rot_mag, cfg.trans_mag) == ([0.7, 0.7], 1024, "crop", 45.0, 0.5)
    assert modelnet.output_size(cfg) == 717
    for nt in ("clean", "jitter"):
        with pytest.raises(NotImplementedError, match=nt):
            modelnet.make_pairs([], get_config("modelnet", noise_type=nt), 0, [])
    with pytest.raises(NotImplementedError, match="partial"):
        modelnet.output_size(get_config("modelnet", partial=[0.7]))
