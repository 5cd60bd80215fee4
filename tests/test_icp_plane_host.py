"""CPU: what the point-to-plane ICP tests rest on, and what the `icp_plane` subpackage and its entry point refuse on
the host.

The replica (tests/icp_plane_replica.py) is held to the geometry: on the corner it reaches the ground-truth pose from
both starts -- to 1.4e-8, in 2 steps (snap) and 4 (slide); the point-to-point replica needs 16 on the same clouds and
stops 0.05 away, because the two independent samples let the source slide along the faces.  The stability condition:
run a second time with every solved pose perturbed by a relative 2^-40, every case gives the same correspondences at
every pass and the same number of passes -- so a disagreement of the kernel with the replica on an integer output
(tests/test_gpu_icp_plane.py asks for equality) can only be the kernel's.  How far pose64 and inlier_rmse move under
that perturbation is the replica's own spread, icp_plane_cases.sensitivity: 0.9e-12 .. 3.4e-12 and <= 2.2e-13 for the
cases at the origin, 9.1e-9 and 5.3e-10 for `far`; the GPU tolerances are 16 x these (icp_plane_cases.bounds)."""
import numpy as np
import pytest
import torch

import icp_cases as C0
import icp_plane_cases as C
import icp_plane_replica as P
import icp_replica as R
from superpoints_registration_amd import _lib, get_config, icp_plane, kitti
from test_workspace_sizes_host import HUGE, sweep_points


@pytest.mark.parametrize("name", C.ITERATED)
def test_integer_outputs_survive_a_relative_2_pow_minus_40(name):
    plain, moved = C.replica(name), C.replica(name, 2.0 ** -40)
    for b, (p, m) in enumerate(zip(plain, moved)):
        assert p["status"] == m["status"] and p["iterations"] == m["iterations"] <= 30, (name, b)
        assert len(p["trace"]) == len(m["trace"]) == (p["iterations"] + 1 if p["status"] == 0 else 0), (name, b)
        assert p["refused"] == m["refused"], (name, b)
        for k, (u, v) in enumerate(zip(p["trace"], m["trace"])):
            assert np.array_equal(u, v), f"{name} pair {b}: pass {k} changes under the perturbation"


@pytest.mark.parametrize("name", C.CASES)
def test_the_replicas_own_spread_is_small_and_gives_the_gpu_bounds(name):
    pose, rmse = C.sensitivity(name)
    print(f"icp_plane {name}: replica sensitivity pose64 {pose:.3e}, inlier_rmse {rmse:.3e}; bounds {C.bounds(name)}")
    # a pose moved by a relative 2^-40 moves by 2^-40 times its entries; the steps after it may amplify that a little
    scale = max(float(np.abs(x).max()) for x in C.case(name)["tgt"] if x.size)
    assert 0.0 < pose <= 64 * 2.0 ** -40 * max(scale, 1.0) and rmse <= 64 * 2.0 ** -40 * max(scale, 1.0), name
    assert C.bounds(name)[0] == (16 * pose if name == "far" else min(16 * pose, 1e-9))


@pytest.mark.parametrize("name,steps", [("corner_snap", 2), ("corner_slide", 4)])
def test_replica_reaches_the_ground_truth_on_the_corner(name, steps):
    r, = C.replica(name)
    c = C.case(name)
    assert r["iterations"] == steps and r["count"] == 257 and r["fitness"] == 1.0 and not any(r["refused"])
    # the target is the ground truth's image rounded to float32 (half an ulp of coordinates below 4: 1.2e-7), and the
    # least-squares fit over 257 points averages that down
    assert C.pose_error(r["pose64"]) <= 1e-7
    # the RMSE is the POINT distance: two independent samples never coincide
    assert r["inlier_rmse"] > 0.05
    # the same clouds and start by point-to-point: more passes, and the source slides along the faces
    p2p = R.icp(c["src"][0], c["tgt"][0], c["pose"][0], c["max_dist"], 30)
    assert p2p["iterations"] > 2 * steps and C.pose_error(p2p["pose64"]) > 1e-3


def test_replica_edge_rules_on_the_plane():
    c, (r,) = C.case("plane"), C.replica("plane")
    assert np.array_equal(c["nrm"][0], np.tile(np.array([[0, 0, 1]], dtype=np.float32), (300, 1)))
    assert r["refused"] == [True] and r["iterations"] == 1 and r["count"] == 257
    assert r["pose64"].tobytes() == np.ascontiguousarray(c["pose"][0]).tobytes()      # U = I: bit-equal to pose_init
    assert len(r["resid"]) == 1 and float(np.abs(r["resid"][0]).min()) > 0.04          # not for want of a residual
    # the pivot that stops it is an exact zero, after two that pass
    a = R.transform(c["pose"][0], c["src"][0])
    hit = r["trace"][0] >= 0
    b, n = c["tgt"][0].astype(np.float64)[r["trace"][0][hit]], c["nrm"][0].astype(np.float64)[r["trace"][0][hit]]
    A, g, _ = P.normal_equations(a[hit], b, n, c["tgt"][0].astype(np.float64).min(0), "l2", None)
    assert not A[2].any() and not A[3].any() and not A[4].any() and A[0, 0] > 0 and A[1, 1] > 0 and A[5, 5] == 257.0
    assert P.ldlt_solve(A, g) is None


def test_replica_other_edge_rules():
    r = C.replica("ragged")
    assert [x["count"] for x in r] == [257, 1, 257, 0, 0]
    assert r[1]["refused"] == [True]                                      # one correspondence: rank one
    for b in (1, 3, 4):
        assert r[b]["iterations"] == 1
        assert r[b]["pose64"].tobytes() == np.ascontiguousarray(C.case("ragged")["pose"][b]).tobytes()
    assert [x["status"] for x in C.replica("nonfinite")] == [0, -1, 0]
    z, plain = C.replica("zero_normals")[0], C.replica("corner_snap")[0]
    assert z["count"] == plain["count"] == 257 and np.array_equal(z["trace"][0], plain["trace"][0])   # they still count
    assert C.pose_error(z["pose64"]) <= 1e-7 and not np.array_equal(z["pose64"], plain["pose64"])


@pytest.mark.parametrize("name", C.ROBUST[1:])
def test_robust_cases_take_both_branches_of_the_weight(name):
    r, = C.replica(name)
    k = C.case(name)["kernel_k"]
    ar = np.abs(np.concatenate(r["resid"]))
    assert int((ar <= k).sum()) > 0 and int((ar > k).sum()) > 0
    w = P.weights(np.array([0.0, 0.5 * k, k, 2.0 * k]), C.case(name)["kernel"], k)
    assert w.tolist() == ([1.0, 1.0, 1.0, 0.5] if name == "robust_huber" else [1.0, 0.5625, 0.0, 0.0])


def test_tukey_rejects_the_outliers_that_bias_l2():
    errs = {n: C.pose_error(C.replica(n)[0]["pose64"]) for n in C.ROBUST}
    assert errs["robust_tukey"] <= 1e-7 < 1e-3 < errs["robust_l2"], errs


def test_negated_normals_change_nothing_in_the_replica():
    c = C.case("corner_slide")
    a, = C.replica("corner_slide")
    b = P.icp(c["src"][0], c["tgt"][0], -c["nrm"][0], c["pose"][0], c["max_dist"], c["max_iter"])
    assert a["pose64"].tobytes() == b["pose64"].tobytes() and a["iterations"] == b["iterations"]


def test_size_query_is_monotone_and_never_huge():
    fn, p2p = _lib.lib().spr_icp_plane_pairs_workspace_size, _lib.lib().spr_icp_pairs_workspace_size
    base, limits = [1000, 1000, 3], [1 << 25, 1 << 25, 32767]            # ns + nt <= 2^26, nb < 32768
    for i, limit in enumerate(limits):
        prev = None
        for v in sweep_points(limit):
            args = list(base)
            args[i] = v
            r = fn(*args)
            assert r < HUGE and (prev is None or r >= prev), (args, prev, r)
            assert r >= p2p(*args)                                        # 29 partials per block, not 17
            prev = r
    assert fn(-1, 0, 1) == 0 and fn(0, 0, 0) > 0


def test_the_entry_point_refuses_bad_arguments_on_the_host():
    L = _lib.lib()
    args = [None, None, 0, None, None, None, 0, None, 1]
    outs = [None] * 8 + [None, 0, None]
    call = lambda dist, it, kernel, k: L.spr_icp_plane_pairs(*args, dist, it, 0.0, 0.0, kernel, k, *outs)
    assert call(0.0, 0, 0, 0.0) != 0 and b"max_dist" in L.spr_last_error()
    assert call(0.1, -1, 0, 0.0) != 0 and b"max_iter" in L.spr_last_error()
    for kernel in (-1, 3):
        assert call(0.1, 1, kernel, 1.0) != 0 and b"kernel must be" in L.spr_last_error()
    for kernel in (1, 2):
        for k in (0.0, -1.0, float("nan")):
            assert call(0.1, 1, kernel, k) != 0 and b"kernel_k" in L.spr_last_error()
    assert call(0.1, 1, 0, float("nan")) != 0 and b"kernel_k" not in L.spr_last_error()   # L2 never reads it
    args[2] = 5
    args[8] = 0
    assert call(0.1, 1, 0, 0.0) != 0 and b"without pairs" in L.spr_last_error()


def test_host_layer_refuses_before_touching_a_device():
    x = torch.zeros((4, 3))
    eye = torch.eye(4)[None]
    with pytest.raises(ValueError, match="1 source clouds, 2 target clouds"):
        icp_plane.icp_pairs([x], [x, x], [x], eye, 0.1)
    with pytest.raises(ValueError, match="0 source clouds"):
        icp_plane.icp_pairs([], [], [], eye[:0], 0.1)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_dist"):
            icp_plane.icp_pairs([x], [x], [x], eye, bad)
    with pytest.raises(ValueError, match="max_iter"):
        icp_plane.icp_pairs([x], [x], [x], eye, 0.1, max_iter=-1)
    with pytest.raises(ValueError, match="pose"):
        icp_plane.icp_pairs([x], [x], [x], torch.eye(4), 0.1)
    with pytest.raises(ValueError, match="kernel 'cauchy'"):
        icp_plane.icp_pairs([x], [x], [x], eye, 0.1, kernel="cauchy")
    for kernel in ("huber", "tukey"):
        for k in (None, 0.0, -0.5, float("nan")):
            with pytest.raises(ValueError, match="kernel_k"):
                icp_plane.icp_pairs([x], [x], [x], eye, 0.1, kernel=kernel, kernel_k=k)
            with pytest.raises(ValueError, match="kernel_k"):                        # before the normals are estimated
                icp_plane.icp_pairs([x], [x], None, eye, 0.1, kernel=kernel, kernel_k=k, normals_radius=0.3)
    with pytest.raises(ValueError, match="give tgt_normals, or normals_radius"):
        icp_plane.icp_pairs([x], [x], None, eye, 0.1)
    with pytest.raises(ValueError, match="not both"):
        icp_plane.icp_pairs([x], [x], [x], eye, 0.1, normals_radius=0.3)
    with pytest.raises(ValueError, match="normals_radius must be > 0"):
        icp_plane.icp_pairs([x], [x], None, eye, 0.1, normals_radius=0.0)
    with pytest.raises(ValueError, match="tgt_normals is None"):
        icp_plane.icp_pairs_raw([x], [x], None, eye, 0.1)
    with pytest.raises(ValueError, match="2 normal tensors for 1 target clouds"):
        icp_plane.icp_pairs([x], [x], [x, x], eye, 0.1)
    with pytest.raises(ValueError, match=r"tgt_normals\[0\] has 5 rows, its cloud 4"):
        icp_plane.icp_pairs([x], [x], [torch.zeros((5, 3))], eye, 0.1)
    with pytest.raises(ValueError, match=r"tgt_normals\[0\] is .*expected an \[n, 3\] tensor"):
        icp_plane.icp_pairs([x], [x], [torch.zeros((4, 4))], eye, 0.1)
    with pytest.raises(ValueError, match=r"tgt_normals\[0\] is torch.float64, expected float32"):
        icp_plane.icp_pairs([x], [x], [x.double()], eye, 0.1)
    with pytest.raises(ValueError, match="expected the MI355X device"):
        icp_plane.icp_pairs([x], [x], [x], eye, 0.1)
    with pytest.raises(ValueError, match="expected the MI355X device"):
        icp_plane.icp_pairs([x], [x], None, eye, 0.1, normals_radius=0.3)


def test_prepare_pairs_point_to_plane_needs_a_radius_and_a_known_method():
    scan = torch.zeros((10, 4))
    pose = torch.eye(4)[None]
    with pytest.raises(ValueError, match="needs icp_normals_radius"):
        kitti.prepare_pairs([scan], [scan], get_config("kitti"), pose=pose, refine_pose=True, icp_method="point_to_plane")
    with pytest.raises(ValueError, match="icp_method 'plane'"):
        kitti.prepare_pairs([scan], [scan], get_config("kitti"), pose=pose, refine_pose=True, icp_method="plane")


def test_config_keys_are_off_by_default():
    for name in ("3dmatch", "kitti", "modelnet"):
        cfg = get_config(name)
        assert cfg.icp_refine is False and cfg.icp_method == "point_to_point"
        assert cfg.icp_normals_radius is None and cfg.icp_kernel == "l2" and cfg.icp_kernel_k is None
    cfg = get_config("kitti", icp_refine=True, icp_method="point_to_plane", icp_normals_radius=0.5, icp_kernel="huber",
                     icp_kernel_k=0.1)
    assert (cfg.icp_method, cfg.icp_normals_radius, cfg.icp_kernel, cfg.icp_kernel_k) == ("point_to_plane", 0.5, "huber", 0.1)


def test_the_header_and_the_binding_agree():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spr.h")).read()
    m = re.search(r"int spr_icp_plane_pairs\((.*?)\);", hdr, re.S)
    assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES["spr_icp_plane_pairs"][1]) == 26
    assert "Point-to-plane ICP for all pairs" in hdr
