"""CPU: what the ICP tests rest on, and what the `icp` subpackage refuses on the host.

The replica (tests/icp_replica.py) is held to the geometry: on `snap` and `slide` it reaches the ground-truth pose.  The
stability condition: run a second time with every solved pose perturbed by a relative 2^-40, every iterated case gives
the same correspondences at every pass and the same number of passes -- so a disagreement of the kernel with the
replica on an integer output (tests/test_gpu_icp.py asks for equality) can only be the kernel's.  Measured here: snap
2 steps, count_0 = 510, fitness 510 / 729, final error to the ground truth 2.5e-9 (the float32 rounding of the target);
slide 6 steps, count_0 = 633; the perturbed runs end within 5.1e-12 of the plain ones (far, whose translation is 1e4:
4.6e-9).
The size query is swept like every other one (tests/test_workspace_sizes_host.py: monotone, never huge)."""
import numpy as np
import pytest
import torch

import icp_cases as C
from superpoints_registration_amd import _lib, get_config, icp, kitti
from test_workspace_sizes_host import HUGE, sweep_points


@pytest.mark.parametrize("name", C.ITERATED)
def test_integer_outputs_survive_a_relative_2_pow_minus_40(name):
    plain, moved = C.replica(name), C.replica(name, 2.0 ** -40)
    for b, (p, m) in enumerate(zip(plain, moved)):
        assert p["iterations"] == m["iterations"] and len(p["trace"]) == len(m["trace"]) == p["iterations"] + 1, (name, b)
        for k, (u, v) in enumerate(zip(p["trace"], m["trace"])):
            assert np.array_equal(u, v), f"{name} pair {b}: pass {k} changes under the perturbation"
        # a rotation moved by 2^-40 moves the translation by 2^-40 times the coordinates it turns (far: 1e4)
        scale = max([1.0] + [float(np.abs(x).max()) for x in (C.case(name)["src"][b], C.case(name)["tgt"][b]) if x.size])
        assert float(np.abs(p["pose64"] - m["pose64"]).max()) <= 1e-11 * scale, (name, b)


@pytest.mark.parametrize("name,steps,count0", [("snap", 2, 510), ("slide", 6, 633)])
def test_replica_reaches_the_ground_truth(name, steps, count0):
    r, = C.replica(name)
    assert r["iterations"] == steps and int((r["trace"][0] >= 0).sum()) == count0
    assert r["count"] == 510 and r["fitness"] == 510 / 729
    assert C.pose_error(r["pose64"]) <= 1e-8            # the target is the ground truth's image rounded to float32
    if name == "slide":                                 # wrong partners among the first correspondences
        first, last = r["trace"][0], r["trace"][-1]
        assert int(((first >= 0) & (first != last)).sum()) > 0


def test_replica_edge_rules():
    b = C.replica("boundary")
    assert b[0]["count"] == 0 and b[0]["corr"].tolist() == [-1]          # d2 == max_dist^2 is no match (strict)
    assert b[1]["corr"].tolist() == [2]
    assert b[2]["corr"].tolist() == [0, 3, 0]                            # ties and duplicates: the lowest index
    assert 0 < b[3]["count"] < len(b[3]["corr"]) and 0 < b[4]["count"] < len(b[4]["corr"])
    n = C.replica("nonfinite")
    assert [r["status"] for r in n] == [0, -1, 0]
    r = C.replica("ragged")
    assert [x["count"] for x in r] == [510, 1, 257, 0, 0]
    assert np.array_equal(r[3]["pose64"], C.case("ragged")["pose"][3])   # empty target: pose = init


def test_size_query_is_monotone_and_never_huge():
    fn = _lib.lib().spr_icp_pairs_workspace_size
    base, limits = [1000, 1000, 3], [1 << 25, 1 << 25, 32767]            # ns + nt <= 2^26, nb < 32768
    for i, limit in enumerate(limits):
        prev = None
        for v in sweep_points(limit):
            args = list(base)
            args[i] = v
            r = fn(*args)
            assert r < HUGE and (prev is None or r >= prev), (args, prev, r)
            prev = r
    assert fn(-1, 0, 1) == 0 and fn(0, 0, 0) > 0


def test_the_entry_point_refuses_bad_arguments_on_the_host():
    L = _lib.lib()
    args = [None, None, 0, None, None, 0, None, 1]
    outs = [None] * 8 + [None, 0, None]
    assert L.spr_icp_pairs(*args, 0.0, 0, 0.0, 0.0, *outs) != 0 and b"max_dist" in L.spr_last_error()
    assert L.spr_icp_pairs(*args, 0.1, -1, 0.0, 0.0, *outs) != 0 and b"max_iter" in L.spr_last_error()
    args[2] = 5
    args[7] = 0
    assert L.spr_icp_pairs(*args, 0.1, 1, 0.0, 0.0, *outs) != 0 and b"without pairs" in L.spr_last_error()


def test_host_layer_refuses_before_touching_a_device():
    x = torch.zeros((4, 3))
    eye = torch.eye(4)[None]
    with pytest.raises(ValueError, match="1 source clouds, 2 target clouds"):
        icp.icp_pairs([x], [x, x], eye, 0.1)
    with pytest.raises(ValueError, match="0 source clouds"):
        icp.icp_pairs([], [], eye[:0], 0.1)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_dist"):
            icp.icp_pairs([x], [x], eye, bad)
    with pytest.raises(ValueError, match="max_iter"):
        icp.icp_pairs([x], [x], eye, 0.1, max_iter=-1)
    with pytest.raises(ValueError, match="pose"):
        icp.icp_pairs([x], [x], torch.eye(4), 0.1)                      # [4, 4]: no batch dimension
    with pytest.raises(ValueError, match="pose"):
        icp.icp_pairs([x], [x], torch.eye(4)[None].repeat(2, 1, 1), 0.1)
    with pytest.raises(ValueError, match=r"expected an \[n, 3\] tensor"):
        icp.icp_pairs([torch.zeros((4, 4))], [x], eye, 0.1)
    with pytest.raises(ValueError, match="expected float32"):
        icp.icp_pairs([x.double()], [x], eye, 0.1)
    with pytest.raises(ValueError, match="expected the MI355X device"):
        icp.icp_pairs([x], [x], eye, 0.1)
    with pytest.raises(ValueError, match="expected the MI355X device"):
        icp.evaluate([x], [x], eye, 0.1)


def test_prepare_pairs_refine_pose_needs_a_pose():
    scan = torch.zeros((10, 4))
    with pytest.raises(ValueError, match="refine_pose=True needs the pose"):
        kitti.prepare_pairs([scan], [scan], get_config("kitti"), refine_pose=True)


def test_config_keys_are_off_by_default():
    for name in ("3dmatch", "kitti", "modelnet"):
        cfg = get_config(name)
        assert cfg.icp_refine is False and cfg.icp_distance is None and cfg.icp_max_iter == 30
    assert get_config("kitti", icp_refine=True, icp_distance=0.4, icp_max_iter=10).icp_distance == 0.4


def test_regtr_icp_refine_is_an_inference_option_of_pair_batches():
    from superpoints_registration_amd.regtr import RegTR
    model = RegTR(get_config("3dmatch", icp_refine=True, icp_distance=0.05))
    x = torch.zeros((8, 3))
    with pytest.raises(NotImplementedError, match="icp_refine"):
        model.train()({"src_xyz": [x], "tgt_xyz": [x]})
    with pytest.raises(NotImplementedError, match="icp_refine"):
        model.eval()({"clouds": [x, x], "pairs": [(0, 1)]})
