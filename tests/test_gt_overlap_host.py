"""CPU: the ground-truth overlap operator's host side -- the C-ABI entry validates its arguments before any
HIP call, the tensor wrapper refuses CPU tensors, the configs carry the reference's overlap radii and
overlap.compute_overlap keeps the reference's signature (utils/pointcloud.py:8)."""
import inspect

import pytest
import torch

from superpoints_registration_amd import _lib, get_config, ops, overlap


def _call(L, ns, nt, nb, radius):
    return L.spr_gt_overlap(None, None, ns, None, None, nt, None, nb, radius, None, None, None, None, None, None,
                            None, 0, None)


def test_spr_gt_overlap_argument_validation():
    L = _lib.lib()
    assert L.spr_gt_overlap_workspace_bytes(1000, 900, 2) > 0
    rc = _call(L, 0, 0, 1, 0.0)
    assert rc != 0 and b"gt_overlap" in L.spr_last_error() and b"radius" in L.spr_last_error()
    rc = _call(L, 0, 0, 1, -0.1)
    assert rc != 0 and b"gt_overlap" in L.spr_last_error()
    rc = _call(L, 0, 0, -1, 0.1)
    assert rc != 0 and b"gt_overlap" in L.spr_last_error()
    # null pointers with non-zero sizes
    rc = _call(L, 10, 10, 1, 0.1)
    assert rc != 0 and b"gt_overlap" in L.spr_last_error()
    # no pairs, no points: nothing to do, no HIP call
    assert _call(L, 0, 0, 0, 0.1) == 0


def test_ops_gt_overlap_refuses_cpu_tensors():
    cu = torch.tensor([0, 4], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gt_overlap(torch.zeros(4, 3), cu, torch.zeros(4, 3), cu, torch.eye(4)[None, :3], 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        overlap.compute_overlap(torch.zeros(4, 3), torch.zeros(4, 3), 0.1)


@pytest.mark.parametrize("tag,radius", [("3dmatch", 0.0375), ("kitti", 0.3), ("modelnet", 0.04)])
def test_config_overlap_radius(tag, radius):
    assert get_config(tag).overlap_radius == radius


def test_compute_overlap_signature():
    assert list(inspect.signature(overlap.compute_overlap).parameters) == ["src", "tgt", "search_voxel_size"]
    assert list(inspect.signature(overlap.label_batch).parameters) == ["batch", "radius"]
