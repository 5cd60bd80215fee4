"""CPU: the normals subpackage's argument refusals, the refusals of its two C-ABI entry points (made on the host before
any HIP call) and the host restatements of tests/normals_cases.py on inputs with a known answer.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import normals_cases as NC
from superpoints_registration_amd import _lib, augment, get_config, modelnet, normals

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "spr.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("spr_estimate_normals", "spr_feats_gather_rotate"):
        assert re.search(rf"\b{name}\s*\(", hdr) and hasattr(raw, name) and name in _lib.SIGNATURES
        assert callable(getattr(_lib.lib(), name))
    # the header's parameter lists and the ctypes signatures have the same lengths
    for name in ("spr_estimate_normals", "spr_feats_gather_rotate"):
        params = re.search(rf"\b{name}\s*\(([^)]*)\)", hdr).group(1).split(",")
        assert len(params) == len(_lib.SIGNATURES[name][1]), name


def test_top_level_modules_do_not_name_the_entry_points():
    pkg = os.path.dirname(_lib.__file__)
    for n in sorted(os.listdir(pkg)):
        if n.endswith(".py") and n != "_lib.py":
            text = open(os.path.join(pkg, n)).read()
            assert "spr_estimate_normals" not in text and "spr_feats_gather_rotate" not in text, n


def test_the_library_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    cols = (ctypes.c_int * 5)(1, 4, 7, 10, 13)
    assert L.spr_feats_gather_rotate(None, 10, 16, None, 5, None, 1, None, cols, 5, None, None) == 2
    assert b"at most 4" in L.spr_last_error()
    cols = (ctypes.c_int * 4)(2, 0, 0, 0)
    assert L.spr_feats_gather_rotate(None, 10, 4, None, 5, None, 1, None, cols, 1, None, None) == 2
    assert b"runs past the 4 columns" in L.spr_last_error()
    cols = (ctypes.c_int * 4)(-1, 0, 0, 0)
    assert L.spr_feats_gather_rotate(None, 10, 4, None, 5, None, 1, None, cols, 1, None, None) == 2
    cols = (ctypes.c_int * 4)(0, 2, 0, 0)
    assert L.spr_feats_gather_rotate(None, 10, 8, None, 5, None, 1, None, cols, 2, None, None) == 2
    assert b"overlap" in L.spr_last_error()
    assert L.spr_feats_gather_rotate(None, 10, 0, None, 5, None, 1, None, None, 0, None, None) == 2
    assert L.spr_feats_gather_rotate(None, 10, 4, None, 5, None, 1, None, None, 0, None, None) == 2      # null rows / out
    assert b"null" in L.spr_last_error()
    assert L.spr_estimate_normals(None, None, 10, 1, None, 3, 4, None, None, None, None) == 2            # stride < kmax
    assert b"nbr_stride" in L.spr_last_error()
    assert L.spr_estimate_normals(None, None, -1, 1, None, 4, 4, None, None, None, None) == 2
    assert L.spr_estimate_normals(None, None, 10, 1, None, 4, 4, None, None, None, None) == 2            # null pointers
    # nothing to do is legal and touches no pointer
    assert L.spr_estimate_normals(None, None, 0, 0, None, 0, 0, None, None, None, None) == 0
    cols = (ctypes.c_int * 4)(1, 0, 0, 0)
    assert L.spr_feats_gather_rotate(None, 10, 4, None, 0, None, 0, None, cols, 1, None, None) == 0


def test_direction_cols_are_validated():
    assert normals.check_direction_cols((1,), 4) == [1] and normals.check_direction_cols((), 1) == []
    assert normals.check_direction_cols((5, 0), 8) == [5, 0]
    with pytest.raises(ValueError, match="runs past the 4 feature columns"):
        normals.check_direction_cols((2,), 4)
    with pytest.raises(ValueError, match="runs past"):
        normals.check_direction_cols((-1,), 4)
    with pytest.raises(ValueError, match="at most 4"):
        normals.check_direction_cols((0, 3, 6, 9, 12), 16)
    with pytest.raises(ValueError, match="overlapping"):
        normals.check_direction_cols((0, 2), 8)


def test_the_python_layer_refuses_wrong_widths_and_counts():
    with pytest.raises(ValueError, match=r"expected \[N, 3\]"):
        normals.estimate(torch.zeros(10, 2), [10], 0.1)
    with pytest.raises(ValueError, match=r"expected \[N, 3\]"):
        normals.from_neighbors(torch.zeros(10, 4), torch.zeros((10, 5), dtype=torch.int32))
    with pytest.raises(ValueError, match="nbr"):
        normals.from_neighbors(torch.zeros(10, 3), torch.zeros((9, 5), dtype=torch.int32))
    with pytest.raises(ValueError, match="3 viewpoints for 2 clouds"):
        normals.estimate(torch.zeros(10, 3), [4, 6], 0.1, viewpoint=np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError, match="needs cu"):
        normals.from_neighbors(torch.zeros(10, 3), torch.zeros((10, 5), dtype=torch.int32), viewpoint=np.zeros((1, 3)))
    with pytest.raises(ValueError, match="runs past"):
        normals.gather_rotate(torch.zeros(10, 4), torch.zeros(3, dtype=torch.int64), torch.tensor([0, 3]), np.eye(3)[None], (2,))
    with pytest.raises(ValueError, match=r"expected \[n, C\]"):
        normals.gather_rotate(torch.zeros(10), torch.zeros(3, dtype=torch.int64), torch.tensor([0, 3]), np.eye(3)[None])
    with pytest.raises(RuntimeError, match="no CPU fallback"):            # valid arguments, but not on the device
        normals.estimate(torch.zeros(10, 3), [10], 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        normals.gather_rotate(torch.zeros(10, 4), torch.zeros(3, dtype=torch.int64), torch.tensor([0, 3]), np.eye(3)[None], (1,))


def test_the_wiring_refuses_before_the_device():
    cfg = get_config("modelnet")
    with pytest.raises(ValueError, match="normals=True needs"):
        modelnet.make_pairs(torch.zeros(2, 64, 3), cfg, 0, [1, 2], normals=True)
    with pytest.raises(ValueError, match="normals=True needs"):
        modelnet.make_pairs([torch.zeros(64, 6), torch.zeros(64, 3)], cfg, 0, [1, 2], normals=True)
    cfg = get_config("3dmatch")
    clouds = [torch.zeros(5, 3)]
    feats = [torch.zeros(5, 4)]
    batch = {"src_xyz": clouds, "tgt_xyz": clouds, "pose": torch.zeros(1, 3, 4), "src_point_feats": feats, "tgt_point_feats": feats}
    with pytest.raises(ValueError, match="runs past the 4 feature columns"):
        augment.augment_batch(batch, cfg, 0, [1], direction_cols=(2,))
    with pytest.raises(ValueError, match="at most 4"):
        augment.augment_batch(batch, cfg, 0, [1], direction_cols=(0, 0, 0, 0, 0))
    with pytest.raises(ValueError, match="direction_cols without"):
        augment.augment_batch({"src_xyz": clouds, "tgt_xyz": clouds, "pose": torch.zeros(1, 3, 4)}, cfg, 0, [1], direction_cols=(1,))
    assert augment.TrainAugmentation(cfg, direction_cols=[1]).direction_cols == (1,)


# ---- the restatements on inputs with a known answer --------------------------------------------------------------------
def test_reference_on_a_plane_a_line_and_too_few_points():
    rng = np.random.default_rng(0)
    plane = np.concatenate([rng.uniform(-1, 1, (30, 2)), np.zeros((30, 1))], 1).astype(np.float32)       # z = 0
    pts = np.concatenate([plane, [[5, 5, 5], [5.5, 5, 5]]]).astype(np.float32)
    nbr = np.full((32, 30), 32, np.int64)
    nbr[:30] = np.arange(30)
    nbr[30, :2] = nbr[31, :2] = [30, 31]
    ref = NC.reference(pts, nbr)
    assert list(ref['m'][[0, 30, 31]]) == [30, 2, 2]
    assert np.allclose(np.abs(ref['vec'][:30]), [0, 0, 1], atol=1e-12) and np.all(ref['curv'][:30] < 1e-12)
    assert not ref['vec'][30:].any() and not ref['curv'][30:].any()
    s, tie = NC.sign_rule(ref['vec'][:30], pts[:30], None)
    assert np.all((ref['vec'][:30] * s[:, None])[:, 2] > 0) and not tie.any()
    view = NC.per_point_view(np.array([[0, 0, -4]], np.float32), [30], 30)
    s, tie = NC.sign_rule(ref['vec'][:30], pts[:30], view)
    assert np.all((ref['vec'][:30] * s[:, None])[:, 2] < 0) and not tie.any()
    # a perfect result passes the checks; a tilted one does not
    good = np.zeros((32, 3), np.float32)
    good[:30, 2] = 1
    NC.check(pts, nbr, [32], None, good, np.zeros(32, np.float32), "plane", cap_gap_share=False)
    bad = good.copy()
    bad[0] = [0.01, 0, 1]
    bad[0] /= np.linalg.norm(bad[0])
    with pytest.raises(AssertionError):
        NC.check(pts, nbr, [32], None, bad, None, "tilted", cap_gap_share=False)
    flipped = good.copy()
    flipped[:30, 2] = -1
    with pytest.raises(AssertionError, match="sign"):
        NC.check(pts, nbr, [32], None, flipped, None, "flipped", cap_gap_share=False)


def test_gather_rotate_restatement():
    feats = np.arange(20, dtype=np.float32).reshape(5, 4)
    quarter = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)             # x -> y
    out = NC.gather_rotate(feats, np.array([4, 0, 0]), [1, 2], np.stack([quarter, np.eye(3, dtype=np.float32)]), (1,))
    assert out.tolist() == [[16, -18, 17, 19], [0, 1, 2, 3], [0, 1, 2, 3]]
