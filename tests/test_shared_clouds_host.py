"""CPU: the host side of training over shared clouds -- the two C-ABI entry points are declared, exported and bound; the
pair layout (segment -> cloud, the use list in CSR form, the per-level cu_out) against a brute-force restatement; every
refusal of RegTR.forward and of the Trainer on a batch of clouds and pairs happens on the host, before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from superpoints_registration_amd import _lib, get_config, shared_clouds
from superpoints_registration_amd.regtr import RegTR
from superpoints_registration_amd.training import Trainer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tests/test_gpu_encode_once.py::LENS / GATHER_PAIRS (that module is all-GPU; the lists are restated, and compared when a
# GPU run imports both: tests/test_gpu_shared_clouds.py)
LENS = [1, 63, 64, 65, 300]
# (0, 0): a cloud paired with itself; cloud 2 is never used; cloud 4 is used three times
GATHER_PAIRS = {1: [(2, 4)], 7: [(0, 0), (4, 1), (3, 4), (1, 3), (4, 0), (0, 3), (1, 1)]}
LEVELS = [[4 * n + 3 for n in LENS], [2 * n for n in LENS], LENS]          # a three-level pyramid's host lengths


def test_entry_points_are_declared_exported_and_bound():
    text = open(os.path.join(REPO, "include", "spr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in (("spr_pair_gather_bwd", 12), ("spr_overlap_pool_pairs", 16)):
        assert re.search(rf"\bint\s+{name}\s*\(", text)
        assert hasattr(raw, name) and name in _lib.SIGNATURES
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert not any(k.startswith(("spr_pair_gather_bwd_", "spr_overlap_pool_pairs_")) for k in _lib.SIGNATURES)  # no workspace
    # bad arguments are rejected on the host before any HIP call
    L = _lib.lib()
    assert L.spr_version() == 6
    rc = L.spr_pair_gather_bwd(None, 10, 256, None, 2, None, None, 1, None, 10, None, None)
    assert rc != 0 and b"pair_gather_bwd" in L.spr_last_error()
    rc = L.spr_overlap_pool_pairs(None, 10, None, 7, 7, 5, None, None, 2, None, 1, None, None, 5, None, None)
    assert rc != 0 and b"overlap_pool_pairs" in L.spr_last_error()


@pytest.mark.parametrize("npairs", [1, 7])
def test_pair_layout_against_brute_force(npairs):
    pairs = GATHER_PAIRS[npairs]
    src, tgt = [i for i, _ in pairs], [j for _, j in pairs]
    lay = shared_clouds.PairLayout(src, tgt, LEVELS)
    order = src + tgt
    assert lay.npairs == npairs and lay.n_clouds == len(LENS) and lay.levels == 3
    assert lay.host["seg_cloud"].dtype == np.int32 and lay.host["seg_cloud"].tolist() == order
    # the use list: for every cloud, every segment that copies it, ascending
    ptr, seg = lay.host["use_ptr"], lay.host["use_seg"]
    assert ptr.dtype == seg.dtype == np.int32 and ptr.shape == (len(LENS) + 1,) and seg.shape == (2 * npairs,)
    assert ptr[0] == 0 and ptr[-1] == 2 * npairs
    for c in range(len(LENS)):
        want = [s for s in range(2 * npairs) if order[s] == c]
        got = seg[ptr[c]:ptr[c + 1]].tolist()
        assert got == want and got == sorted(got), c
    assert sorted(seg.tolist()) == list(range(2 * npairs))
    if npairs == 7:
        assert ptr[3] - ptr[2] == 0                                   # cloud 2: unused
        assert seg[ptr[4]:ptr[5]].tolist() == [1, 4, 9]               # cloud 4: src of pairs 1 and 4, tgt of pair 2
        assert seg[ptr[0]:ptr[1]].tolist() == [0, 5, 7, 11]           # the self-pair (0, 0): segments 0 and 7
    # per level: the segment lengths and their exclusive prefix
    for l, lens in enumerate(LEVELS):
        want = [lens[c] for c in order]
        assert lay.seg_lens[l] == want and lay.rows[l] == sum(want)
        cu = lay.host["cu_out"][l]
        assert cu.dtype == np.int32 and cu.tolist() == [sum(want[:k]) for k in range(2 * npairs + 1)]
    assert lay.seg_cloud is None and lay.cu_out is None               # no device given: nothing uploaded


def test_pair_layout_refuses_what_it_cannot_describe():
    with pytest.raises(ValueError):
        shared_clouds.PairLayout([], [], LEVELS)
    with pytest.raises(ValueError):
        shared_clouds.PairLayout([0, 1], [0], LEVELS)
    with pytest.raises(ValueError):
        shared_clouds.PairLayout([0], [5], LEVELS)
    with pytest.raises(ValueError):
        shared_clouds.PairLayout([0], [1], [LENS, LENS[:4]])
    with pytest.raises(ValueError):
        shared_clouds.PairLayout([0], [1], [[2 ** 30, 2 ** 30]])      # 2^31 rows on one level


@pytest.fixture(scope="module")
def model():
    return RegTR(get_config("3dmatch"))


def _batch(**over):
    clouds = [torch.zeros(10 + i, 3) for i in range(3)]
    b = {"clouds": clouds, "pairs": [(0, 1), (2, 2), (0, 1)], "pose": torch.zeros(3, 3, 4)}
    b.update(over)
    return {k: v for k, v in b.items() if v is not None}


@pytest.mark.parametrize("train", [True, False])
def test_forward_refuses_on_the_host(model, train):
    model.train(train)
    with pytest.raises(ValueError, match="not both"):
        model(_batch(src_xyz=[torch.zeros(10, 3)] * 3))
    with pytest.raises(ValueError, match="not both"):
        model(_batch(tgt_xyz=[torch.zeros(10, 3)] * 3))
    for bad in ((0, 3), (3, 0), (-1, 0), (0, 1.0), (True, 0)):
        with pytest.raises(ValueError, match="not an index in range"):
            model(_batch(pairs=[(0, 1), bad]))
    with pytest.raises(ValueError, match="src_index, tgt_index"):
        model(_batch(pairs=[(0, 1, 2)], pose=None))
    with pytest.raises(ValueError, match="one \\[3, 4\\] transform per pair"):
        model(_batch(pose=torch.zeros(2, 3, 4)))
    with pytest.raises(ValueError, match="empty pair list"):
        model(_batch(pairs=[], pose=None))
    with pytest.raises(ValueError, match="empty cloud list"):
        model(_batch(clouds=[]))
    with pytest.raises(ValueError, match="needs 'pairs'"):
        model({"clouds": [torch.zeros(10, 3)]})
    with pytest.raises(ValueError, match="one entry per pair"):
        model(_batch(pair_key=[1, 2]))
    # a CPU tensor follows the rule of every operator wrapper (ops._dev); the pose is optional (inference)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(_batch())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(_batch(pose=None))


def test_views_left_by_an_earlier_forward_are_legal(model):
    """forward leaves src_xyz / tgt_xyz = the per-pair views of the clouds in the batch; the same batch goes through a
    second step (Trainer.fit over a list of batches, several epochs) and is not mistaken for a mixed one."""
    b = _batch()
    b["src_xyz"], b["tgt_xyz"] = shared_clouds.pair_views(b)
    assert all(v is b["clouds"][i] for v, (i, _) in zip(b["src_xyz"], b["pairs"]))
    assert all(v is b["clouds"][j] for v, (_, j) in zip(b["tgt_xyz"], b["pairs"]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # past every ValueError
        shared_clouds.check_batch(b)
    b["src_xyz"] = [c.clone() for c in b["src_xyz"]]                  # equal values, other tensors: a mixed batch
    with pytest.raises(ValueError, match="not both"):
        shared_clouds.check_batch(b)


@pytest.mark.parametrize("train", [True, False])
def test_a_pair_list_batch_still_takes_the_old_path(model, train):
    model.train(train)
    b = {"src_xyz": [torch.zeros(10, 3)], "tgt_xyz": [torch.zeros(12, 3)]}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(b)
    assert set(b) == {"src_xyz", "tgt_xyz"}                           # nothing of the cloud route was left in it


def test_trainer_refusals(model):
    cfg = get_config("3dmatch")
    with pytest.raises(ValueError, match="augment"):
        Trainer(cfg, augment=True).train_step(model, _batch())
    tr = Trainer(cfg)
    with pytest.raises(ValueError, match="not an index in range"):
        tr.train_step(model, _batch(pairs=[(0, 1), (0, 1), (0, 7)]))
    with pytest.raises(ValueError, match="one \\[3, 4\\] transform per pair"):
        tr.validate(model, [_batch(pose=torch.zeros(1, 3, 4))])
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # labelling is the first device work
        tr.train_step(model, _batch())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.validate(model, [_batch()])
    assert Trainer(cfg, augment=True).global_step == 0


def test_operator_wrappers_refuse_cpu_tensors_and_bad_shapes():
    lay = shared_clouds.PairLayout([0], [1], [[4, 5], [2, 3]])
    i32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shared_clouds.pair_gather_bwd(torch.zeros(5, 8), i32([0, 2, 5]), i32(lay.host["use_ptr"]),
                                      i32(lay.host["use_seg"]), i32(lay.host["cu_out"][1]), rows=5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        shared_clouds.overlap_pool_pairs(torch.zeros(9), i32(np.zeros((5, 7))), i32([0, 4, 9]), i32([0, 2, 5]),
                                         i32(lay.host["seg_cloud"]), i32(lay.host["cu_out"][0]),
                                         i32(lay.host["cu_out"][1]), rows=5)
