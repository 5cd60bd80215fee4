"""CPU: the host side of encode-once registration -- the C-ABI entry point spr_pair_gather is declared, exported and
bound; RegTR.encode / RegTR.register reject bad input before any launch; EncodedClouds keeps the right counts."""
import ctypes
import os
import re

import pytest
import torch

from superpoints_registration_amd import _lib, get_config
from superpoints_registration_amd.regtr import EncodedClouds, RegTR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_gather_is_declared_exported_and_bound():
    text = open(os.path.join(REPO, "include", "spr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+spr_pair_gather\s*\(", text)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "spr_pair_gather")
    assert "spr_pair_gather" in _lib.SIGNATURES
    # bad arguments are rejected on the host before any HIP call
    L = _lib.lib()
    rc = L.spr_pair_gather(None, 10, 256, None, 2, None, None, 1, None, 10, None, None)
    assert rc != 0 and b"pair_gather" in L.spr_last_error()


def _enc(lens, d=8, meta=None):
    """An encoding on the CPU: enough for everything register() checks before it touches the device."""
    n = sum(lens)
    tokens = torch.arange(n * d, dtype=torch.float32).view(n, d)
    points = torch.arange(n * 3, dtype=torch.float32).view(n, 3)
    return EncodedClouds(tokens, points, lens, kpconv_meta=meta)


@pytest.fixture(scope="module")
def model():
    return RegTR(get_config("3dmatch")).eval()


def test_rejected_input(model):
    enc = _enc([5, 7, 3])
    with pytest.raises(ValueError, match="empty cloud list"):
        model.encode([])
    with pytest.raises(ValueError, match="empty pair list"):
        model.register(enc, [])
    for bad in ((0, 3), (3, 0), (-1, 0), (0, 1.0)):
        with pytest.raises(ValueError, match="not an index in range"):
            model.register(enc, [(0, 1), bad])
    # a CPU tensor follows the rule of every operator wrapper (ops._dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.encode([torch.zeros(10, 3)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.register(enc, [(0, 1), (2, 2)])


def test_training_mode_is_refused():
    m = RegTR(get_config("3dmatch"))
    m.train()
    with pytest.raises(RuntimeError, match="inference"):
        m.encode([torch.zeros(10, 3)])
    with pytest.raises(RuntimeError, match="inference"):
        m.register(_enc([4, 4]), [(0, 1)])


def test_select_and_cat_keep_the_counts():
    lens = [5, 1, 7, 3]
    enc = _enc(lens, meta={"points": []})
    assert len(enc) == 4 and enc.lens == lens
    assert enc.cu.dtype == torch.int32 and enc.cu.tolist() == [0, 5, 6, 13, 16]

    sel = enc.select([2, 0, 2])
    assert len(sel) == 3 and sel.lens == [7, 5, 7] and sel.cu.tolist() == [0, 7, 12, 19]
    assert sel.kpconv_meta is None
    assert torch.equal(sel.tokens, torch.cat([enc.tokens[6:13], enc.tokens[0:5], enc.tokens[6:13]]))
    assert torch.equal(sel.points, torch.cat([enc.points[6:13], enc.points[0:5], enc.points[6:13]]))

    both = EncodedClouds.cat([enc.select([0, 1]), enc.select([2, 3])])
    assert both.lens == lens and both.cu.tolist() == enc.cu.tolist() and both.kpconv_meta is None
    assert torch.equal(both.tokens, enc.tokens) and torch.equal(both.points, enc.points)
    longer = EncodedClouds.cat([enc, _enc([2])])          # a sequence appends the next frame
    assert longer.lens == lens + [2] and longer.cu.tolist() == [0, 5, 6, 13, 16, 18]
    assert longer.kpconv_meta is None and enc.kpconv_meta is not None

    for bad in ([4], [-1], []):
        with pytest.raises(ValueError):
            enc.select(bad)
    with pytest.raises(ValueError):
        EncodedClouds.cat([])
    with pytest.raises(ValueError):
        EncodedClouds(torch.zeros(4, 8), torch.zeros(4, 3), [3, 2])
