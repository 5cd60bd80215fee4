"""GPU: subsample_attrs.grid_subsample inside exactly the workspace it asks for, poisoned, and with every tensor --
inputs, outputs, host-side scratch -- between guard bands: what tests/test_gpu_workspace.py and
tests/test_gpu_tensor_bounds.py guarantee for the package's top-level modules, given here for the subpackage with those
modules' own helpers (run_three, _one_byte_short, bounded).  The last test scans the subpackage's files: every spr_*
entry point and every `_workspace(` call site in them must have been reached by the cases above.  Run the module as a
whole."""
import os
import re

import numpy as np
import pytest
import torch

import subsample_attrs_replica as R
import test_gpu_tensor_bounds as B
import test_gpu_workspace as W
from superpoints_registration_amd import _lib, ops, subsample_attrs

pytestmark = pytest.mark.gpu
T = torch.from_numpy
PKG = os.path.dirname(subsample_attrs.__file__)
# (fdim, ldim, order): both passes together and alone, one and several label columns, both order modes
FORMS = [(3, 1, ops.ORDER_REFERENCE), (33, 3, ops.ORDER_CANONICAL), (0, 3, ops.ORDER_REFERENCE), (4, 0, ops.ORDER_CANONICAL)]


@pytest.fixture(autouse=True)
def _recording(monkeypatch):
    real = _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: B._Recorder(real))


def _inputs(counts, fdim, ldim, device):
    """The clouds of test_gpu_workspace.py (0.2 grid: two points per voxel on average), features of mixed magnitude, labels
    from a palette of four (small voxels tie)."""
    host, pts, cu = W._clouds(counts, device, 1)
    rng = np.random.default_rng(7)
    n = len(host)
    feat = (rng.normal(0, 1, (n, fdim)) * 10.0 ** rng.uniform(-3, 3, (n, fdim))).astype(np.float32) if fdim else None
    lab = np.array([5, -1, 18, -(1 << 31)], np.int32)[rng.integers(0, 4, (n, ldim))] if ldim else None
    return host, feat, lab, pts, cu


def _check(counts, order, host, feat, lab, got):
    e = R.grid_subsample(host, list(counts), 0.2, 0, "reference" if order == ops.ORDER_REFERENCE else "canonical", feat, lab)
    want = [e[0], e[1]] + [x for x in e[2:] if x is not None]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g = g.cpu().numpy()
        assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32))


@pytest.mark.parametrize("fdim,ldim,order", FORMS)
@pytest.mark.parametrize("counts", W.POINT_COUNTS)
def test_inside_the_workspace_it_asks_for(device, monkeypatch, counts, fdim, ldim, order):
    host, feat, lab, pts, cu = _inputs(counts, fdim, ldim, device)
    d_feat, d_lab = (None if a is None else T(a).to(device) for a in (feat, lab))
    got = W.run_three(monkeypatch, lambda: subsample_attrs.grid_subsample(pts, cu, 0.2, order=order, features=d_feat,
                                                                          labels=d_lab), f"subsample_attrs {counts} f{fdim} l{ldim}")
    _check(counts, order, host, feat, lab, got)


@pytest.mark.parametrize("fdim,ldim,order", FORMS)
@pytest.mark.parametrize("counts", W.POINT_COUNTS)
def test_with_every_tensor_between_guard_bands(device, monkeypatch, counts, fdim, ldim, order):
    host, feat, lab, pts, cu = _inputs(counts, fdim, ldim, device)

    def f(put):
        d_feat, d_lab = (None if a is None else put(T(a).to(device)) for a in (feat, lab))
        return subsample_attrs.grid_subsample(put(pts.clone()), put(cu.clone()), 0.2, order=order, features=d_feat,
                                              labels=d_lab)
    got = B.bounded(monkeypatch, f, f"subsample_attrs {counts} f{fdim} l{ldim}")
    _check(counts, order, host, feat, lab, got)


def test_one_byte_short_is_refused(device, monkeypatch):
    host, feat, lab, pts, cu = _inputs(W.POINT_COUNTS[0], 3, 1, device)
    d_feat, d_lab = T(feat).to(device), T(lab).to(device)
    for what, kw in (("attrs", dict(features=d_feat, labels=d_lab)), ("attrs, labels only", dict(labels=d_lab)),
                     ("attrs, neither", dict())):
        W._one_byte_short(monkeypatch, what, lambda: None, lambda _, kw=kw: subsample_attrs.grid_subsample(pts, cu, 0.2, **kw))


# ---- coverage: keep this test last -----------------------------------------------------------------------------------
def test_every_entry_point_and_workspace_site_of_the_subpackage_was_reached(device):
    names = sorted(n for n in os.listdir(PKG) if n.endswith(".py"))
    assert names
    text = "".join(open(os.path.join(PKG, n)).read() for n in names)
    referenced = {n for n in _lib.SIGNATURES if re.search(rf"\b{n}\b", text)}
    assert {"spr_grid_subsample_attrs", "spr_grid_subsample_attrs_workspace_size"} <= referenced
    wanted = {n for n in referenced if not any(re.search(p, n) for p in B.EXEMPT)}
    assert "spr_grid_subsample_attrs" in wanted
    missing = sorted(n for n in wanted if n not in B.CALLED)
    assert not missing, f"no case of this module called {missing} with guarded tensors"
    sites = [(name, no) for name in names for no, line in enumerate(open(os.path.join(PKG, name)).read().splitlines(), 1)
             if re.search(r"_workspace\(|_loss_ws\(", line) and not re.match(r"\s*def (_workspace|_loss_ws)\(", line)]
    assert len(sites) >= 1
    unreached = [s for s in sites if s not in W.SEEN]
    assert not unreached, f"no case of this module reached {unreached}"
