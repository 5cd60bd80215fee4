"""GPU: the normals subpackage inside exactly the workspace it asks for, poisoned, and with every tensor -- inputs,
outputs, host-side scratch -- between guard bands: what tests/test_gpu_workspace.py and tests/test_gpu_tensor_bounds.py
guarantee for the package's top-level modules, given here for the subpackage with those modules' own helpers
(run_three, bounded).  Neither entry point takes a workspace of its own (there is no size query, so nothing can be
handed over a byte short); normals.estimate asks for one through its radius search, and both entry points run beside it
inside the poisoned arena.  The last test scans the subpackage's files: every spr_* entry point and every
`_workspace(` call site in them must have been reached by the cases above.  Run the module as a whole."""
import os
import re

import numpy as np
import pytest
import torch

import normals_cases as NC
import test_gpu_tensor_bounds as B
import test_gpu_workspace as W
from superpoints_registration_amd import _lib, normals, ops

pytestmark = pytest.mark.gpu
T = torch.from_numpy
PKG = os.path.dirname(normals.__file__)
RADIUS, LIMIT = 0.2, 40
# (C, triples): the in_feats_dim = 4 form, and two triples with scalar columns before, between and after
FORMS = [(4, (1,)), (9, (1, 5))]


@pytest.fixture(autouse=True)
def _recording(monkeypatch):
    real = _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: B._Recorder(real))


def _inputs(counts, c, device):
    """The clouds of test_gpu_workspace.py (a one-point cloud among them: m < 3), one viewpoint per cloud, features of
    mixed magnitude, a gather with repeats into clouds of other lengths (one of them empty) and their rotations."""
    host, pts, cu = W._clouds(counts, device, 2)
    rng = np.random.default_rng(7)
    n = len(host)
    view = rng.uniform(2, 3, (len(counts), 3)).astype(np.float32)
    feat = (rng.normal(0, 1, (n, c)) * 10.0 ** rng.uniform(-3, 3, (n, c))).astype(np.float32)
    lens_out = [counts[1], 0, counts[0] + 3]
    rows = rng.integers(0, n, sum(lens_out)).astype(np.int32)
    rot = np.stack([NC.rot_matrix(20 + b) for b in range(3)]).astype(np.float32)
    return host, pts, cu, view, feat, lens_out, rows, rot


def _check(counts, host, view, feat, lens_out, rows, rot, cols, got):
    nrm, curv, nbr, again, moved = got
    NC.check(host, nbr.cpu().numpy(), list(counts), view, nrm.cpu().numpy(), curv.cpu().numpy(), f"guarded {counts}",
             cap_gap_share=False)
    assert torch.equal(nrm.view(torch.int32), again.view(torch.int32))
    want = NC.gather_rotate(feat, rows, lens_out, rot, cols)
    assert np.array_equal(moved.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("c,cols", FORMS)
@pytest.mark.parametrize("counts", W.POINT_COUNTS)
def test_inside_the_workspace_it_asks_for(device, monkeypatch, counts, c, cols):
    host, pts, cu, view, feat, lens_out, rows, rot = _inputs(counts, c, device)
    d_view, d_feat, d_rows, d_rot = (T(a).to(device) for a in (view, feat, rows, rot))
    cu_out = ops.lengths_to_cu(lens_out, device)

    def f():
        nrm, curv = normals.estimate(pts, cu, RADIUS, LIMIT, viewpoint=d_view, curvature=True)
        nbr, _ = ops.radius_neighbors(pts, pts, cu, cu, RADIUS, LIMIT)
        again = normals.from_neighbors(pts, nbr, cu, d_view)
        return nrm, curv, nbr, again, normals.gather_rotate(d_feat, d_rows, cu_out, d_rot, cols)
    got = W.run_three(monkeypatch, f, f"normals {counts} C{c}")
    _check(counts, host, view, feat, lens_out, rows, rot, cols, got)


@pytest.mark.parametrize("c,cols", FORMS)
@pytest.mark.parametrize("counts", W.POINT_COUNTS)
def test_with_every_tensor_between_guard_bands(device, monkeypatch, counts, c, cols):
    host, pts, cu, view, feat, lens_out, rows, rot = _inputs(counts, c, device)
    wide, _ = ops.radius_neighbors(pts, pts, cu, cu, RADIUS, LIMIT)

    def f(put):
        p, q, v = put(pts.clone()), put(cu.clone()), put(T(view).to(device))
        nrm, curv = normals.estimate(p, q, RADIUS, LIMIT, viewpoint=v, curvature=True)
        nbr = put(wide.contiguous().clone())
        again = normals.from_neighbors(p, nbr, q, v)
        moved = normals.gather_rotate(put(T(feat).to(device)), put(T(rows).to(device)),
                                      put(ops.lengths_to_cu(lens_out, device)), put(T(rot).to(device)), cols)
        return nrm, curv, nbr, again, moved
    got = B.bounded(monkeypatch, f, f"normals {counts} C{c}")
    _check(counts, host, view, feat, lens_out, rows, rot, cols, got)


# ---- coverage: keep this test last -----------------------------------------------------------------------------------
def test_every_entry_point_and_workspace_site_of_the_subpackage_was_reached(device):
    names = sorted(n for n in os.listdir(PKG) if n.endswith(".py"))
    assert names
    text = "".join(open(os.path.join(PKG, n)).read() for n in names)
    referenced = {n for n in _lib.SIGNATURES if re.search(rf"\b{n}\b", text)}
    assert {"spr_estimate_normals", "spr_feats_gather_rotate"} <= referenced
    wanted = {n for n in referenced if not any(re.search(p, n) for p in B.EXEMPT)}
    assert {"spr_estimate_normals", "spr_feats_gather_rotate"} <= wanted
    missing = sorted(n for n in wanted if n not in B.CALLED)
    assert not missing, f"no case of this module called {missing} with guarded tensors"
    # the subpackage carves no workspace of its own today; a call site that appears must be reached by a case above
    sites = [(name, no) for name in names for no, line in enumerate(open(os.path.join(PKG, name)).read().splitlines(), 1)
             if re.search(r"_workspace\(|_loss_ws\(", line) and not re.match(r"\s*def (_workspace|_loss_ws)\(", line)]
    unreached = [s for s in sites if s not in W.SEEN]
    assert not unreached, f"no case of this module reached {unreached}"
