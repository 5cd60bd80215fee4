"""GPU: the icp_plane subpackage inside exactly the workspace it asks for, poisoned, and with every tensor -- clouds,
normals, poses, outputs -- between guard bands: what tests/test_gpu_workspace.py and tests/test_gpu_tensor_bounds.py
guarantee for the package's top-level modules, given here with the same helpers (run_three, bounded, _one_byte_short).
`ragged`: five pairs, a partial association block, empty clouds (clouds and normals are concatenated by the host
layer); `corner_slide`: one pair, four steps, its tensors handed to the library as they are; `robust_tukey`: a robust
kernel.  The last test scans the subpackage's files: every spr_* entry point and every `_workspace(` call site in them
must have been reached by the cases above.  Run the module as a whole."""
import os
import re

import pytest

import icp_plane_cases as C
import test_gpu_tensor_bounds as B
import test_gpu_workspace as W
from superpoints_registration_amd import _lib, icp_plane
from test_gpu_icp_plane import check_against_replica, run

pytestmark = pytest.mark.gpu
PKG = os.path.dirname(icp_plane.__file__)
ENTRY_POINTS = {"spr_icp_plane_pairs"}
CASES = ["ragged", "corner_slide", "robust_tukey"]


@pytest.fixture(autouse=True)
def _recording(monkeypatch):
    real = _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: B._Recorder(real))


def _case_fn(name, device):
    """f(put): the iteration, then the pure evaluation of the initial poses."""
    def f(put=lambda t: t):
        return run(name, device, put=put), run(name, device, max_iter=0, put=put)
    return f


def _check(name, got):
    check_against_replica(name, got[0], C.replica(name))
    check_against_replica(name, got[1], C.replica(name, 0.0, 0), exact_pose=True)


@pytest.mark.parametrize("name", CASES)
def test_inside_the_workspace_it_asks_for(device, monkeypatch, name):
    _check(name, W.run_three(monkeypatch, _case_fn(name, device), f"icp_plane {name}"))


@pytest.mark.parametrize("name", CASES)
def test_with_every_tensor_between_guard_bands(device, monkeypatch, name):
    _check(name, B.bounded(monkeypatch, _case_fn(name, device), f"icp_plane {name}"))


@pytest.mark.parametrize("max_iter", [0, 30], ids=["evaluate", "iterate"])
@pytest.mark.parametrize("name", CASES[:2])
def test_one_byte_short_is_refused(device, monkeypatch, name, max_iter):
    """The size query minus one byte: the operator's own status (RuntimeError naming the workspace), nothing written,
    guards intact; the query's own size is what test_inside_the_workspace_it_asks_for hands over."""
    c = C.case(name)
    ns, nt = sum(len(x) for x in c["src"]), sum(len(x) for x in c["tgt"])
    assert _lib.lib().spr_icp_plane_pairs_workspace_size(ns, nt, len(c["src"])) > 64 * nt
    W._one_byte_short(monkeypatch, f"icp_plane {name} max_iter={max_iter}", lambda: None,
                      lambda _: run(name, device, max_iter=max_iter))


# ---- coverage: keep this test last -----------------------------------------------------------------------------------
def test_every_entry_point_and_workspace_site_of_the_subpackage_was_reached(device):
    names = sorted(n for n in os.listdir(PKG) if n.endswith(".py"))
    assert names
    text = "".join(open(os.path.join(PKG, n)).read() for n in names)
    referenced = {n for n in _lib.SIGNATURES if re.search(rf"\b{n}\b", text)}
    assert ENTRY_POINTS <= referenced
    wanted = {n for n in referenced if not any(re.search(p, n) for p in B.EXEMPT)}
    assert ENTRY_POINTS == wanted
    missing = sorted(n for n in wanted if n not in B.CALLED)
    assert not missing, f"no case of this module called {missing} with guarded tensors"
    sites = [(name, no) for name in names for no, line in enumerate(open(os.path.join(PKG, name)).read().splitlines(), 1)
             if re.search(r"_workspace\(|_loss_ws\(", line) and not re.match(r"\s*def (_workspace|_loss_ws)\(", line)]
    assert len(sites) == 1, sites
    unreached = [s for s in sites if s not in W.SEEN]
    assert not unreached, f"no case of this module reached {unreached}"
