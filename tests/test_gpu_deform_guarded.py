"""GPU: the deformable subpackage inside exactly the workspace it asks for, poisoned, and with every tensor -- inputs,
outputs, host-side scratch -- between guard bands: what tests/test_gpu_workspace.py and tests/test_gpu_tensor_bounds.py
guarantee for the package's top-level modules, given here for the subpackage with those modules' own helpers
(run_three, bounded).  Every entry point, forward and backward, on the tile route and the one-thread-per-output route,
modulated and not; each of the three carved workspaces handed over one byte short.  The last test scans the
subpackage's files: every spr_* entry point and every `_workspace(` call site in them must have been reached by the
cases above.  Run the module as a whole."""
import os
import re

import pytest
import torch

import deform_cases as dc
import test_gpu_tensor_bounds as B
import test_gpu_workspace as W
from superpoints_registration_amd import _lib, deformable, synthetic
from test_gpu_backward import _rel
from test_gpu_deform import MOD, _chain_grads, case_of, mod_id, on_device, run_kernel, scale_err

pytestmark = pytest.mark.gpu
PKG = os.path.dirname(deformable.__file__)
ENTRY_POINTS = {"spr_kpconv_deform_fwd", "spr_kpconv_deform_weighted_features", "spr_kpconv_deform_bwd_dx",
                "spr_kpconv_deform_bwd_offsets"}
# the tile route with rows wider than one staging pass, the strided tile route at 32-channel chunks, the simple route
CASES = ["nq130 k70 64-256 int64 unsorted", "strided nq37 ns130 k33 32-64", "simple 48-40", "simple cin1 1-32"]


@pytest.fixture(autouse=True)
def _recording(monkeypatch):
    real = _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: B._Recorder(real))


def _case_fn(name, modulated, device):
    """f(put): the chain's forward and backward (all four entry points), then the plain forward with min_d2 on the
    route the shape takes and on the one-thread-per-output route.  Fresh tensors per run: the weight planes are built
    inside the arena."""
    case, _, aux, go, _ = case_of(name, modulated)

    def f(put=lambda t: t):
        out, grads = _chain_grads(case, go, device, put)
        d = on_device(case, device, put)
        of = put(aux["offset_features"].float().to(device))
        with torch.no_grad():
            plain, min_d2 = run_kernel(d, of, want_min_d2=True)
            simple = run_kernel(on_device(case, device, put), of, impl=1)
        return out, plain, min_d2, simple, grads
    return f


def _check(name, modulated, got):
    _, ref, aux, _, gref = case_of(name, modulated)
    out, plain, min_d2, simple, grads = got
    assert scale_err(out, ref) <= 1e-5 and scale_err(plain, ref) <= 1e-5 and scale_err(simple, ref) <= 1e-5
    assert float(((min_d2.double().cpu() - aux["min_d2"]).abs() / aux["min_d2"]).max()) <= 1e-5
    for k in ("dx", "dw", "d_of"):
        assert _rel(grads[k], gref[k]) <= 2e-5, k


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
@pytest.mark.parametrize("name", CASES)
def test_inside_the_workspace_it_asks_for(device, monkeypatch, name, modulated):
    got = W.run_three(monkeypatch, _case_fn(name, modulated, device), f"deformable {name} {mod_id(modulated)}")
    _check(name, modulated, got)


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
@pytest.mark.parametrize("name", CASES)
def test_with_every_tensor_between_guard_bands(device, monkeypatch, name, modulated):
    got = B.bounded(monkeypatch, _case_fn(name, modulated, device), f"deformable {name} {mod_id(modulated)}")
    _check(name, modulated, got)


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
@pytest.mark.parametrize("name", ["nq37 k5 64-64", "simple 48-40"])
def test_one_byte_short_is_refused(device, monkeypatch, name, modulated):
    """Each of the three entry points that carve a workspace, handed its size query minus one byte: the operator's own
    status (RuntimeError naming the workspace), nothing written, guards intact."""
    case, _, aux, _, _ = case_of(name, modulated)
    d = on_device(case, device)
    of = aux["offset_features"].float().to(device)
    cin = d["x"].shape[1]
    dwfm = synthetic.rand((d["q"].shape[0], d["kp"].shape[0] * cin), 5).to(device)
    W._one_byte_short(monkeypatch, f"deformable forward {name}", lambda: None,
                      lambda _: deformable.kpconv_deform_raw(d["q"], d["s"], d["idx"], d["x"], d["w"].clone(), d["kp"],
                                                             d["extent"], of, modulated))
    W._one_byte_short(monkeypatch, f"deformable weighted features {name}", lambda: None,
                      lambda _: deformable.weighted_features(d["q"], d["s"], d["idx"], d["x"], d["kp"], d["extent"], of))
    W._one_byte_short(monkeypatch, f"deformable bwd_dx {name}", lambda: None,
                      lambda _: deformable.bwd_dx(d["q"], d["s"], d["idx"], cin, d["kp"], d["extent"], of, modulated, dwfm))


# ---- coverage: keep this test last -----------------------------------------------------------------------------------
def test_every_entry_point_and_workspace_site_of_the_subpackage_was_reached(device):
    names = sorted(n for n in os.listdir(PKG) if n.endswith(".py"))
    assert names
    text = "".join(open(os.path.join(PKG, n)).read() for n in names)
    referenced = {n for n in _lib.SIGNATURES if re.search(rf"\b{n}\b", text)}
    assert ENTRY_POINTS <= referenced
    wanted = {n for n in referenced if not any(re.search(p, n) for p in B.EXEMPT)}
    assert ENTRY_POINTS <= wanted
    missing = sorted(n for n in wanted if n not in B.CALLED)
    assert not missing, f"no case of this module called {missing} with guarded tensors"
    sites = [(name, no) for name in names for no, line in enumerate(open(os.path.join(PKG, name)).read().splitlines(), 1)
             if re.search(r"_workspace\(|_loss_ws\(", line) and not re.match(r"\s*def (_workspace|_loss_ws)\(", line)]
    assert len(sites) == 3, sites                      # forward, weighted features, the scatter
    unreached = [s for s in sites if s not in W.SEEN]
    assert not unreached, f"no case of this module reached {unreached}"
