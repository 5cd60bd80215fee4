"""GPU: the deform_reg subpackage inside exactly the workspace it asks for, poisoned, and with every tensor -- inputs,
outputs, the gradient row, host-side scratch -- between guard bands: what tests/test_gpu_workspace.py and
tests/test_gpu_tensor_bounds.py guarantee for the package's top-level modules and tests/test_gpu_deform_guarded.py for
the deformable subpackage, given here with the same helpers (run_three, bounded, _one_byte_short).  The launch with and
without the gradient, on rows narrower than one 16-lane pass with shadows and an all-shadow row, and on int64 rows wider
than four passes.  The last test scans the subpackage's files: every spr_* entry point and every `_workspace(` call
site in them must have been reached by the cases above.  Run the module as a whole."""
import os
import re

import pytest
import torch

import deform_reg_cases as rc
import test_gpu_tensor_bounds as B
import test_gpu_workspace as W
from superpoints_registration_amd import _lib, deform_reg
from test_gpu_backward import _rel
from test_gpu_deform import on_device

pytestmark = pytest.mark.gpu
PKG = os.path.dirname(deform_reg.__file__)
ENTRY_POINTS = {"spr_deform_reg"}
CASES = ["nq37 k5 64-64", "nq130 k70 64-256 int64 unsorted"]
MOD, mod_id = rc.MOD, rc.mod_id


@pytest.fixture(autouse=True)
def _recording(monkeypatch):
    real = _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: B._Recorder(real))


def _case_fn(name, modulated, device):
    """f(put): the launch with the gradient (through the autograd Function and its backward), then without."""
    case, ref = rc.case_of(name, modulated)

    def f(put=lambda t: t):
        d = on_device(case, device, put)
        of = put(ref["offset_features"].float().to(device)).requires_grad_(True)
        value, fit, rep = deform_reg.deform_reg(d["q"], d["s"], d["idx"], of, d["kp"], d["extent"], rc.R_DEFAULT)
        value.backward()
        with torch.no_grad():
            plain = deform_reg.deform_reg(d["q"], d["s"], d["idx"], of, d["kp"], d["extent"], rc.R_DEFAULT)
        return value.detach(), fit, rep, of.grad, list(plain)
    return f


def _check(name, modulated, got):
    _, ref = rc.case_of(name, modulated)
    value, fit, rep, d_of, plain = got
    for k, v in (("value", value), ("fit", fit), ("rep", rep)):
        assert abs(float(v) - float(ref[k])) <= 1e-5 * float(ref[k]), k
    assert _rel(d_of, ref["d_of"]) <= 1e-5
    for a, b in zip((value, fit, rep), plain):
        assert torch.equal(a, b)


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
@pytest.mark.parametrize("name", CASES)
def test_inside_the_workspace_it_asks_for(device, monkeypatch, name, modulated):
    got = W.run_three(monkeypatch, _case_fn(name, modulated, device), f"deform_reg {name} {mod_id(modulated)}")
    _check(name, modulated, got)


@pytest.mark.parametrize("modulated", MOD, ids=mod_id)
@pytest.mark.parametrize("name", CASES)
def test_with_every_tensor_between_guard_bands(device, monkeypatch, name, modulated):
    got = B.bounded(monkeypatch, _case_fn(name, modulated, device), f"deform_reg {name} {mod_id(modulated)}")
    _check(name, modulated, got)


@pytest.mark.parametrize("grad", [True, False], ids=["gradient", "value"])
@pytest.mark.parametrize("name", CASES)
def test_one_byte_short_is_refused(device, monkeypatch, name, grad):
    """The size query minus one byte: the operator's own status (RuntimeError naming the workspace), nothing written,
    guards intact; the query's own size is what test_inside_the_workspace_it_asks_for hands over."""
    case, ref = rc.case_of(name, False)
    d = on_device(case, device)
    of = ref["offset_features"].float().to(device)
    nq = d["q"].shape[0]
    assert _lib.lib().spr_deform_reg_workspace_size(nq) == 256 * -(-(2 * 8 * -(-nq // 16)) // 256)
    W._one_byte_short(monkeypatch, f"deform_reg {name} grad={grad}", lambda: None,
                      lambda _: deform_reg.deform_reg_raw(d["q"], d["s"], d["idx"], of, d["kp"], d["extent"],
                                                          rc.R_DEFAULT, want_grad=grad))


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
    assert len(sites) == 1, sites
    unreached = [s for s in sites if s not in W.SEEN]
    assert not unreached, f"no case of this module reached {unreached}"
