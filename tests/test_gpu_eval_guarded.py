"""GPU: the evaluation subpackage inside exactly the workspace it asks for, poisoned, and with every tensor -- clouds,
correspondences, poses, outputs -- between guard bands: what tests/test_gpu_workspace.py and
tests/test_gpu_tensor_bounds.py guarantee for the package's top-level modules, given here with the same helpers
(run_three, bounded, _one_byte_short).  `ragged`: five pairs, empty clouds, a partial query block and a partial target
tile (the clouds are concatenated by the host layer); `ones`: one pair of one-point clouds, handed to the library as
they are; `tiles`: whole and partial tiles in both directions.  Each case also runs in the forms without the raw shape
and without correspondences.  The last test scans the subpackage's files: every spr_* entry point and every
`_workspace(` call site in them must have been reached by the cases above.  Run the module as a whole."""
import os
import re

import pytest
import torch

import eval_cases as C
import test_gpu_tensor_bounds as B
import test_gpu_workspace as W
from superpoints_registration_amd import _lib, evaluation
from test_gpu_eval import check_against_replica, run

pytestmark = pytest.mark.gpu
PKG = os.path.dirname(evaluation.__file__)
ENTRY_POINTS = {"spr_eval_pairs"}
CASES = ["ragged", "ones", "tiles"]


@pytest.fixture(autouse=True)
def _recording(monkeypatch):
    real = _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: B._Recorder(real))


def _case_fn(name, device):
    """f(put): the whole call, then the forms without the raw shape and without correspondences.  The per-column views
    of 'metrics' are left out: the table itself is compared."""
    def f(put=lambda t: t):
        outs = (run(name, device, put=put), run(name, device, put=put, raw=False), run(name, device, put=put, corr=False))
        return tuple({k: v for k, v in o.items() if k not in evaluation.COLUMNS} for o in outs)
    return f


def _check(name, got):
    whole = dict(got[0])
    whole.update({k: whole["metrics"][:, i] for i, k in enumerate(evaluation.COLUMNS)})
    check_against_replica(name, whole, C.replica(name))
    assert torch.equal(got[1]["metrics"][:, :7], got[0]["metrics"][:, :7])
    assert torch.equal(got[2]["metrics"][:, :10], got[0]["metrics"][:, :10])


@pytest.mark.parametrize("name", CASES)
def test_inside_the_workspace_it_asks_for(device, monkeypatch, name):
    _check(name, W.run_three(monkeypatch, _case_fn(name, device), f"evaluation {name}"))


@pytest.mark.parametrize("name", CASES)
def test_with_every_tensor_between_guard_bands(device, monkeypatch, name):
    _check(name, B.bounded(monkeypatch, _case_fn(name, device), f"evaluation {name}"))


@pytest.mark.parametrize("raw", [True, False], ids=["chamfer", "poses"])
@pytest.mark.parametrize("name", CASES)
def test_one_byte_short_is_refused(device, monkeypatch, name, raw):
    """The size query minus one byte: the operator's own status (RuntimeError naming the workspace), nothing written,
    guards intact; the query's own size is what test_inside_the_workspace_it_asks_for hands over."""
    c = C.case(name)
    ns, nt, nr = (sum(len(x) for x in c[k]) for k in ("src", "ref", "raw"))
    assert _lib.lib().spr_eval_pairs_workspace_size(ns, nt, nr, 0, len(c["src"])) >= 24 * (ns + nr)
    W._one_byte_short(monkeypatch, f"evaluation {name} raw={raw}", lambda: None,
                      lambda _: {k: v for k, v in run(name, device, raw=raw).items() if k not in evaluation.COLUMNS})


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
