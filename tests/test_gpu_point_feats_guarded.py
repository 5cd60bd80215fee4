"""GPU: ops.kpconv_raw on per-point input features (2 <= Cin <= 8, the small-Cin kernel and its record pass) inside
exactly the workspace spr_kpconv_workspace_bytes reports, poisoned, one byte short, and with every tensor between guard
bands -- tests/test_gpu_workspace.py's run_three / _one_byte_short and tests/test_gpu_tensor_bounds.py's bounded, on the
cases of tests/point_feats_cases.py (held against float64 in tests/test_gpu_point_feats.py; the same bound is asserted
here on the production run)."""
import numpy as np
import pytest
import torch

import forward_cases as fc
import point_feats_cases as pc
import test_gpu_tensor_bounds as B
import test_gpu_workspace as W
from superpoints_registration_amd import _lib, ops

pytestmark = pytest.mark.gpu
T = torch.from_numpy
# (nq, ns, kmax, cout, rows_sorted): one wave short of a workgroup with rows of one record batch; several workgroups
# with rows of three staged chunks and a partial 16-column block
FORMS = [(17, 60, 8, 64, True), (150, 200, 129, 40, False)]


@pytest.fixture(autouse=True)
def _recording(monkeypatch):
    real = _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: B._Recorder(real))


def _case(c, form):
    nq, ns, kmax, cout, srt = form
    q, s, nb, x, w, kp, ext = pc.kernel_case(nq, ns, kmax, c, cout, 2000 + c, "signed", rows_sorted=srt)
    pc.check_conditions(x)
    return (q, s, nb.astype(np.int32), x, w, kp), ext, srt, fc.kpconv_f64(q, s, nb, x, w, kp, ext)


def _held(y, ref, what):
    err, scale = float(np.abs(y.cpu().double().numpy() - ref).max()), float(np.abs(ref).max())
    assert scale > 0 and err <= 1e-5 * scale, f"{what}: {err:.3e} > 1e-5 * {scale:.3e}"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("c", [2, 4, 8])
def test_inside_the_workspace_it_asks_for(device, monkeypatch, c, form):
    host, ext, srt, ref = _case(c, form)
    dev = [T(np.ascontiguousarray(a)).to(device) for a in host]
    y = W.run_three(monkeypatch, lambda: ops.kpconv_raw(*dev, ext, rows_sorted=srt), f"kpconv few C={c} {form}")
    _held(y, ref, f"kpconv few C={c} {form}")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("c", [2, 4, 8])
def test_with_every_tensor_between_guard_bands(device, monkeypatch, c, form):
    host, ext, srt, ref = _case(c, form)

    def f(put):
        dev = [put(T(np.ascontiguousarray(a)).to(device)) for a in host]
        return ops.kpconv_raw(*dev, ext, rows_sorted=srt)
    y = B.bounded(monkeypatch, f, f"kpconv few C={c} {form}")
    _held(y, ref, f"kpconv few C={c} {form}")
    assert "spr_kpconv_fwd" in B.CALLED


@pytest.mark.parametrize("c", [2, 4, 8])
def test_one_byte_short_is_refused(device, monkeypatch, c):
    host, ext, srt, _ = _case(c, FORMS[0])
    dev = [T(np.ascontiguousarray(a)).to(device) for a in host]
    W._one_byte_short(monkeypatch, f"kpconv few C={c}", lambda: None, lambda _: ops.kpconv_raw(*dev, ext, rows_sorted=srt))
