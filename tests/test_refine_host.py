"""CPU: the refinement head's contract without a GPU -- the float64 replica (tests/refine_replica.py) against the
reference's own outputs (tests/golden/refine_ops.npz, scripts/gen_refine_golden.py), the C ABI and the host-side
argument checks of ops.refine_pairs."""
import ctypes

import numpy as np
import pytest
import torch

import refine_replica
from conftest import load_golden
from oracle.gen_golden import REFINE_CASES
from superpoints_registration_amd import _lib, ops

REPLICA_KW = {"use_ratio_test": "ratio", "threshold_corr": "median", "remove_outliers_overlap": "overlap",
              "use_overlap_as_weights": "overlap_w"}
# The float32 reference against the float64 replica: gen_refine_golden.py observed at most 1.8e-6 (Frobenius, [3,4]) over
# all cases -- translations of a few metres carry a float32 ulp of ~5e-7 per entry.  The bound leaves a factor of ~5.
POSE_BOUND = 1e-5


def replica_case(g, case, b, **extra):
    flags = REFINE_CASES[case]
    n, m = g[f"src{b}"].shape[0], g[f"tgt{b}"].shape[0]
    kw = {REPLICA_KW[f]: True for f in flags if f in REPLICA_KW}
    k = int(float(g["val_threshold"]) * min(n, m)) if flags.get("remove_points_from_val") else None
    return refine_replica.refine_pair(
        g[f"val_in{b}"], g[f"val2_in{b}"], g[f"ind_in{b}"], g[f"ov_s{b}"], g[f"ov_t{b}"], g[f"src{b}"], g[f"tgt{b}"],
        k=k, lgr_steps=int(g["num_refinement_steps"]) if flags.get("use_lgr") else 0,
        lowe_thres=float(g["lowe_thres"]), radius=float(g["acceptance_radius"]), **kw, **extra)


@pytest.mark.parametrize("case", list(REFINE_CASES))
def test_replica_reproduces_the_reference(case):
    g = load_golden("refine_ops.npz")
    assert list(g["cases"]) == list(REFINE_CASES)
    for b in range(int(g["B"])):
        pose, val, ind, a, bb = replica_case(g, case, b)
        rv, ri = g[f"{case}.val{b}"], g[f"{case}.ind{b}"]
        assert val.shape == rv.shape and ind.shape == ri.shape
        live = rv > 0                     # torch.topk orders the zeroed entries arbitrarily
        assert np.array_equal(val > 0, live)
        assert np.array_equal(ind[live], ri[live])
        assert np.array_equal(val[live].view(np.uint32), rv[live].view(np.uint32))
        assert np.array_equal(a[live], g[f"{case}.src_corr{b}"][live])
        assert np.array_equal(bb[live], g[f"{case}.tgt_corr{b}"][live])
        err = np.linalg.norm(pose - g[f"{case}.pose"][b].astype(np.float64))
        assert err < POSE_BOUND, f"{case} pair {b}: {err:.2e}"


def test_golden_inputs_keep_their_gaps():
    """What the generator asserted, re-checked on the committed file: no ratio within 1e-5 of lowe_thres, no LGR
    residual within 1e-4 (relative) of the radius."""
    g = load_golden("refine_ops.npz")
    for case in ("ratio", "lgr", "all"):
        for b in range(int(g["B"])):
            tr = {}
            replica_case(g, case, b, trace=tr)
            if "ratios" in tr:
                r = tr["ratios"][np.isfinite(tr["ratios"])]
                assert np.abs(r - np.float32(g["lowe_thres"])).min() >= 1e-5
            rad = float(g["acceptance_radius"])
            for res in tr["residuals"]:
                assert (np.abs(res - rad) >= 1e-4 * rad).all()


def test_library_exports_the_refine_symbols():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("spr_refine_pairs", "spr_refine_pairs_workspace_bytes"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    L = _lib.lib()
    assert L.spr_refine_pairs_workspace_bytes(4, 4096) == 0          # the LDS path needs no scratch
    assert L.spr_refine_pairs_workspace_bytes(4, 4100) >= 4 * 4100 * 20
    assert L.spr_refine_pairs_workspace_bytes(4, ops.REFINE_MAX_N + 1) == 0
    # host-side refusals, before any HIP call
    rc = L.spr_refine_pairs(None, None, None, None, None, None, 1, 0, None, None, 0, 0.0, 0.0, 0, None, 0, None, None,
                            None, None, None, None, None, 0, None)
    assert rc != 0 and b"refine_pairs" in L.spr_last_error()


def test_refine_pairs_rejects_cpu_tensors_and_mismatched_lengths():
    n, m = 5, 7
    val, ind = torch.rand(n + m), torch.zeros(n + m, dtype=torch.int32)
    ov, xyz = torch.rand(n + m), torch.rand(n + m, 3)
    cu = torch.tensor([0, n, n + m], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.refine_pairs(val, None, ind, ov, xyz, cu, [0, n, n + m], 1)
    with pytest.raises(ValueError, match="cu_host"):
        ops.refine_pairs(val, None, ind, ov, xyz, cu, [0, n, n + m], 2)          # 2 pairs need 5 prefix entries
    with pytest.raises(ValueError, match="k "):
        ops.refine_pairs(val, None, ind, ov, xyz, cu, [0, n, n + m], 1, k=[n + 1])   # more than min(N, M)
    with pytest.raises(ValueError, match="k "):
        ops.refine_pairs(val, None, ind, ov, xyz, cu, [0, n, n + m], 1, k=[1, 1])
    with pytest.raises(ValueError, match="overlap_prune"):
        ops.refine_pairs(val, None, ind, ov, xyz, cu, [0, n, n + m], 1, overlap_as_weights=True)
    with pytest.raises(ValueError, match="val2"):
        ops.refine_pairs(val, None, ind, ov, xyz, cu, [0, n, n + m], 1, ratio=True)
    with pytest.raises(ValueError, match="cap"):
        big = ops.REFINE_MAX_N + 1
        ops.refine_pairs(val, None, ind, ov, xyz, cu, [0, big, 2 * big], 1)
