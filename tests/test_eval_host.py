"""CPU: what the evaluation tests rest on, and what the `evaluation` subpackage does on the host.

The replica (tests/eval_replica.py: the contract of spr_eval_pairs in numpy float64) is held to the reference's own
outputs (tests/golden/eval_modelnet.npz, written by scripts/gen_eval_golden.py from benchmark_modelnet.compute_metrics
at batch size 1).  Tolerances, from the reference's float32 arithmetic (measured over 200 random cases of the
fixture's kind: worst 1.9e-6 relative, and 1.8e-4 degrees near 3 degrees):
  r_mse, r_mae, t_mse, t_mae, err_t, chamfer_dist   relative 2e-5 with a floor of 1e-9: ten times the worst seen
  err_r_deg                                         4e-6 / sin(err) radians: the reference takes a float32 acos of a
                                                    trace that carries about 2^-22 of error
summarize_metrics / format_metrics reproduce the recorded summary (1e-12) and the recorded log lines (exactly) when fed
the reference's own per-pair values.  Evaluator's arithmetic is checked on canned per-pair tables, and every host
refusal must come before any library call."""
import math
import os
import re

import numpy as np
import pytest
import torch

import eval_cases as C
import eval_replica as R
from conftest import REPO, load_golden
from superpoints_registration_amd import _lib, evaluation as E, get_config
from test_workspace_sizes_host import HUGE, sweep_points

KEYS = E.MODELNET_KEYS


def fixture_pairs():
    g = load_golden("eval_modelnet.npz")
    n = int(g["n"])
    return g, [(g[f"src.{b}"], g[f"ref.{b}"], g[f"raw.{b}"], g["gt"][b], g["pred"][b]) for b in range(n)]


def check_against_fixture(g, got, what):
    """got: dict key -> [n] float64.  The tolerances of the module docstring."""
    for k in KEYS:
        ref = g["ref_" + k].astype(np.float64)
        for b, (x, r) in enumerate(zip(got[k], ref)):
            if k == "err_r_deg":
                bound = math.degrees(4e-6 / math.sin(math.radians(r)))
            else:
                bound = max(2e-5 * abs(r), 1e-9)
            print(f"{what} {k}[{b}]: {x:.9g} vs the reference's {r:.9g}, bound {bound:.3g}")
            assert abs(x - r) <= bound, (what, k, b, x, r, bound)


def test_replica_matches_the_reference():
    g, pairs = fixture_pairs()
    out = [R.eval_pair(s, t, gt, pr, raw) for s, t, raw, gt, pr in pairs]
    assert all(o["status"] == 0 for o in out)
    check_against_fixture(g, {k: np.array([o[k] for o in out]) for k in KEYS}, "replica")


def test_fixture_holds_data_only_and_stays_in_its_range():
    g, pairs = fixture_pairs()
    assert all(v.dtype.kind in "fiU" for v in g.values())
    for s, t, raw, gt, pr in pairs:
        assert all(1 <= len(x) <= 120 for x in (s, t, raw))
        assert abs(gt[2, 0]) <= 0.99 and abs(pr[2, 0]) <= 0.99


def test_summary_and_log_lines_are_the_reference_s():
    g, _ = fixture_pairs()
    per_pair = {k: g["ref_" + k] for k in KEYS}                           # the reference's own values and dtypes
    s = E.summarize_metrics(per_pair)
    assert sorted(s) == list(g["summary_keys"])
    for k, v in zip(g["summary_keys"], g["summary_values"]):
        assert abs(float(s[k]) - v) <= 1e-12 * abs(v), k
    lines = [str(x) for x in g["log"]]
    assert lines[:2] == ["Metrics:", "========"] and E.format_metrics(s) == lines[2:] and len(lines) == 6


def test_summarize_rule_key_for_key():
    m = {"t_mse": np.array([1.0, 3.0]), "err_t": np.array([3.0, 4.0]), "t_mae": np.array([1.0, 2.0]),
         "chamfer_dist": torch.tensor([2.0, 4.0], dtype=torch.float64)}
    s = E.summarize_metrics(m)
    assert s == {"t_rmse": math.sqrt(2.0), "err_t_mean": 3.5, "err_t_rmse": math.sqrt(12.5), "t_mae": 1.5,
                 "chamfer_dist": 3.0}


def test_replica_edge_rules():
    b, = C.replica("boundary")
    assert b["inlier_count"] == 1.0 and b["inlier_ratio"] == 0.25          # d2 == radius^2 is no inlier (strict)
    for r, raw in zip(C.replica("ties"), C.case("ties")["raw"]):
        n = len(raw) // 2
        assert int(r["nn_src"].max()) < n and int(r["nn_ref"].max()) < n   # the lower of j and j + n
    assert [r["status"] for r in C.replica("emptyraw")] == [0, -2, 0]
    e = C.replica("emptyraw")[1]
    assert e["chamfer_dist"] == 0.0 and e["err_t"] > 0.0 and set(e["nn_src"]) == {-1}
    assert [r["status"] for r in C.replica("nonfinite")] == [0, -1, 0]
    s0, s1 = C.replica("same")
    assert all(s0[k] == 0.0 for k in R.COLUMNS)
    assert all(s1[k] == 0.0 for k in ("r_mse", "r_mae", "t_mse", "t_mae")) and s1["err_t"] < 1e-15
    r = C.replica("ragged")
    assert r[0]["chamfer_src"] == 0.0 and r[0]["chamfer_ref"] > 0.0 and r[3]["chamfer_ref"] == 0.0
    assert r[1]["inlier_ratio"] == 0.0 and 0 < r[2]["inlier_count"] < 300


def test_trans_err_and_err_r_deg_are_se3_compare_s():
    from superpoints_registration_amd.se3 import se3_compare
    c = C.case("tiles")
    cmp = se3_compare(torch.from_numpy(c["pred"]), torch.from_numpy(c["gt"]))
    for b, r in enumerate(C.replica("tiles")):
        assert abs(float(cmp["trans"][b]) - r["trans_err"]) <= 1e-12
        assert abs(float(cmp["rot_deg"][b]) - r["err_r_deg"]) <= 1e-9


def test_tile_constants_are_the_header_s():
    hdr = open(os.path.join(REPO, "include", "spr.h")).read()
    val = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", hdr).group(1))
    assert (E.TILE, E.QUERIES, len(E.COLUMNS)) == (val("SPR_EVAL_TILE"), val("SPR_EVAL_QUERIES"), val("SPR_EVAL_COLS"))
    assert E.COLUMNS == R.COLUMNS


def test_size_query_is_monotone_and_never_huge():
    fn = _lib.lib().spr_eval_pairs_workspace_size
    base, limits = [1000, 1000, 1000, 100, 3], [1 << 24, 1 << 24, 1 << 24, 1 << 24, 32767]
    for i, limit in enumerate(limits):
        prev = None
        for v in sweep_points(limit):
            args = list(base)
            args[i] = v
            r = fn(*args)
            assert r < HUGE and (prev is None or r >= prev), (args, prev, r)
            prev = r
    assert fn(-1, 0, 0, 0, 1) == 0 and fn(0, 0, 0, 0, 0) > 0


def test_the_entry_point_refuses_bad_arguments_on_the_host():
    L = _lib.lib()
    tail = [None] * 6 + [None, 0, None]                                   # outputs, status, ws, ws_bytes, stream
    clouds = [None, None, 0, None, None, 0, None, None, 0, None, None, None, 0]
    assert L.spr_eval_pairs(*clouds, None, None, -1, 0.0, *tail) != 0 and b"negative" in L.spr_last_error()
    bad = list(clouds)
    bad[2] = 5
    assert L.spr_eval_pairs(*bad, None, None, 0, 0.0, *tail) != 0 and b"without pairs" in L.spr_last_error()
    bad = list(clouds)
    bad[8] = 5                                                            # raw points without raw_cu
    assert L.spr_eval_pairs(*bad, None, None, 1, 0.0, *tail) != 0 and b"without raw_cu" in L.spr_last_error()
    assert L.spr_eval_pairs(*clouds, None, None, 1, 0.0, *tail) != 0 and b"must not be null" in L.spr_last_error()


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name}) before the host refusal")


def test_host_layer_refuses_before_any_library_call(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _NoLibrary())
    x = torch.zeros((4, 3))
    eye = torch.eye(4)[None]
    with pytest.raises(ValueError, match="1 source clouds, 2 reference clouds"):
        E.eval_pairs([x], [x, x], eye, eye)
    with pytest.raises(ValueError, match="0 source clouds"):
        E.eval_pairs([], [], eye[:0], eye[:0])
    with pytest.raises(ValueError, match="1 source clouds, 2 raw clouds"):
        E.eval_pairs([x], [x], eye, eye, raw_list=[x, x])
    with pytest.raises(ValueError, match="corr must be a pair"):
        E.eval_pairs([x], [x], eye, eye, corr=[x], acceptance_radius=0.1)
    with pytest.raises(ValueError, match="correspondence sets"):
        E.eval_pairs([x], [x], eye, eye, corr=([x], [x, x]), acceptance_radius=0.1)
    for bad in (None, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="acceptance_radius"):
            E.eval_pairs([x], [x], eye, eye, corr=([x], [x]), acceptance_radius=bad)
    with pytest.raises(ValueError, match="pose_gt"):
        E.eval_pairs([x], [x], torch.eye(4), eye)                          # [4, 4]: no batch dimension
    with pytest.raises(ValueError, match="pose_pred"):
        E.eval_pairs([x], [x], eye, eye.repeat(2, 1, 1))
    with pytest.raises(ValueError, match="pose_pred is torch.int64"):
        E.eval_pairs([x], [x], eye, eye.long())
    with pytest.raises(ValueError, match=r"expected an \[n, 3\] tensor"):
        E.eval_pairs([torch.zeros((4, 4))], [x], eye, eye)
    with pytest.raises(ValueError, match=r"src_list\[0\] is torch.float64, expected float32"):
        E.eval_pairs([x.double()], [x], eye, eye, raw_list=[x])
    with pytest.raises(ValueError, match="expected the MI355X device"):
        E.eval_pairs([x], [x], eye, eye)
    with pytest.raises(ValueError, match="expected the MI355X device"):
        E.modelnet_metrics([x], [x], [x], eye, eye)
    with pytest.raises(ValueError, match="non-empty list"):
        E.inlier_ratio([], [], eye[:0], 0.1)
    with pytest.raises(ValueError, match="expected the MI355X device"):
        E.inlier_ratio([x], [x], eye, 0.1)
    with pytest.raises(ValueError, match="expected the MI355X device"):
        E.Evaluator(get_config("modelnet")).update({"src_xyz": [x], "tgt_xyz": [x], "tgt_raw": [x], "pose": eye},
                                                   {"pose": eye})


def test_feature_matching_recall_is_strict_at_tau():
    assert E.feature_matching_recall([0.05, 0.0500001, 0.04, 1.0]) == 0.5
    assert E.feature_matching_recall(np.array([0.2]), tau=0.2) == 0.0
    t = E.feature_matching_recall(torch.tensor([0.05, 0.06], dtype=torch.float64))
    assert isinstance(t, torch.Tensor) and float(t) == 0.5
    with pytest.raises(ValueError, match="no pairs"):
        E.feature_matching_recall([])


def _table(ev, rows, status=None):
    """Puts canned per-pair rows (dicts of columns) into an Evaluator, as update() would have."""
    t = np.zeros((len(rows), len(E.COLUMNS) + 13))
    for i, r in enumerate(rows):
        for k, v in r.items():
            t[i, E.COLUMNS.index(k)] = v
        t[i, len(E.COLUMNS) + 1:] = np.arange(12) + 100 * i
    if status is not None:
        t[:, len(E.COLUMNS)] = status
    ev._rows = [torch.from_numpy(t)]
    return ev


def test_evaluator_kitti_is_the_mean_over_successes():
    cfg = get_config("kitti")                                             # thresholds 5 degrees and 2 m, strict
    rows = [dict(err_r_deg=1.0, trans_err=0.5), dict(err_r_deg=5.0, trans_err=0.1), dict(err_r_deg=3.0, trans_err=2.0),
            dict(err_r_deg=2.0, trans_err=1.5), dict(err_r_deg=9.0, trans_err=9.0)]
    ev = _table(E.Evaluator(cfg), rows)
    s = ev.summary()
    assert s == {"rot_err_deg": 1.5, "trans_err": 1.0, "recall": 0.4, "n_success": 2, "n_pairs": 5}
    assert len(ev.report()) == 1 and "2 of 5 pairs" in ev.report()[0]
    none = _table(E.Evaluator(cfg), rows[-1:]).summary()
    assert math.isnan(none["rot_err_deg"]) and none["recall"] == 0.0


def test_evaluator_3dmatch_and_modelnet_tables(tmp_path):
    ev = _table(E.Evaluator(get_config("3dmatch")), [dict(inlier_ratio=v) for v in (0.05, 0.25, 0.0, 0.06)])
    s = ev.summary()
    assert s["inlier_ratio"] == pytest.approx(0.09, abs=1e-15) and s["n_pairs"] == 4
    assert s["feature_matching_recall"] == 0.5                            # 0.05 itself is not above tau
    with pytest.raises(ValueError, match="src_path"):
        ev.write_est_log(str(tmp_path), "3DMatch")
    ev._paths = [(os.path.join("d", "scene", f"cloud_bin_{i}.pth"), os.path.join("d", "scene", f"cloud_bin_{i + 1}.pth"))
                 for i in range(4)]
    ev.write_est_log(str(tmp_path), "3DMatch")
    text = open(os.path.join(str(tmp_path), "3DMatch", "scene", "est.log")).read().splitlines()
    assert len(text) == 20 and text[0] == "1\t0\t-1" and text[5] == "2\t1\t-1"
    assert text[6].split("\t") == [f"{v:.12f}" for v in (100.0, 101.0, 102.0, 103.0)]

    g, _ = fixture_pairs()
    rows = [{k: float(g["ref_" + k][b]) for k in KEYS} for b in range(int(g["n"]))]
    ev = _table(E.Evaluator(get_config("modelnet")), rows)
    s = ev.summary()
    want = E.summarize_metrics({k: g["ref_" + k].astype(np.float64) for k in KEYS})
    assert all(s[k] == want[k] for k in want) and sorted(set(s) - set(want)) == ["pred_transforms"]
    assert s["pred_transforms"].shape == (len(rows), 3, 4) and s["pred_transforms"][1, 0, 1] == 101.0
    assert ev.report() == E.format_metrics(want)
    assert np.array_equal(ev.per_pair()["err_t"], np.array([r["err_t"] for r in rows]))


def test_evaluator_edges():
    with pytest.raises(ValueError, match="no pairs"):
        E.Evaluator(get_config("kitti")).summary()
    with pytest.raises(NotImplementedError):
        E.Evaluator(type("Cfg", (), {"dataset": "other"})())
    ev = _table(E.Evaluator(get_config("kitti")), [dict(err_r_deg=1.0)] * 3, status=[0, -1, -2])
    with pytest.raises(ValueError, match=r"pair 1: a non-finite coordinate or pose, pair 2: an empty raw cloud"):
        ev.summary()
