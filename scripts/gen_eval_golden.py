"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/eval_modelnet.npz by running the reference's ModelNet evaluation
(benchmark/benchmark_modelnet.py: compute_metrics at batch size 1 -- the only batch size at which it is right --
summarize_metrics and print_metrics) on a few small pairs.  Run from the repo root in the dev container (the reference
tree must be present):

    python scripts/gen_eval_golden.py <path to the reference's src directory>

benchmark_modelnet.py is loaded by file path with the reference's src directory on sys.path (it imports
cvhelpers.torch_helpers and utils.se3_torch from there).  The file holds inputs, the reference's per-pair outputs, its
summary and the lines it logs, and nothing else (data only).

Cases: clouds of 1 to 120 points, ground-truth rotations up to 45 degrees, predicted poses 1 to 5 degrees and at most
0.05 away from the ground truth, every |R20| <= 0.99 (no gimbal lock: there the closed form of the contract and
scipy's as_euler part ways).  The script asserts these conditions.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import eval_cases as C  # noqa: E402
import eval_replica as R  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "eval_modelnet.npz")
SIZES = [(1, 1, 1), (2, 3, 5), (17, 9, 33), (64, 64, 120), (120, 120, 120), (100, 37, 64), (5, 120, 77), (33, 1, 2),
         (90, 80, 70), (12, 12, 12), (120, 1, 120), (50, 60, 100)]
KEYS = ('r_mse', 'r_mae', 't_mse', 't_mae', 'err_r_deg', 'err_t', 'chamfer_dist')


def load_benchmark(ref_src):
    sys.path.insert(0, ref_src)
    spec = importlib.util.spec_from_file_location("ref_benchmark_modelnet",
                                                  os.path.join(ref_src, "benchmark", "benchmark_modelnet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Lines:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(str(msg))


def angle_deg(rot):
    return float(np.degrees(np.arccos(np.clip(0.5 * (np.trace(rot) - 1.0), -1.0, 1.0))))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    bm = load_benchmark(sys.argv[1])
    case = C._sized(SIZES, 20241021)
    gt32, pred32 = case["gt"].astype(np.float32), case["pred"].astype(np.float32)
    per_pair = {k: [] for k in KEYS}
    for b, (ns, nt, nr) in enumerate(SIZES):
        assert all(1 <= n <= 120 for n in (ns, nt, nr))
        g, p = gt32[b].astype(np.float64), pred32[b].astype(np.float64)
        delta = R.compose(p, R.inverse(g))
        assert angle_deg(g[:, :3]) <= 45.0 and 1.0 <= angle_deg(delta[:, :3]) <= 5.0, b
        assert float(np.linalg.norm(delta[:, 3])) <= 0.05, b                 # the translation of pred o gt^-1
        assert abs(g[2, 0]) <= 0.99 and abs(p[2, 0]) <= 0.99, b
        data = {'points_src': torch.from_numpy(case["src"][b])[None], 'points_ref': torch.from_numpy(case["ref"][b])[None],
                'points_raw': torch.from_numpy(case["raw"][b])[None], 'transform_gt': torch.from_numpy(gt32[b])[None]}
        m = bm.compute_metrics(data, torch.from_numpy(pred32[b]))
        for k in KEYS:
            v = np.asarray(m[k])
            assert v.shape == (1,), (k, v.shape)
            per_pair[k].append(v)
    metrics_cat = {k: np.concatenate(per_pair[k]) for k in KEYS}      # test_epoch_end: concatenate, then summarise
    summary = bm.summarize_metrics(metrics_cat)
    log = Lines()
    bm.print_metrics(log, summary)
    out = {"n": np.int64(len(SIZES)), "gt": gt32, "pred": pred32, "log": np.array(log.lines)}
    for b in range(len(SIZES)):
        out[f"src.{b}"], out[f"ref.{b}"], out[f"raw.{b}"] = case["src"][b], case["ref"][b], case["raw"][b]
    for k in KEYS:
        out["ref_" + k] = metrics_cat[k]
    out["summary_keys"] = np.array(sorted(summary))
    out["summary_values"] = np.array([float(summary[k]) for k in sorted(summary)], dtype=np.float64)
    np.savez_compressed(OUT, **out)
    print("\n".join(log.lines))
    print({k: str(v.dtype) for k, v in metrics_cat.items()})
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
