"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/calibrate.npz: the histograms and limits the reference's
calibrate_neighbors procedure (kpconv.py:714-747) gives on six small synthetic pairs under the 3DMatch geometry.
Run from the repo root:

    python scripts/gen_calibrate_golden.py

The rows come from the compiled reference core (oracle/_ref: ref_radius_neighbors / ref_grid_subsample) where it
was built, from the CPU oracle otherwise; the file records which (`source`).  samples_threshold is set between the
smallest level total after the third and after the fourth pair, so the reference's stop rule ends the loop after
the fourth.  The file holds the inputs, the settings and the recorded results, nothing else.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import calibrate_cases as cc  # noqa: E402
from oracle import native  # noqa: E402

KEEP_RATIO = 0.8


def main():
    cfg = cc.golden_config()
    data = cc.golden_dataset()
    source = "reference" if native.ref_available() else "oracle"
    per_sample = [cc.sample_hists(it, cfg, source) for it in data]
    totals = np.cumsum(np.stack([h.sum(1) for h in per_sample]), axis=0).min(1)      # smallest level total after sample i
    lo, hi = int(totals[cc.GOLDEN_STOP - 2]), int(totals[cc.GOLDEN_STOP - 1])
    assert lo < hi - 1, (lo, hi)
    threshold = (lo + hi) // 2
    limits, hists, used = cc.replica(data, cfg, KEEP_RATIO, threshold, per_sample=per_sample)
    assert used == cc.GOLDEN_STOP, used
    level0 = np.repeat(np.arange(hists.shape[1]), hists[0])
    print(f"source {source}; threshold {threshold} (level totals after 3 / 4 pairs: {lo} / {hi}); limits {limits.tolist()}")
    print(f"level-0 counts: 2 % {np.percentile(level0, 2):.0f}, median {np.median(level0):.0f}, "
          f"98 % {np.percentile(level0, 98):.0f}; level totals {hists.sum(1).tolist()}")
    out = {"source": np.array(source), "keep_ratio": np.float64(KEEP_RATIO), "samples_threshold": np.int64(threshold),
           "hist_n": np.int64(hists.shape[1]), "hists": hists.astype(np.int64), "limits": np.asarray(limits, np.int64),
           "samples_used": np.int64(used), "per_sample": np.stack(per_sample).astype(np.int32)}
    for k, it in enumerate(data):
        out[f"pair{k}.src_xyz"], out[f"pair{k}.tgt_xyz"] = it["src_xyz"], it["tgt_xyz"]
    np.savez_compressed(cc.GOLDEN, **out)
    print(f"wrote {cc.GOLDEN} ({os.path.getsize(cc.GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
