"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/refine_ops.npz by running the reference's
RegTR.softmax_correlation (models/qk_regtr_full.py:423-672, loaded through oracle.ref_harness) on the CPU for every
switch set of oracle.gen_golden.REFINE_CASES.  Run from the repo root in the dev container:

    python scripts/gen_refine_golden.py

Inputs are small and synthetic: one batch of 3 pairs with (N, M) = (37, 52), (64, 64), (130, 90) -- own side src, the
tie, own side tgt -- 32-wide features, KITTI-scale points and random overlap scores.  Most tgt points are a rigidly
moved src point with a near-copy of its feature (clean matches); some carry a matching feature but sit metres away
(LGR has something to reject); the rest are clutter.

Stored: the inputs; the matching head's own-side top-2 of the reference's dual-softmax matrix (val_in / val2_in /
ind_in: what spr_refine_pairs is handed); per case and pair the reference's val, ind, src_corr, tgt_corr and pose.
(use_sinkhorn with remove_points_from_val is not here: the reference itself cannot run it -- its Sinkhorn solve
multiplies the [N, M] matrix with the k pruned points, utils/se3_torch.py:218.)

Discrete choices flip on a last-bit difference, so the float64 replica (tests/refine_replica.py) is run beside the
reference and the inputs are accepted only if it keeps a gap at every one of them (asserted below):
  every Lowe ratio                            >= 1e-3 from lowe_thres                        (required: 1e-5)
  every LGR residual      >= 1e-3 (relative) from acceptance_radius      (required: 1e-4), at every refinement step,
                          and at least 8 correspondences inside the radius (a well-posed solve)
  the median              >= 3e-3 (relative) from its live neighbours in the sorted values
  the k-th largest value  >= 3e-3 (relative) from the (k+1)-th, where both are > 0
The gaps are wider than required because the GPU matching head's values agree with the reference's to a few 1e-3
relative (the tolerance of the existing golden test): the selections must come out the same from either.  The script prints the replica's pose distance from the reference per case: the bound the CPU test uses.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import ref_harness  # noqa: E402
from oracle.gen_golden import REFINE_CASES  # noqa: E402
import refine_replica  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
SIZES = ((37, 52), (64, 64), (130, 90))
D = 32
RATIO_GAP, RADIUS_GAP, ORDER_GAP = 1e-3, 1e-3, 3e-3
REPLICA_KW = {"use_ratio_test": "ratio", "threshold_corr": "median", "remove_outliers_overlap": "overlap",
              "use_overlap_as_weights": "overlap_w"}


def rot(axis, deg):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    a = np.deg2rad(deg)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def make_inputs(seed):
    rng = np.random.default_rng(seed)
    pairs = []
    for b, (n, m) in enumerate(SIZES):
        R, t = rot(rng.standard_normal(3), 8.0 + 3 * b), rng.uniform(-1.5, 1.5, 3)
        src = rng.uniform(-12, 12, (n, 3))
        fs = 1.0 * rng.standard_normal((n, D))
        tgt = rng.uniform(-12, 12, (m, 3))                         # clutter
        ft = 1.0 * rng.standard_normal((m, D))
        c = min(n, m)
        pick = rng.permutation(n)[:c]
        n_clean, n_far = int(0.7 * c), int(0.1 * c)
        rows = rng.permutation(m)[:n_clean + n_far]
        moved = src[pick] @ R.T + t
        tgt[rows[:n_clean]] = moved[:n_clean] + rng.normal(0, 0.03, (n_clean, 3))
        tgt[rows[n_clean:]] = moved[n_clean:n_clean + n_far] + rng.uniform(1.5, 3.0, (n_far, 3))   # right feature, wrong place
        ft[rows] = fs[pick[:n_clean + n_far]] + rng.normal(0, 0.2, (n_clean + n_far, D))
        pairs.append(dict(src=src.astype(np.float32), tgt=tgt.astype(np.float32), fs=fs.astype(np.float32),
                          ft=ft.astype(np.float32), ov_s=rng.uniform(0.05, 1.0, n).astype(np.float32),
                          ov_t=rng.uniform(0.05, 1.0, m).astype(np.float32)))
    return pairs


def own_top2(attn, n, m):
    """The own side's best / runner-up of the reference's [1, N, M] matrix (torch.topk, as ratio_test does)."""
    v, i = torch.topk(attn, 2, dim=1 if n > m else 2)
    if n > m:
        return v[0, 0].numpy(), v[0, 1].numpy(), i[0, 0].numpy().astype(np.int32)
    return v[0, :, 0].numpy(), v[0, :, 1].numpy(), i[0, :, 0].numpy().astype(np.int32)


def gaps_ok(cfg, flags, p, head, k):
    tr = {}
    kw = {REPLICA_KW[f]: True for f in flags if f in REPLICA_KW}
    out = refine_replica.refine_pair(*head, p["ov_s"], p["ov_t"], p["src"], p["tgt"], k=k,
                                     lgr_steps=int(cfg.num_refinement_steps) if flags.get("use_lgr") else 0,
                                     lowe_thres=cfg.lowe_thres, radius=cfg.acceptance_radius, trace=tr, **kw)
    ok = True
    if "ratios" in tr:
        r = tr["ratios"][np.isfinite(tr["ratios"])]
        ok &= bool(np.abs(r - np.float32(cfg.lowe_thres)).min() >= RATIO_GAP)
    for res in tr["residuals"]:
        ok &= bool((np.abs(res - cfg.acceptance_radius) >= RADIUS_GAP * cfg.acceptance_radius).all())
        ok &= int((res < cfg.acceptance_radius).sum()) >= 8          # a well-posed solve at every step
    if "median" in tr:
        med, srt = tr["median"]
        live = srt[(srt != med) & (srt > 0)].astype(np.float64)
        ok &= med > 0 and bool((np.abs(live - med) >= ORDER_GAP * med).all())
    if "topk" in tr:
        v, order = tr["topk"]
        srt = -np.sort(-v.astype(np.float64))
        if k < len(srt) and srt[k] > 0:
            ok &= bool(srt[k - 1] - srt[k] >= ORDER_GAP * srt[k - 1])
    return ok, out


def main():
    ns = ref_harness.load_regtr()
    model, cfg = ref_harness.make_model("qk_regtr_full_kitti.yaml", seed=0)
    del ns
    for seed in range(200):
        pairs = make_inputs(seed)
        fx = {"B": np.int32(len(SIZES)), "seed": np.int32(seed), "lowe_thres": np.float64(cfg.lowe_thres),
              "acceptance_radius": np.float64(cfg.acceptance_radius), "val_threshold": np.float64(cfg.val_threshold),
              "num_refinement_steps": np.int32(cfg.num_refinement_steps), "cases": np.array(list(REFINE_CASES))}
        args = ([torch.from_numpy(p["fs"])[None] for p in pairs], [torch.from_numpy(p["ft"])[None] for p in pairs],
                [torch.from_numpy(p["src"]) for p in pairs], [torch.from_numpy(p["tgt"]) for p in pairs],
                [torch.from_numpy(p["ov_s"])[None, :, None] for p in pairs],
                [torch.from_numpy(p["ov_t"])[None, :, None] for p in pairs])
        good, worst = True, {}
        for case, flags in REFINE_CASES.items():
            for f in ("use_lgr", "use_ransac", "use_ratio_test", "threshold_corr", "remove_outliers_overlap",
                      "use_overlap_as_weights", "remove_points_from_val"):
                model.cfg[f] = bool(flags.get(f, False))
            with torch.no_grad():
                pose, attn, vals, inds, s_pts, t_pts = model.softmax_correlation(*args)
            for b, p in enumerate(pairs):
                n, m = SIZES[b]
                head = own_top2(attn[b], n, m)
                fx[f"val_in{b}"], fx[f"val2_in{b}"], fx[f"ind_in{b}"] = head
                k = int(cfg.val_threshold * min(n, m)) if flags.get("remove_points_from_val") else None
                ok, rep = gaps_ok(cfg, flags, p, head, k)
                good &= ok
                fx[f"{case}.val{b}"] = vals[b].numpy()
                fx[f"{case}.ind{b}"] = inds[b].numpy().astype(np.int32)
                fx[f"{case}.src_corr{b}"] = s_pts[b].numpy()
                fx[f"{case}.tgt_corr{b}"] = t_pts[b].numpy()
                worst[case] = max(worst.get(case, 0.0), float(np.linalg.norm(rep[0] - pose[b].double().numpy())))
            fx[f"{case}.pose"] = pose.numpy()
        if good:
            break
    else:
        raise SystemExit("no seed keeps the gaps")
    for b, p in enumerate(pairs):
        for key, arr in p.items():
            fx[f"{key}{b}"] = arr
    fx["replica_pose_dist"] = np.array([worst[c] for c in REFINE_CASES])
    path = os.path.join(OUT, "refine_ops.npz")
    np.savez_compressed(path, **fx)
    print("seed", seed, os.path.basename(path), os.path.getsize(path) // 1024, "KB")
    for c in REFINE_CASES:
        print(f"  {c:10s} replica (f64) vs reference (f32) pose distance {worst[c]:.3e}")


if __name__ == "__main__":
    main()
