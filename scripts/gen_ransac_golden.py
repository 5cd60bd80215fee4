"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/ransac_ops.npz by running the reference's own RegTR.ransac
(models/qk_regtr_full.py:400-421, loaded through oracle.ref_harness) on the CPU.  Run from the repo root in the dev
container:

    python scripts/gen_ransac_golden.py

The reference's loop moves its draws to the device with `.cuda()`; for the duration of the call torch.Tensor.cuda is
the identity.  torch.randint and the module's compute_rigid_transform / se3_transform are wrapped so that every draw,
every hypothesis pose and every loss is recorded (the loss is the reference's expression,
torch.linalg.norm(tgt - src_tf, dim=1).mean(), evaluated on the src_tf the reference itself computed; the script
asserts that the first minimum of the recorded losses is the pose the reference returned).

Inputs: three sets of n = 37, 64, 130 correspondences (every index fits uint8): KITTI-scale points under a planted
rigid transform with 0.2 % noise, 10 % gross outliers, weights in [0.05, 1].  500 hypotheses of 100 samples, the
reference's literals.

The pick flips on a last-bit difference of two scores, and an ill-conditioned sample has no stable pose, so the float64
replica (tests/ransac_replica.py) is run beside the reference and a seed is accepted only if, for every set,
  the best score is >= 1e-4 (relative) below the runner-up, and
  >= 90 % of the hypotheses are well-posed (second singular value of the covariance >= 1e-3 of the first).
Both are asserted, printed and stored (gap [3], well_posed_frac [3]).
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
import ransac_replica  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
SIZES = (37, 64, 130)
N_HYP, SAMPLE = 500, 100
MIN_GAP, MIN_WELL_POSED = 1e-4, 0.9


def rot(axis, deg):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    a = np.deg2rad(deg)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def make_inputs(seed):
    rng = np.random.default_rng(seed)
    sets = []
    for b, n in enumerate(SIZES):
        R, t = rot(rng.standard_normal(3), 8.0 + 3 * b), rng.uniform(-1.5, 1.5, 3)
        src = rng.uniform(-12, 12, (n, 3))
        tgt = src @ R.T + t + rng.normal(0, 0.002 * 12, (n, 3))            # 0.2 % of the extent
        bad = rng.permutation(n)[:max(1, n // 10)]                          # 10 % gross outliers
        tgt[bad] += rng.uniform(1.5, 3.0, (len(bad), 3)) * rng.choice([-1.0, 1.0], (len(bad), 3))
        sets.append(dict(src=src.astype(np.float32), tgt=tgt.astype(np.float32),
                         w=rng.uniform(0.05, 1.0, n).astype(np.float32),
                         planted=np.concatenate([R, t[:, None]], axis=1).astype(np.float32)))
    return sets


def run_reference(mod, src, tgt, w):
    """The reference's ransac() on CPU tensors -> (returned pose, idx [H,S], poses [H,3,4], losses [H])."""
    rec = {'idx': [], 'pose': [], 'loss': []}
    tgt_t = torch.from_numpy(tgt)
    real_randint, real_crt, real_tf, real_cuda = torch.randint, mod.compute_rigid_transform, mod.se3_transform, \
        torch.Tensor.cuda

    def randint(*a, **k):
        out = real_randint(*a, **k)
        rec['idx'].append(out.numpy().copy())
        return out

    def crt(*a, **k):
        out = real_crt(*a, **k)
        rec['pose'].append(out.numpy().copy())
        return out

    def tf(pose, xyz):
        out = real_tf(pose, xyz)
        rec['loss'].append(torch.linalg.norm(tgt_t - out, dim=1).mean().numpy().copy())
        return out

    torch.randint, mod.compute_rigid_transform, mod.se3_transform = randint, crt, tf
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        with torch.no_grad():
            T = mod.RegTR.ransac(None, torch.from_numpy(src), tgt_t, torch.from_numpy(w))
    finally:
        torch.randint, mod.compute_rigid_transform, mod.se3_transform = real_randint, real_crt, real_tf
        torch.Tensor.cuda = real_cuda
    idx, poses, losses = np.stack(rec['idx']), np.stack(rec['pose']), np.stack(rec['loss'])
    assert idx.shape == (N_HYP, SAMPLE) and poses.shape == (N_HYP, 3, 4) and losses.shape == (N_HYP,)
    assert np.array_equal(T.numpy(), poses[ransac_replica.pick(losses)]), "the recorded losses do not explain the pick"
    return T.numpy(), idx, poses, losses


def main():
    mod = ref_harness.load_regtr()["regtr"]
    for seed in range(200):
        sets = make_inputs(seed)
        torch.manual_seed(seed)
        fx = {"B": np.int32(len(SIZES)), "seed": np.int32(seed), "n_hyp": np.int32(N_HYP), "sample": np.int32(SAMPLE)}
        gaps, fracs, good = [], [], True
        for b, s in enumerate(sets):
            T, idx, poses, losses = run_reference(mod, s["src"], s["tgt"], s["w"])
            rep = ransac_replica.ransac_pair(s["src"], s["tgt"], s["w"], idx)
            gaps.append(ransac_replica.gap(rep["score"])[1])
            fracs.append(float(ransac_replica.well_posed(rep["sv"]).mean()))
            good &= gaps[-1] >= MIN_GAP and fracs[-1] >= MIN_WELL_POSED and rep["best"] == ransac_replica.pick(losses)
            assert idx.max() < 256
            fx.update({f"src{b}": s["src"], f"tgt{b}": s["tgt"], f"w{b}": s["w"], f"planted{b}": s["planted"],
                       f"idx{b}": idx.astype(np.uint8), f"hyp_pose{b}": poses, f"loss{b}": losses.astype(np.float32),
                       f"pose{b}": T, f"best{b}": np.int32(ransac_replica.pick(losses))})
        if good:
            break
    else:
        raise SystemExit("no seed keeps the gaps")
    assert min(gaps) >= MIN_GAP and min(fracs) >= MIN_WELL_POSED
    fx["gap"], fx["well_posed_frac"] = np.asarray(gaps), np.asarray(fracs)
    path = os.path.join(OUT, "ransac_ops.npz")
    np.savez_compressed(path, **fx)
    print("seed", seed, os.path.basename(path), os.path.getsize(path) // 1024, "KB")
    for b, n in enumerate(SIZES):
        print(f"  n = {n:3d}: best-to-runner-up gap {gaps[b]:.3e} (relative), well-posed {fracs[b]:.3f}, "
              f"reference pick {int(fx[f'best{b}'])}")


if __name__ == "__main__":
    main()
