"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/augment_ops.npz by running the reference's four training
transforms (data_loaders/transforms.py: RigidPerturb, Jitter, ShufflePoints, RandomSwap) on a few small labelled pairs.
Run from the repo root in the dev container (the reference tree must be present):

    python scripts/gen_augment_golden.py <path to the reference's src directory>

The transforms draw from the global numpy / random / torch generators; here np.random.permutation, torch.randn,
random.random and RigidPerturb._sample_pose_{small,large} are patched to return recorded draws, so the file holds
inputs, draws and the reference's outputs, and nothing else (data only).  Coordinates are multiples of 2^-12 below
2^10 in magnitude: the float64 centroid sum of the contract (include/spr.h, "8f-6") is then exact in any order.
data_loaders/__init__.py is not imported (it needs h5py / torchvision); transforms.py is loaded by file path.
"""
import importlib.util
import os
import random
import sys
from unittest import mock

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from superpoints_registration_amd import ops, synthetic  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "augment_ops.npz")
MAX_PTS = 40

# name -> (mode, perturb source?, swap?, n_src, n_tgt, n_corr, jitter scale)
CASES = {
    "small_src": ("small", True, False, 33, 37, 0, 0.005),        # no correspondences at all
    "small_tgt_swap": ("small", False, True, 36, 29, 20, 0.005),
    "large_src_swap": ("large", True, True, 52, 31, 25, 0.01),    # source longer than max_pts: points are cut
    "large_tgt": ("large", False, False, 30, 47, 25, 0.01),       # target longer than max_pts
}


def load_transforms(ref_src):
    sys.path.insert(0, ref_src)
    spec = importlib.util.spec_from_file_location("ref_transforms", os.path.join(ref_src, "data_loaders", "transforms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def quantise(x):
    return (np.round(np.asarray(x, np.float64) * 4096.0) / 4096.0).astype(np.float32)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_src = sys.argv[1]
    T = load_transforms(ref_src)
    out = {"max_pts": np.int64(MAX_PTS), "cases": np.array(sorted(CASES))}
    for ci, name in enumerate(sorted(CASES)):
        mode, psrc, swap, n_s, n_t, n_c, scale = CASES[name]
        rng = np.random.default_rng(100 + ci)
        src, tgt, pose = synthetic.make_pair(max(n_s, n_t), seed=200 + ci, extent=3.0)
        src, tgt = quantise(src[:n_s] + 5.0), quantise(tgt[:n_t] + 5.0)    # off-centre: the centring matters
        src_ov, tgt_ov = rng.random(n_s) > 0.4, rng.random(n_t) > 0.4
        corr = np.stack([rng.integers(0, n_s, n_c), rng.integers(0, n_t, n_c)]).astype(np.int64)
        # recorded draws: the perturbation comes from this project's own decision draw (a proper float32 rotation)
        _, _, P = ops.augment_draw(900 + ci, [ci], mode)
        P = P[0]
        noise_s = rng.standard_normal((n_s, 3)).astype(np.float32)
        noise_t = rng.standard_normal((n_t, 3)).astype(np.float32)
        perm_s, perm_t = rng.permutation(n_s), rng.permutation(n_t)
        data = {"src_xyz": torch.from_numpy(src.copy()), "tgt_xyz": torch.from_numpy(tgt.copy()),
                "pose": torch.from_numpy(pose.copy()), "src_overlap": torch.from_numpy(src_ov.copy()),
                "tgt_overlap": torch.from_numpy(tgt_ov.copy()), "correspondences": torch.from_numpy(corr.copy()),
                "src_path": "s", "tgt_path": "t"}
        sample = staticmethod(lambda *a, **k: torch.from_numpy(P.copy()).float())
        with mock.patch.object(T.RigidPerturb, "_sample_pose_small", sample), \
                mock.patch.object(T.RigidPerturb, "_sample_pose_large", sample), \
                mock.patch.object(random, "random", side_effect=[0.75 if psrc else 0.25, 0.75 if swap else 0.25]), \
                mock.patch.object(torch, "randn", side_effect=[torch.from_numpy(noise_s), torch.from_numpy(noise_t)]), \
                mock.patch.object(np.random, "permutation", side_effect=[perm_s.copy(), perm_t.copy()]):
            for tr in (T.RigidPerturb(mode), T.Jitter(scale), T.ShufflePoints(max_pts=MAX_PTS), T.RandomSwap()):
                data = tr(data)
        assert (data["src_path"], data["tgt_path"]) == (("t", "s") if swap else ("s", "t"))
        p = f"{name}."
        out.update({
            p + "mode": np.array(mode), p + "perturb_src": np.bool_(psrc), p + "swap": np.bool_(swap),
            p + "scale": np.float64(scale), p + "src": src, p + "tgt": tgt, p + "pose": pose,
            p + "src_overlap": src_ov, p + "tgt_overlap": tgt_ov, p + "corr": corr, p + "perturb": P,
            p + "noise_src": noise_s, p + "noise_tgt": noise_t, p + "perm_src": perm_s.astype(np.int64),
            p + "perm_tgt": perm_t.astype(np.int64),
            p + "ref_src": data["src_xyz"].numpy().astype(np.float32),
            p + "ref_tgt": data["tgt_xyz"].numpy().astype(np.float32),
            p + "ref_pose": data["pose"].numpy().astype(np.float32),
            p + "ref_src_overlap": data["src_overlap"].numpy(), p + "ref_tgt_overlap": data["tgt_overlap"].numpy(),
            p + "ref_corr": data["correspondences"].numpy().astype(np.int64),
        })
        print(name, {k: tuple(v.shape) for k, v in data.items() if hasattr(v, "shape")})
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
