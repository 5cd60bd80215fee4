"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/modelnet_pairs.npz by running the reference's six ModelNet training
transforms (data_loaders/modelnet_transforms.py: SplitSourceRef, RandomCrop, RandomTransformSE3_euler, Resampler,
RandomJitter, ShufflePoints) on a few small clouds.  Run from the repo root in the dev container (the reference tree
must be present):

    python scripts/gen_modelnet_pairs_golden.py <path to the reference's src directory>

The transforms draw from numpy's global generator; here np.random.uniform, choice, normal and permutation are patched
to return the draws of the contract (include/spr.h, "8f-7"; tests/modelnet_replica.py) in the order the reference asks
for them -- ShufflePoints draws the reference cloud's permutation before the source's -- and RandomCrop.crop is wrapped
to record the masks that the patched choice needs.  The file holds inputs, draws and the reference's outputs, and
nothing else (data only).  modelnet_transforms.py is loaded by file path, with np.bool aliased where numpy lacks it.

Resampler forces 717 points whenever the sample carries a two-entry crop_proportion; the cases with another k drop
that entry from the sample after the crop, which sends Resampler down its `num` branch for both clouds.

Coordinates are multiples of 2^-12 in (-1, 1): the reference's float32 mean and the contract's float64 sum are then
both exact.  The script asserts the conditions under which the reference and the contract must agree on every integer
output: frac(h) in [0.05, 0.95], no plane distance within 1e-9 of the threshold, no duplicate keys.
"""
import importlib.util
import os
import sys
from unittest import mock

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import modelnet_replica as mr  # noqa: E402
from augment_replica import block, uniform  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "modelnet_pairs.npz")
SEED, ROT_MAG, TRANS_MAG, P_KEEP, SCALE, CLIP = 20240607, 45.0, 0.5, 0.7, 0.01, 0.05

# name -> (n, k, wanted cosine between the two crop directions: None = any, else an upper bound)
CASES = {
    "down_64_32": (64, 32, None),
    "up_300_717": (300, 717, None),          # the up-sampling path with repeats
    "opposed_200_32": (200, 32, -0.97),      # nearly opposite crops: few or no correspondences
}


def load_transforms(ref_src):
    if not hasattr(np, "bool"):             # numpy 1.24 .. 1.26 dropped the alias the module uses; numpy 2 has it
        np.bool = bool
    sys.path.insert(0, ref_src)
    spec = importlib.util.spec_from_file_location("ref_modelnet_transforms",
                                                  os.path.join(ref_src, "data_loaders", "modelnet_transforms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cloud(n, rng):
    """A lumpy shell, quantised to multiples of 2^-12 inside (-1, 1)."""
    v = rng.standard_normal((n, 3))
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * (0.5 + 0.3 * rng.random((n, 1))) + 0.1
    return np.clip(np.round(v * 4096.0) / 4096.0, -0.999, 0.999).astype(np.float32)


def pick_key(limit):
    for key in range(1, 100000):
        dirs, _ = mr.decide(SEED, key, ROT_MAG, TRANS_MAG)
        if limit is None or float(dirs[0] @ dirs[1]) < limit:
            return key
    raise RuntimeError("no key found")


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    T = load_transforms(sys.argv[1])
    out = {"cases": np.array(sorted(CASES)), "seed": np.int64(SEED), "rot_mag": np.float64(ROT_MAG),
           "trans_mag": np.float64(TRANS_MAG), "p_keep": np.float64(P_KEEP), "scale": np.float64(SCALE),
           "clip": np.float64(CLIP)}
    q = mr.percentile_q(P_KEEP)
    for ci, name in enumerate(sorted(CASES)):
        n, k, limit = CASES[name]
        xyz = cloud(n, np.random.default_rng(300 + ci))
        key = pick_key(limit)
        dirs, tf = mr.decide(SEED, key, ROT_MAG, TRANS_MAG)
        rkeys = np.stack([mr.resample_keys(SEED, key, s, n) for s in range(2)])
        extra = np.stack([mr.extra_words(SEED, key, s, k) for s in range(2)])
        skeys = np.stack([mr.shuffle_keys(SEED, key, s, k) for s in range(2)])
        noise = np.stack([mr.noise64(SEED, key, s, k)[0] for s in range(2)]).astype(np.float32)
        if ci == 0:
            noise[0, 3, 1], noise[1, 5, 2] = 7.0, -7.0           # beyond the clip on both sides
        for s in range(2):
            assert np.unique(rkeys[s]).size == n and np.unique(skeys[s]).size == k, "duplicate keys"
        frac = ((n - 1) * (q / 100.0)) % 1.0
        assert 0.05 <= frac <= 0.95, frac

        # the reference's draws, in its own order
        pair_words = [block(SEED, key, s, [0], mr.TAG_PAIR)[0] for s in range(2)]
        tw = block(SEED, key, 0, [1, 2], mr.TAG_PAIR)
        uniform_q = []
        for s in range(2):
            uniform_q += [2.0 * np.pi * float(uniform(pair_words[s][0])), 2.0 * float(uniform(pair_words[s][1])) - 1.0]
        uniform_q += [float(uniform(tw[0, j])) for j in range(3)]
        uniform_q.append(np.array([-TRANS_MAG + 2.0 * TRANS_MAG * float(uniform(tw[1, j])) for j in range(3)]))
        masks, state = [], {"side": 0}

        def crop(points, p_keep, _orig=T.RandomCrop.crop):
            cropped, mask = _orig(points, p_keep)
            masks.append(mask.copy())
            return cropped, mask

        def choice(a, size, replace=True):
            s = state["side"]
            kept = np.nonzero(masks[s])[0]
            assert a == kept.size
            order = np.argsort(rkeys[s][kept], kind="stable")             # cropped-local indices
            if not replace:
                if size < a or a == k:
                    state["side"] += 1
                return order[:size]
            state["side"] += 1
            return np.floor(uniform(extra[s][:size]) * a).astype(np.int64)

        normal_q = [(noise[s].astype(np.float32) * np.float32(SCALE)).astype(np.float64) for s in range(2)]
        perm_q = [np.argsort(skeys[s], kind="stable") for s in (1, 0)]     # reference cloud first
        sample = {"points": xyz.copy(), "idx": np.int64(ci)}
        with mock.patch.object(T.RandomCrop, "crop", staticmethod(crop)), \
                mock.patch.object(np.random, "uniform", side_effect=uniform_q), \
                mock.patch.object(np.random, "choice", side_effect=choice), \
                mock.patch.object(np.random, "normal", side_effect=lambda *a, **kw: normal_q.pop(0)), \
                mock.patch.object(np.random, "permutation", side_effect=lambda m: perm_q.pop(0)):
            sample = T.SplitSourceRef()(sample)
            sample = T.RandomCrop([P_KEEP, P_KEEP])(sample)
            if k != 717:
                del sample["crop_proportion"]
            for tr in (T.RandomTransformSE3_euler(rot_mag=ROT_MAG, trans_mag=TRANS_MAG), T.Resampler(k), T.RandomJitter(),
                       T.ShufflePoints()):
                sample = tr(sample)
        assert not normal_q and not perm_q and state["side"] == 2 and len(masks) == 2

        # where the reference and the contract must agree: its own masks against the contract's distances
        want = mr.make_pair(xyz, (P_KEEP, P_KEEP), (q, q), k, SCALE, CLIP, tf, dirs, rkeys, extra, noise, skeys)
        for s in range(2):
            assert np.abs(want["d"][s] - want["thr"][s]).min() > 1e-9, "a plane distance at the threshold"
            assert np.array_equal(want["crop_masks"][s], masks[s])
        index = []
        for s, nm in enumerate(("src", "tgt")):                          # raw row of every output point, from the
            kept = np.nonzero(masks[s])[0]                               # reference's own masks and the draws it was fed
            order = kept[np.argsort(rkeys[s][kept], kind="stable")]
            sel = order[:k] if kept.size >= k else np.concatenate(
                [order, kept[np.floor(uniform(extra[s][:k - kept.size]) * kept.size).astype(np.int64)]])
            index.append(sel[np.argsort(skeys[s], kind="stable")])
        p = f"{name}."
        out.update({
            p + "key": np.int64(key), p + "k": np.int64(k), p + "xyz": xyz, p + "dirs": dirs, p + "transform": tf,
            p + "rkeys": rkeys, p + "extra": extra, p + "noise": noise, p + "skeys": skeys,
            p + "ref_crop_src": masks[0], p + "ref_crop_tgt": masks[1],
            p + "ref_src": sample["points_src"].astype(np.float32), p + "ref_tgt": sample["points_ref"].astype(np.float32),
            p + "ref_pose": sample["transform_gt"].astype(np.float32),
            p + "ref_src_overlap": sample["src_overlap"].astype(bool), p + "ref_tgt_overlap": sample["ref_overlap"].astype(bool),
            p + "ref_corr": sample["correspondences"].astype(np.int64),
            p + "ref_src_index": index[0].astype(np.int64), p + "ref_tgt_index": index[1].astype(np.int64),
        })
        print(name, "key", key, "kept", [int(m.sum()) for m in masks], "corr", sample["correspondences"].shape,
              "cos", float(dirs[0] @ dirs[1]))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
