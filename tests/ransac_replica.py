"""numpy float64 statement of the RANSAC contract of include/spr.h ("RANSAC for all pairs in one call", points 1-4),
written from the header: the draws, the hypothesis solve, the scores and the pick.  Shared by test_ransac_host.py,
test_gpu_ransac.py and scripts/gen_ransac_golden.py (not a test module).  Sums are numpy's float64 sums, not the
kernel's lane order: what is compared against this replica is compared within a tolerance."""
import numpy as np

import augment_replica

TAG_RANSAC = 3
EMPTY, BAD_INDEX, BAD_LAYOUT = 1, 2, 4
WELL_POSED = 1e-3          # a hypothesis is well-posed when s_2 >= WELL_POSED * s_1 of its covariance


def draw(seed, pair_key, n, n_hyp, sample):
    """Point 1: int32 [n_hyp, sample] -- sample s of hypothesis h is word s & 3 of block h * SB + (s >> 2) of the
    pair's tag-3 stream (side 0), idx = (word * n) >> 32."""
    sb = (sample + 3) // 4
    assert n_hyp * sb < 2 ** 32
    words = augment_replica.block(seed, pair_key, 0, np.arange(n_hyp * sb, dtype=np.uint64), TAG_RANSAC)
    words = words.reshape(n_hyp, sb * 4)[:, :sample].astype(np.uint64)
    return ((words * np.uint64(n)) >> np.uint64(32)).astype(np.int32)


def hypotheses(a, b, w, idx):
    """Point 2: compute_rigid_transform on the gathered triples of every row of idx [H, S].  Returns the float64 poses
    [H,3,4] and the singular values [H,3] (descending) of the covariances."""
    a, b, w = (np.asarray(x, dtype=np.float64) for x in (a, b, w))
    sa, sb, sw = a[idx], b[idx], w[idx]                                   # [H,S,3], [H,S,3], [H,S]
    wn = sw / np.maximum(sw.sum(axis=1, keepdims=True), 1e-6)
    ca = (sa * wn[..., None]).sum(axis=1)
    cb = (sb * wn[..., None]).sum(axis=1)
    da, db = sa - ca[:, None], (sb - cb[:, None]) * wn[..., None]
    cov = np.einsum('hsr,hsc->hrc', da, db)
    u, s, vt = np.linalg.svd(cov)
    v = np.swapaxes(vt, 1, 2)
    rot = v @ np.swapaxes(u, 1, 2)
    v_neg = v.copy()
    v_neg[:, :, 2] *= -1
    rot = np.where((np.linalg.det(rot) > 0)[:, None, None], rot, v_neg @ np.swapaxes(u, 1, 2))
    t = cb - np.einsum('hrc,hc->hr', rot, ca)
    return np.concatenate([rot, t[..., None]], axis=2), s


def scores(poses, a, b):
    """Point 3 in float64: mean_i ||b_i - (R a_i + t)|| for poses [H,3,4] (hand in the float32-rounded ones)."""
    poses, a, b = (np.asarray(x, dtype=np.float64) for x in (poses, a, b))
    moved = np.einsum('hrc,ic->hir', poses[:, :, :3], a) + poses[:, None, :, 3]
    return np.linalg.norm(b[None] - moved, axis=2).mean(axis=1)


def pick(score):
    """Point 4, the loop as written: the first minimum; a NaN never wins; a NaN score[0] keeps 0."""
    best = 0
    for h in range(1, len(score)):
        if score[h] < score[best]:
            best = h
    return best


def well_posed(s):
    return (s[:, 0] > 0) & (s[:, 1] >= WELL_POSED * s[:, 0])


def ransac_pair(a, b, w, idx):
    """Points 2-4 for one pair.  Returns a dict: pose64 [H,3,4], hyp_pose (float32), score (float64, from the rounded
    poses), best, pose (float32), sv [H,3]."""
    pose64, sv = hypotheses(a, b, w, idx)
    hyp = pose64.astype(np.float32)
    sc = scores(hyp, a, b)
    best = pick(sc)
    return {'pose64': pose64, 'hyp_pose': hyp, 'score': sc, 'best': best, 'pose': hyp[best], 'sv': sv}


def gap(score):
    """(best score, relative gap of the runner-up above it)."""
    srt = np.sort(np.asarray(score, dtype=np.float64))
    return srt[0], (srt[1] - srt[0]) / srt[0]
