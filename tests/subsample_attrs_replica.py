"""A numpy restatement of grid subsampling with features and labels (include/spr.h, "a1 with attributes").

Which voxel a point falls into is restated here in float32 (grid_subsampling.cpp:25-31, :53-56); the ROW ORDER of the
voxels, the barycentres and the max_p cut are taken from oracle.native.grid_subsample, which the suite pins to the
reference.  What this file adds is the contract of the attributes:

  features   per voxel and column the float32 sum in point order, from +0, then one float32 division by float32(count);
  labels     per voxel and column the label with the largest count; among tied labels the one that comes first in the
             iteration order of the std::unordered_map<int, int> that received the voxel's labels in point order, restated
             as the list rule of umap_order().
"""
import numpy as np

from oracle import native

# bucket counts of libstdc++'s prime rehash policy: an empty map has 1, the first key brings 13, and the k-th distinct
# key (k from 0) arrives under the first count > k
BUCKETS = (1, 13, 29, 59, 127, 257, 541, 1109, 2357, 5087, 10273, 20753, 42043)


def voxel_keys(pts, dl):
    """uint64 voxel key of every point of ONE cloud: the reference's size_t arithmetic, modulo 2^64."""
    pts, dl = np.asarray(pts, np.float32), np.float32(dl)
    mn, mx = pts.min(0), pts.max(0)
    org = np.floor(mn * (np.float32(1.0) / dl)) * dl
    nx = np.int64(np.floor((mx[0] - org[0]) / dl)) + 1
    ny = np.int64(np.floor((mx[1] - org[1]) / dl)) + 1
    idx = np.floor((pts - org) / dl).astype(np.int64)
    with np.errstate(over="ignore"):
        return (idx[:, 0] + nx * idx[:, 1] + nx * ny * idx[:, 2]).view(np.uint64)


def voxel_rows(pts, lens, dl, max_p=0, order="reference"):
    """(sub_points, sub_lens, rows): rows[r] = ascending global point indices of the voxel behind output row r."""
    pts = np.asarray(pts, np.float32)
    sub, sub_lens, keys, _ = native.grid_subsample(pts, np.asarray(lens, np.int32), dl, max_p=max_p, order=order,
                                                   return_keys=True)
    rows, off, r = [], 0, 0
    for n, m in zip(lens, sub_lens):
        k = voxel_keys(pts[off:off + n], dl)
        members = {}
        for i, key in enumerate(k.tolist()):
            members.setdefault(key, []).append(off + i)
        assert max_p > 0 or len(members) == m
        for key in keys[r:r + m].tolist():
            rows.append(np.asarray(members[key], np.int64))
        off, r = off + n, r + m
    return sub, sub_lens, rows


def ordered_sum(x):
    """float32 sum of the rows of x [k, d] in order, from +0."""
    acc = np.zeros(x.shape[1], np.float32)
    for row in np.asarray(x, np.float32):
        acc = acc + row
    return acc


def tree_sum(x):
    """float32 pairwise-tree sum of the rows of x: what a parallel reduction would compute (NOT the contract)."""
    x = np.asarray(x, np.float32)
    while len(x) > 1:
        if len(x) % 2:
            x = np.concatenate([x, np.zeros((1,) + x.shape[1:], np.float32)])
        x = x[0::2] + x[1::2]
    return x[0]


def umap_order(labels):
    """Distinct values of `labels` (ints, in arrival order) in the iteration order of a std::unordered_map<int, int>:
    hash = the value sign-extended to 64 bits, bucket = hash % bucket_count; a new key goes to the front of the list
    if its bucket is empty, otherwise directly in front of the first list element of its bucket; when the bucket count
    grows the old list is re-inserted, front to back, by the same rule."""
    def insert(lst, key, nbk):
        b = (key % (1 << 64)) % nbk
        for i, other in enumerate(lst):
            if (other % (1 << 64)) % nbk == b:
                lst.insert(i, key)
                return
        lst.insert(0, key)

    lst, seen, epoch = [], set(), 0
    for key in (int(v) for v in labels):
        if key in seen:
            continue
        if epoch == 0 or len(seen) >= BUCKETS[epoch]:
            epoch += 1
            old, lst = lst, []
            for k in old:
                insert(lst, k, BUCKETS[epoch])
        seen.add(key)
        insert(lst, key, BUCKETS[epoch])
    return lst


def vote(labels):
    """(winner, tied labels in arrival order, distinct count) of one voxel's label column."""
    labels = [int(v) for v in labels]
    count, arrival = {}, []
    for v in labels:
        if v not in count:
            arrival.append(v)
        count[v] = count.get(v, 0) + 1
    top = max(count.values())
    tied = [v for v in arrival if count[v] == top]
    if len(tied) == 1:
        return tied[0], tied, len(arrival)
    return next(v for v in umap_order(labels) if count[v] == top), tied, len(arrival)


def grid_subsample(pts, lens, dl, max_p=0, order="reference", feat=None, lab=None):
    """(sub_points, sub_lens, sub_features or None, sub_labels [M, ldim] or None)."""
    sub, sub_lens, rows = voxel_rows(pts, lens, dl, max_p, order)
    out_feat = out_lab = None
    if feat is not None:
        feat = np.asarray(feat, np.float32)
        out_feat = np.empty((len(rows), feat.shape[1]), np.float32)
        for r, members in enumerate(rows):
            out_feat[r] = ordered_sum(feat[members]) / np.float32(len(members))
    if lab is not None:
        lab = np.asarray(lab, np.int32).reshape(len(lab), -1)
        out_lab = np.empty((len(rows), lab.shape[1]), np.int32)
        for r, members in enumerate(rows):
            for col in range(lab.shape[1]):
                out_lab[r, col] = vote(lab[members, col])[0]
    return sub, sub_lens, out_feat, out_lab
