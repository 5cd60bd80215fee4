"""Training augmentation of a batch of pairs, on the device.

The reference's 3DMatch and KITTI training loaders run RigidPerturb(cfg.perturb_pose) -> Jitter(cfg.augment_noise) ->
ShufflePoints() -> RandomSwap() per pair on the CPU, on the global numpy / random / torch generators
(data_loaders/__init__.py:17-54, data_loaders/transforms.py:15-179).  Here all pairs of a step are augmented by one
library call (ops.augment_pairs -> spr_augment_pairs, csrc/augment.hip) and every draw is a pure function of
(seed, pair_key): a pair is augmented identically whatever batch, position or rank it lands in.  The draw contract and
the float64 apply contract are in include/spr.h ("8f-6").  ModelNet's own pipeline (modelnet_transforms.py) is
modelnet.make_pairs (include/spr.h "8f-7").
"""
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import ops


def output_lengths(src_lens: Sequence[int], tgt_lens: Sequence[int], swap: Sequence[bool], max_pts: int
                   ) -> Tuple[List[int], List[int]]:
    """Per-pair lengths of the augmented clouds: min(len, max_pts), sides exchanged where the pair swaps.  Known on the
    host from the decisions alone (no device read)."""
    out_s, out_t = [], []
    for ls, lt, sw in zip(src_lens, tgt_lens, swap):
        ls, lt = min(int(ls), int(max_pts)), min(int(lt), int(max_pts))
        out_s.append(lt if sw else ls)
        out_t.append(ls if sw else lt)
    return out_s, out_t


def augment_batch(batch: dict, cfg, seed: int, pair_keys, max_pts: int = 30000, direction_cols=()) -> dict:
    """The reference's transforms_aug on a collate_pair dict: src_xyz / tgt_xyz (lists of [N,3] device tensors), pose
    ([B,3,4] or [B,4,4], src -> tgt) and, if present, src_overlap / tgt_overlap (lists of per-point bool masks),
    correspondences (list of [2,K] integer tensors, local indices) and src_path / tgt_path.  cfg.perturb_pose
    ('none' | 'small' | 'large') and cfg.augment_noise select the perturbation and the jitter scale; pair_keys [B]
    (ints below 2^63, e.g. dataset index + epoch * dataset size) and seed select the draws.
    Per-point input features (src_point_feats / tgt_point_feats: lists of [N, C] tensors row-aligned with the clouds)
    follow their points through ShufflePoints and RandomSwap -- gathered by the permutation the library call returns
    and exchanged where the pair swaps -- with their values untouched: every column is treated as a scalar per point
    (colour, intensity, height).  Direction-valued columns such as normals are named in direction_cols: every entry is
    the first column of an (x, y, z) triple (at most 4, inside C, not overlapping), and RigidPerturb rotates that
    triple by the rotation it applies to the cloud -- R of the drawn perturbation on the perturbed side, the identity
    on the other and in mode 'none'; component k becomes f32((R_k0 x + R_k1 y) + R_k2 z) in float64, not renormalised
    (normals.gather_rotate: one library call per side in place of the gather).  With the empty default no column is
    rotated.  With features the returned dict also holds 'src_perm' / 'tgt_perm' (lists of int64 [n]:
    the row of every output point in the cloud it came from, i.e. the caller's tgt cloud where the pair swapped).
    Returns a NEW dict (other entries are carried over by reference); the caller's is not modified.  One library
    call for all pairs and one small device-to-host read (per-pair status and surviving correspondence counts)."""
    src_list, tgt_list = list(batch['src_xyz']), list(batch['tgt_xyz'])
    nb = len(src_list)
    if len(tgt_list) != nb:
        raise ValueError(f"augment_batch: {nb} source clouds, {len(tgt_list)} target clouds")
    pair_keys = np.asarray(pair_keys, dtype=np.uint64).reshape(-1)
    if pair_keys.size != nb:
        raise ValueError(f"augment_batch: {pair_keys.size} pair keys for {nb} pairs")
    dev = src_list[0].device if src_list else batch['pose'].device
    mode = cfg.get('perturb_pose', 'none') or 'none'
    scale = float(cfg.get('augment_noise', 0.0))
    src_lens = [int(s.shape[0]) for s in src_list]
    tgt_lens = [int(t.shape[0]) for t in tgt_list]
    has_feats = batch.get('src_point_feats') is not None or batch.get('tgt_point_feats') is not None
    if has_feats:
        if batch.get('src_point_feats') is None or batch.get('tgt_point_feats') is None:
            raise ValueError("augment_batch: 'src_point_feats' and 'tgt_point_feats' come together")
        feats = list(batch['src_point_feats']) + list(batch['tgt_point_feats'])
        if len(feats) != 2 * nb or any(f.dim() != 2 or int(f.shape[0]) != n or f.shape[1] != feats[0].shape[1]
                                       for f, n in zip(feats, src_lens + tgt_lens)):
            raise ValueError("augment_batch: point features must be one [n, C] tensor per cloud, row-aligned with it")
    direction_cols = tuple(direction_cols)
    if direction_cols:
        if not has_feats:
            raise ValueError("augment_batch: direction_cols without 'src_point_feats' / 'tgt_point_feats'")
        from . import normals
        direction_cols = tuple(normals.check_direction_cols(direction_cols, int(feats[0].shape[1]) if feats else 3))
    perturb_src, swap, perturb = ops.augment_draw(seed, pair_keys, mode)
    out_s, out_t = output_lengths(src_lens, tgt_lens, swap, max_pts)

    def _cat(ts, dtype, width=None):
        shape = (0,) if width is None else (0, width)
        ts = [t.reshape(-1, width) if width else t.reshape(-1) for t in ts]
        return torch.cat(ts).to(dtype) if ts else torch.empty(shape, dtype=dtype, device=dev)

    src, tgt = _cat(src_list, torch.float32, 3), _cat(tgt_list, torch.float32, 3)
    pose = batch['pose'].to(device=dev, dtype=torch.float32)[:, :3, :].contiguous()
    has_mask = 'src_overlap' in batch and 'tgt_overlap' in batch
    has_corr = 'correspondences' in batch
    kw = {}
    if has_mask:
        kw['src_mask'] = _cat(list(batch['src_overlap']), torch.uint8)
        kw['tgt_mask'] = _cat(list(batch['tgt_overlap']), torch.uint8)
    if has_corr:
        corrs = [c.reshape(2, -1) for c in batch['correspondences']]
        counts = [int(c.shape[1]) for c in corrs]
        kw['corr'] = torch.cat(corrs, dim=1).to(torch.int32) if corrs else torch.empty((2, 0), dtype=torch.int32, device=dev)
        kw['corr_off'] = np.concatenate([[0], np.cumsum(counts)])[:nb].astype(np.int32)
        kw['corr_count'] = np.asarray(counts, dtype=np.int32)
    r = ops.augment_pairs(src, ops.lengths_to_cu(src_lens, dev), tgt, ops.lengths_to_cu(tgt_lens, dev), pose,
                          perturb_src, swap, perturb, mode, scale, max_pts=max_pts, seed=seed, pair_keys=pair_keys,
                          out_lens=(out_s, out_t), **kw)
    host = torch.cat([r['status'], r['corr_count']]).tolist() if has_corr else r['status'].tolist()
    if any(host[:nb]):
        bad = [b for b in range(nb) if host[b]]
        raise RuntimeError(f"spr_augment_pairs: non-finite coordinates, pose or perturbation in pairs {bad}")

    out = dict(batch)
    out['src_xyz'] = list(torch.split(r['src_xyz'], out_s))
    out['tgt_xyz'] = list(torch.split(r['tgt_xyz'], out_t))
    new_pose = r['pose']
    if batch['pose'].shape[-2] == 4:          # keep a homogeneous [B,4,4] pose homogeneous
        new_pose = torch.cat([new_pose, batch['pose'].to(device=dev, dtype=torch.float32)[:, 3:, :]], dim=1)
    out['pose'] = new_pose
    if has_mask:
        out['src_overlap'] = list(torch.split(r['src_mask'], out_s))
        out['tgt_overlap'] = list(torch.split(r['tgt_mask'], out_t))
    if has_corr:
        new_counts, corr64 = host[nb:], r['corr'].long()          # one conversion; the per-pair entries are views
        out['correspondences'] = [corr64[:, int(o):int(o) + k] for o, k in zip(kw['corr_off'], new_counts)]
    if has_feats:
        rot = None
        if direction_cols:      # per pair: (rotation of the caller's src cloud, of its tgt cloud)
            eye = np.eye(3, dtype=np.float32)
            rot = [(perturb[b, :, :3] if mode != 'none' and perturb_src[b] else eye,
                    perturb[b, :, :3] if mode != 'none' and not perturb_src[b] else eye) for b in range(nb)]
        out.update(permute_point_feats(feats, r['src_perm'], r['tgt_perm'], src_lens, tgt_lens, out_s, out_t, swap,
                                       rot, direction_cols))
    if 'src_path' in batch and 'tgt_path' in batch:
        sp, tp = list(batch['src_path']), list(batch['tgt_path'])
        out['src_path'] = [tp[b] if swap[b] else sp[b] for b in range(nb)]
        out['tgt_path'] = [sp[b] if swap[b] else tp[b] for b in range(nb)]
    return out


def permute_point_feats(feats, src_perm, tgt_perm, src_lens, tgt_lens, out_s, out_t, swap, rot=None,
                        direction_cols=()) -> dict:
    """ShufflePoints and RandomSwap on per-point features.  feats: [src_0.., tgt_0..] tensors [n, C]; src_perm /
    tgt_perm: packed per OUTPUT side, each entry the local row of that output point in the cloud it came from
    (ops.augment_pairs' contract: on a swap the permutations change sides with the clouds).  One gather per side over
    the packed features; works on any device.  Returns the four batch entries.
    With direction_cols, rot holds per pair the [3,3] rotations of the caller's (src, tgt) clouds, and the gather of a
    side is one normals.gather_rotate call that rotates the listed triples by the rotation of each row's cloud of
    origin (device only)."""
    nb = len(src_lens)
    packed = torch.cat(feats)
    dev = packed.device
    starts = np.concatenate([[0], np.cumsum(list(src_lens) + list(tgt_lens))]).astype(np.int64)
    res = {}
    for side, perm, lens in (('src', src_perm, out_s), ('tgt', tgt_perm, out_t)):
        # where each output cloud of this side came from in `packed`: the other side's cloud where the pair swapped
        origin = [(b + nb if bool(swap[b]) else b) if side == 'src' else (b if bool(swap[b]) else b + nb) for b in range(nb)]
        base = torch.from_numpy(np.repeat(starts[origin], np.asarray(lens, dtype=np.int64))).to(dev)
        local = perm.to(device=dev, dtype=torch.int64)
        if direction_cols:
            from . import normals
            r_out = np.stack([rot[o % nb][o // nb] for o in origin]) if nb else np.zeros((0, 3, 3), np.float32)
            moved = normals.gather_rotate(packed, local + base, ops.lengths_to_cu(list(lens), dev), r_out, direction_cols)
        else:
            moved = packed.index_select(0, local + base)
        res[f'{side}_point_feats'] = list(torch.split(moved, list(lens)))
        res[f'{side}_perm'] = list(torch.split(local, list(lens)))
    return res


class TrainAugmentation:
    """Callable form: TrainAugmentation(cfg)(batch, seed, pair_keys) -> augmented copy of the batch."""

    def __init__(self, cfg, max_pts: int = 30000, direction_cols=()):
        self.cfg, self.max_pts, self.direction_cols = cfg, int(max_pts), tuple(direction_cols)

    def __call__(self, batch: dict, seed: int, pair_keys) -> dict:
        return augment_batch(batch, self.cfg, seed, pair_keys, self.max_pts, self.direction_cols)
