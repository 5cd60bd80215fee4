"""Ground-truth overlap labels from clouds and poses, on the device.

The reference labels every training pair on the CPU (utils/pointcloud.py:8-65 compute_overlap: one Open3D
kd-tree radius query per point; called by the loaders, data_loaders/threedmatch.py:78-84, and by
data_processing/compute_overlap_*.py).  Here the labels of all pairs of a batch come from one library call
(ops.gt_overlap -> spr_gt_overlap, csrc/gt_overlap.hip); the contract is the float64 definition in
include/spr.h, including the reference's `> 0` in the mutual test (a source point whose mutual partner is
target index 0 is absent from the correspondence list but set in the mask).
"""
from typing import List, Tuple

import torch

from . import ops


def _label(src_list, tgt_list, pose, radius: float):
    """Per-pair (src_mask, tgt_mask, corr [2,K] int64) lists from one ops.gt_overlap call."""
    dev = src_list[0].device if src_list else pose.device
    src_lens = [int(s.shape[0]) for s in src_list]
    tgt_lens = [int(t.shape[0]) for t in tgt_list]
    src_cu = ops.lengths_to_cu(src_lens, dev)
    tgt_cu = ops.lengths_to_cu(tgt_lens, dev)
    src = torch.cat([s.reshape(-1, 3).to(torch.float32) for s in src_list]) if src_list else torch.empty((0, 3), device=dev)
    tgt = torch.cat([t.reshape(-1, 3).to(torch.float32) for t in tgt_list]) if tgt_list else torch.empty((0, 3), device=dev)
    _, _, src_mask, tgt_mask, corr, counts = ops.gt_overlap(src, src_cu, tgt, tgt_cu, pose, radius)
    src_ov = list(torch.split(src_mask, src_lens))
    tgt_ov = list(torch.split(tgt_mask, tgt_lens))
    corrs, beg = [], 0
    for n, k in zip(src_lens, counts):
        corrs.append(corr[:, beg:beg + k].long())
        beg += n
    return src_ov, tgt_ov, corrs


def compute_overlap(src: torch.Tensor, tgt: torch.Tensor, search_voxel_size: float
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The reference's compute_overlap (utils/pointcloud.py:8-65) for one pair whose source is already in the
    target's frame: (has_corr_src [N] bool, has_corr_tgt [M] bool, src_tgt_corr [2, K] int64), device tensors.
    A point has a correspondence when the other cloud has a point closer than `search_voxel_size` (strict)."""
    src = ops._dev(src, "src", torch.float32)
    tgt = ops._dev(tgt, "tgt", torch.float32)
    pose = torch.eye(4, dtype=torch.float32, device=src.device)[:3][None].contiguous()
    src_ov, tgt_ov, corrs = _label([src], [tgt], pose, search_voxel_size)
    return src_ov[0], tgt_ov[0], corrs[0]


def label_batch(batch: dict, radius: float) -> dict:
    """Fills batch['src_overlap'], batch['tgt_overlap'] (lists of per-point bool masks) and
    batch['correspondences'] (list of [2, K] int64, local indices) from batch['src_xyz'], batch['tgt_xyz']
    (lists of [N,3] device tensors) and batch['pose'] ([B,3,4], src -> tgt): one library call for all pairs."""
    src_list: List[torch.Tensor] = list(batch['src_xyz'])
    tgt_list: List[torch.Tensor] = list(batch['tgt_xyz'])
    if len(src_list) != len(tgt_list):
        raise ValueError(f"label_batch: {len(src_list)} source clouds, {len(tgt_list)} target clouds")
    dev = src_list[0].device if src_list else batch['pose'].device
    pose = batch['pose'].to(device=dev, dtype=torch.float32)[:, :3, :].contiguous()
    batch['src_overlap'], batch['tgt_overlap'], batch['correspondences'] = _label(src_list, tgt_list, pose, radius)
    return batch
