"""Point-to-point ICP for all pairs of a batch in one library call (csrc/icp.hip), and the evaluation of a pose that
is its first pass: fitness = the share of source points with a target point within max_dist, inlier_rmse = the RMS
distance over those.

    icp_pairs(src_list, tgt_list, pose_init, max_dist, ...)   refine pose_init per pair; dict of per-pair results
    icp_pairs_raw(...)                                        the same with 'status' per pair instead of raising
    evaluate(src_list, tgt_list, pose, max_dist)              the max_iter = 0 form: the goodness of fit of a pose

The contract -- Open3D's registration_icp loop with the point-to-point estimate, as a float64 definition -- is
include/spr.h's ("ICP for all pairs").  The target clouds' cell table is built once per call, the iteration runs on the
device (one integer is read back per four passes) and a pair that has converged costs nothing in later passes.
A subpackage: the top-level modules (kitti.prepare_pairs(refine_pose=True), RegTR with cfg.icp_refine) import it
lazily and never name its entry points.
"""
from typing import Sequence

import numpy as np
import torch

from .. import _lib, ops


def _clouds(clouds, name: str):
    clouds = list(clouds)
    for b, c in enumerate(clouds):
        if not isinstance(c, torch.Tensor) or c.dim() != 2 or c.shape[1] != 3:
            raise ValueError(f"icp: {name}[{b}] is {tuple(c.shape) if isinstance(c, torch.Tensor) else type(c)}, "
                             "expected an [n, 3] tensor")
        if c.dtype != torch.float32:
            raise ValueError(f"icp: {name}[{b}] is {c.dtype}, expected float32")
        if not c.is_cuda:
            raise ValueError(f"icp: {name}[{b}] is on {c.device}, expected the MI355X device (no CPU fallback)")
    return clouds


def _pose(pose, nb: int) -> torch.Tensor:
    """The [nb, 3, 4] part of a [nb, 3, 4] or [nb, 4, 4] floating-point tensor or array, checked."""
    if not isinstance(pose, torch.Tensor):
        pose = torch.from_numpy(np.ascontiguousarray(pose, dtype=np.float64))
    if pose.dim() != 3 or pose.shape[0] != nb or tuple(pose.shape[1:]) not in ((3, 4), (4, 4)):
        raise ValueError(f"icp: pose {tuple(pose.shape)} for {nb} pairs, expected [{nb}, 3, 4] or [{nb}, 4, 4]")
    if not pose.is_floating_point():
        raise ValueError(f"icp: pose is {pose.dtype}, expected a floating-point type")
    return pose[:, :3, :]


def icp_pairs_raw(src_list: Sequence[torch.Tensor], tgt_list: Sequence[torch.Tensor], pose_init, max_dist: float,
                  max_iter: int = 30, rel_fitness: float = 1e-6, rel_rmse: float = 1e-6) -> dict:
    """icp_pairs without the status check: the same dict with 'status' int32 [B] (0, or -1 for a pair with a non-finite
    coordinate or pose, whose pose is pose_init and whose other outputs are 0 / -1), still on the device.  Reads nothing
    back here."""
    src, tgt = list(src_list), list(tgt_list)
    nb = len(src)
    if nb < 1 or len(tgt) != nb:                                      # everything is refused on the host, shapes first
        raise ValueError(f"icp: {nb} source clouds, {len(tgt)} target clouds")
    if not float(max_dist) > 0.0 or not np.isfinite(float(max_dist)):
        raise ValueError(f"icp: max_dist must be > 0, got {max_dist}")
    if int(max_iter) < 0:
        raise ValueError(f"icp: max_iter must be >= 0, got {max_iter}")
    pose_init = _pose(pose_init, nb)
    src, tgt = _clouds(src, "src_list"), _clouds(tgt, "tgt_list")
    dev = src[0].device
    if any(c.device != dev for c in src + tgt):
        raise ValueError("icp: the clouds of a call must be on one device")
    pose0 = pose_init.to(device=dev, dtype=torch.float64).contiguous()
    s_lens, t_lens = [int(c.shape[0]) for c in src], [int(c.shape[0]) for c in tgt]
    # one pair: its clouds as they are, no copy
    s_xyz, t_xyz = ((src[0], tgt[0]) if nb == 1 else (torch.cat(src), torch.cat(tgt)))
    s_xyz, t_xyz = s_xyz.contiguous(), t_xyz.contiguous()
    s_cu, t_cu = ops.lengths_to_cu(s_lens, dev), ops.lengths_to_cu(t_lens, dev)
    ns, nt = sum(s_lens), sum(t_lens)
    L = _lib.lib()
    ws = ops._workspace(L.spr_icp_pairs_workspace_size(ns, nt, nb), dev)
    pose = torch.empty((nb, 3, 4), dtype=torch.float32, device=dev)
    pose64 = torch.empty((nb, 3, 4), dtype=torch.float64, device=dev)
    fitness = torch.empty((nb,), dtype=torch.float64, device=dev)
    rmse = torch.empty((nb,), dtype=torch.float64, device=dev)
    iterations = torch.empty((nb,), dtype=torch.int32, device=dev)
    count = torch.empty((nb,), dtype=torch.int32, device=dev)
    corr = torch.empty((ns,), dtype=torch.int32, device=dev)
    status = torch.empty((nb,), dtype=torch.int32, device=dev)
    _lib.check(L.spr_icp_pairs(ops._ptr(s_xyz), ops._ptr(s_cu), ns, ops._ptr(t_xyz), ops._ptr(t_cu), nt,
                               ops._ptr(pose0), nb, float(max_dist), int(max_iter), float(rel_fitness),
                               float(rel_rmse), ops._ptr(pose), ops._ptr(pose64), ops._ptr(fitness), ops._ptr(rmse),
                               ops._ptr(iterations), ops._ptr(count), ops._ptr(corr), ops._ptr(status), ops._ptr(ws),
                               ws.numel(), ops._stream(s_xyz)), "spr_icp_pairs")
    return {'pose': pose, 'pose64': pose64, 'fitness': fitness, 'inlier_rmse': rmse, 'iterations': iterations,
            'count': count, 'corr': list(torch.split(corr, s_lens)), 'status': status}


def icp_pairs(src_list: Sequence[torch.Tensor], tgt_list: Sequence[torch.Tensor], pose_init, max_dist: float,
              max_iter: int = 30, rel_fitness: float = 1e-6, rel_rmse: float = 1e-6) -> dict:
    """src_list / tgt_list: B clouds each, [n_i, 3] / [m_i, 3] float32 device tensors (empty ones are legal);
    pose_init [B, 3, 4] or [B, 4, 4], src -> tgt (tensor on any device, or array; used in float64).  max_dist: the
    correspondence threshold (strict: d2 < max_dist^2).  Stops per pair after max_iter steps, or when fitness and RMSE
    both move by less than rel_fitness / rel_rmse between two passes.
    Returns 'pose' [B,3,4] f32 (= 'pose64' rounded), 'pose64' [B,3,4] f64, 'fitness' / 'inlier_rmse' [B] f64,
    'iterations' / 'count' [B] i32 and 'corr': per pair the int32 [n_i] local target index of every source point under
    the final pose, or -1.  A pair with a non-finite coordinate or pose raises ValueError naming it.  One device-to-host
    read here (the status) beside the library's one integer per four passes."""
    out = icp_pairs_raw(src_list, tgt_list, pose_init, max_dist, max_iter, rel_fitness, rel_rmse)
    bad = [b for b, s in enumerate(out.pop('status').tolist()) if s != 0]
    if bad:
        raise ValueError(f"icp: non-finite coordinate or pose in pair {bad[0]}" +
                         (f" (and in pairs {bad[1:]})" if len(bad) > 1 else ""))
    return out


def evaluate(src_list: Sequence[torch.Tensor], tgt_list: Sequence[torch.Tensor], pose, max_dist: float) -> dict:
    """The goodness of fit of `pose` per pair: icp_pairs with max_iter = 0 ('pose64' is then `pose` itself, 'iterations'
    0).  The library call reads nothing back from the device."""
    return icp_pairs(src_list, tgt_list, pose, max_dist, max_iter=0)
