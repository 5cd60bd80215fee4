"""Point-to-plane ICP for all pairs of a batch in one library call (csrc/icp.hip), with an L2, Huber or Tukey kernel.

    icp_pairs(src_list, tgt_list, tgt_normals, pose_init, max_dist, ...)   refine pose_init per pair; dict of results
    icp_pairs(src_list, tgt_list, None, pose_init, max_dist, normals_radius=r, ...)
                                                     the same with the target normals estimated here (normals.estimate)
    icp_pairs_raw(...)                               the first form with 'status' per pair instead of raising

The contract -- Open3D's registration_icp loop with TransformationEstimationPointToPlane, as a float64 definition -- is
include/spr.h's ("Point-to-plane ICP for all pairs"); evaluation (fitness, inlier RMSE, correspondences), stopping rule,
frozen pairs and the read-back of one integer per four passes are those of the `icp` subpackage.  A subpackage: the top-level modules (kitti.prepare_pairs(icp_method='point_to_plane'), RegTR with
cfg.icp_method) import it lazily and never name its entry points.
"""
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _lib, ops
from ..icp import _pose

KERNELS = {'l2': 0, 'huber': 1, 'tukey': 2}


def _kernel(kernel, kernel_k):
    """(code, k) of a kernel name and its parameter, checked."""
    if kernel not in KERNELS:
        raise ValueError(f"icp_plane: kernel {kernel!r}, expected one of {sorted(KERNELS)}")
    if kernel == 'l2':
        return 0, 0.0
    if kernel_k is None or not float(kernel_k) > 0.0 or not np.isfinite(float(kernel_k)):
        raise ValueError(f"icp_plane: kernel_k must be > 0 with kernel {kernel!r}, got {kernel_k}")
    return KERNELS[kernel], float(kernel_k)


def _shapes(clouds, name: str):
    """A list of [n, 3] float32 tensors, checked; where they live is checked last (_on_device)."""
    clouds = list(clouds)
    for b, c in enumerate(clouds):
        if not isinstance(c, torch.Tensor) or c.dim() != 2 or c.shape[1] != 3:
            raise ValueError(f"icp_plane: {name}[{b}] is {tuple(c.shape) if isinstance(c, torch.Tensor) else type(c)}, "
                             "expected an [n, 3] tensor")
        if c.dtype != torch.float32:
            raise ValueError(f"icp_plane: {name}[{b}] is {c.dtype}, expected float32")
    return clouds


def _on_device(**lists):
    first = None
    for name, clouds in lists.items():
        for b, c in enumerate(clouds):
            if not c.is_cuda:
                raise ValueError(f"icp_plane: {name}[{b}] is on {c.device}, expected the MI355X device (no CPU fallback)")
            first = c.device if first is None else first
            if c.device != first:
                raise ValueError("icp_plane: the clouds and normals of a call must be on one device")
    return first


def _checked(src_list, tgt_list, pose_init, max_dist, max_iter, kernel, kernel_k):
    """The host checks that need no normals, shapes first: (src, tgt, pose_init [B, 3, 4], kernel code, k)."""
    src, tgt = list(src_list), list(tgt_list)
    nb = len(src)
    if nb < 1 or len(tgt) != nb:
        raise ValueError(f"icp_plane: {nb} source clouds, {len(tgt)} target clouds")
    if not float(max_dist) > 0.0 or not np.isfinite(float(max_dist)):
        raise ValueError(f"icp_plane: max_dist must be > 0, got {max_dist}")
    if int(max_iter) < 0:
        raise ValueError(f"icp_plane: max_iter must be >= 0, got {max_iter}")
    code, k = _kernel(kernel, kernel_k)
    pose_init = _pose(pose_init, nb)
    return _shapes(src, "src_list"), _shapes(tgt, "tgt_list"), pose_init, code, k


def icp_pairs_raw(src_list: Sequence[torch.Tensor], tgt_list: Sequence[torch.Tensor],
                  tgt_normals: Sequence[torch.Tensor], pose_init, max_dist: float, max_iter: int = 30,
                  rel_fitness: float = 1e-6, rel_rmse: float = 1e-6, kernel: str = 'l2',
                  kernel_k: Optional[float] = None) -> dict:
    """icp_pairs without the status check and without the estimation of normals: the same dict with 'status' int32 [B]
    (0, or -1 for a pair with a non-finite coordinate, normal or pose, whose pose is pose_init and whose other outputs
    are 0 / -1), still on the device.  Reads nothing back here."""
    if tgt_normals is None:                                           # everything is refused on the host, shapes first
        raise ValueError("icp_plane: tgt_normals is None (icp_pairs estimates them when given normals_radius)")
    src, tgt, pose_init, code, k = _checked(src_list, tgt_list, pose_init, max_dist, max_iter, kernel, kernel_k)
    nb = len(src)
    nrm = list(tgt_normals)
    if len(nrm) != nb:
        raise ValueError(f"icp_plane: {len(nrm)} normal tensors for {nb} target clouds")
    nrm = _shapes(nrm, "tgt_normals")
    for b, (t, n) in enumerate(zip(tgt, nrm)):
        if n.shape[0] != t.shape[0]:
            raise ValueError(f"icp_plane: tgt_normals[{b}] has {n.shape[0]} rows, its cloud {t.shape[0]}")
    dev = _on_device(src_list=src, tgt_list=tgt, tgt_normals=nrm)
    pose0 = pose_init.to(device=dev, dtype=torch.float64).contiguous()
    s_lens, t_lens = [int(c.shape[0]) for c in src], [int(c.shape[0]) for c in tgt]
    # one pair: its clouds as they are, no copy
    s_xyz, t_xyz, t_nrm = ((src[0], tgt[0], nrm[0]) if nb == 1 else (torch.cat(src), torch.cat(tgt), torch.cat(nrm)))
    s_xyz, t_xyz, t_nrm = s_xyz.contiguous(), t_xyz.contiguous(), t_nrm.contiguous()
    s_cu, t_cu = ops.lengths_to_cu(s_lens, dev), ops.lengths_to_cu(t_lens, dev)
    ns, nt = sum(s_lens), sum(t_lens)
    L = _lib.lib()
    ws = ops._workspace(L.spr_icp_plane_pairs_workspace_size(ns, nt, nb), dev)
    pose = torch.empty((nb, 3, 4), dtype=torch.float32, device=dev)
    pose64 = torch.empty((nb, 3, 4), dtype=torch.float64, device=dev)
    fitness = torch.empty((nb,), dtype=torch.float64, device=dev)
    rmse = torch.empty((nb,), dtype=torch.float64, device=dev)
    iterations = torch.empty((nb,), dtype=torch.int32, device=dev)
    count = torch.empty((nb,), dtype=torch.int32, device=dev)
    corr = torch.empty((ns,), dtype=torch.int32, device=dev)
    status = torch.empty((nb,), dtype=torch.int32, device=dev)
    _lib.check(L.spr_icp_plane_pairs(ops._ptr(s_xyz), ops._ptr(s_cu), ns, ops._ptr(t_xyz), ops._ptr(t_nrm),
                                     ops._ptr(t_cu), nt, ops._ptr(pose0), nb, float(max_dist), int(max_iter),
                                     float(rel_fitness), float(rel_rmse), code, k, ops._ptr(pose), ops._ptr(pose64),
                                     ops._ptr(fitness), ops._ptr(rmse), ops._ptr(iterations), ops._ptr(count),
                                     ops._ptr(corr), ops._ptr(status), ops._ptr(ws), ws.numel(), ops._stream(s_xyz)),
               "spr_icp_plane_pairs")
    return {'pose': pose, 'pose64': pose64, 'fitness': fitness, 'inlier_rmse': rmse, 'iterations': iterations,
            'count': count, 'corr': list(torch.split(corr, s_lens)), 'status': status}


def estimate_target_normals(tgt_list: Sequence[torch.Tensor], radius: float, limit: int = 40, viewpoint=None):
    """The normals of B target clouds from one radius search and one kernel over the packed clouds (normals.estimate):
    a list of [m_i, 3] float32 tensors.  viewpoint: [B, 3] to orient them, or None."""
    from .. import normals
    tgt = _shapes(tgt_list, "tgt_list")
    _on_device(tgt_list=tgt)
    lens = [int(t.shape[0]) for t in tgt]
    packed = tgt[0] if len(tgt) == 1 else torch.cat(tgt)
    return list(torch.split(normals.estimate(packed, lens, float(radius), int(limit), viewpoint), lens))


def icp_pairs(src_list: Sequence[torch.Tensor], tgt_list: Sequence[torch.Tensor],
              tgt_normals: Optional[Sequence[torch.Tensor]], pose_init, max_dist: float, max_iter: int = 30,
              rel_fitness: float = 1e-6, rel_rmse: float = 1e-6, kernel: str = 'l2', kernel_k: Optional[float] = None,
              normals_radius: Optional[float] = None, normals_limit: int = 40) -> dict:
    """src_list / tgt_list: B clouds each, [n_i, 3] / [m_i, 3] float32 device tensors (empty ones are legal);
    tgt_normals: one [m_i, 3] float32 device tensor per target, row-aligned with it (used as given, not renormalised;
    a zero normal takes no part in the step), or None with normals_radius: the normals are then estimated over the
    normals_limit nearest points within that radius, one search and one kernel for all pairs, and returned as
    'tgt_normals'.  pose_init, max_dist, max_iter, rel_fitness, rel_rmse: as icp.icp_pairs.  kernel: 'l2', 'huber' or
    'tukey' with the parameter kernel_k > 0 (a residual, in the clouds' units).
    Returns the keys of icp.icp_pairs: 'pose' [B,3,4] f32 (= 'pose64' rounded), 'pose64', 'fitness' / 'inlier_rmse' [B]
    f64 (the RMSE is the point distance), 'iterations' / 'count' [B] i32 and 'corr'.  A pair with a non-finite
    coordinate, normal or pose raises ValueError naming it."""
    if tgt_normals is None and normals_radius is None:
        raise ValueError("icp_plane: give tgt_normals, or normals_radius to estimate them")
    if tgt_normals is not None and normals_radius is not None:
        raise ValueError("icp_plane: give tgt_normals or normals_radius, not both")
    estimated = None
    if tgt_normals is None:
        if not float(normals_radius) > 0.0 or not np.isfinite(float(normals_radius)):
            raise ValueError(f"icp_plane: normals_radius must be > 0, got {normals_radius}")
        src, tgt = _checked(src_list, tgt_list, pose_init, max_dist, max_iter, kernel, kernel_k)[:2]
        _on_device(src_list=src, tgt_list=tgt)                        # all of it before the search runs
        tgt_normals = estimated = estimate_target_normals(tgt_list, normals_radius, normals_limit)
    out = icp_pairs_raw(src_list, tgt_list, tgt_normals, pose_init, max_dist, max_iter, rel_fitness, rel_rmse, kernel,
                        kernel_k)
    bad = [b for b, s in enumerate(out.pop('status').tolist()) if s != 0]
    if bad:
        raise ValueError(f"icp_plane: non-finite coordinate, normal or pose in pair {bad[0]}" +
                         (f" (and in pairs {bad[1:]})" if len(bad) > 1 else ""))
    if estimated is not None:
        out['tgt_normals'] = estimated
    return out
