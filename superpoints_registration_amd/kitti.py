"""The KITTI loader's point path on the device: raw Velodyne scans of a whole batch -> the batch dict of the forward.

KittiDataset.__getitem__ (data_loaders/kitti_pred.py:203-230) runs, per scan and on the CPU, kiss-icp's first-point
voxel filter at config.first_subsampling_dl, the crop to config.crop_radius and the ground cut of config.remove_ground.
prepare_pairs does the same for every scan of a batch with one library call (ops.prepare_scans) and one device->host
copy.  The loader's ICP refinement of the ground-truth pose (:161-183: Open3D point-to-point ICP on the raw scans,
threshold 0.2 m, 200 iterations, cached on disk because it takes seconds per pair) is refine_pose=True: all pairs of
the batch in one call of the `icp` subpackage, or with icp_method='point_to_plane' of the `icp_plane` subpackage.
"""
from typing import List, Optional, Sequence

import torch

from . import ops


def prepare_pairs(src_scans: Sequence[torch.Tensor], tgt_scans: Sequence[torch.Tensor], cfg,
                  pose: Optional[torch.Tensor] = None, intensity: bool = False, normals_radius: Optional[float] = None,
                  normals_limit: int = 40, refine_pose: bool = False, icp_distance: float = 0.2,
                  icp_max_iter: int = 200, icp_method: str = 'point_to_point',
                  icp_normals_radius: Optional[float] = None, icp_kernel: str = 'l2',
                  icp_kernel_k: Optional[float] = None) -> dict:
    """src_scans / tgt_scans: B raw scans each, [n_i, 3] or [n_i, 4] float32 device tensors (4 columns:
    np.fromfile(...).reshape(-1, 4) as it is, x y z reflectance; all scans of a call have the same width).  cfg: the
    experiment's config (first_subsampling_dl; crop_radius and remove_ground default to 0.0 and False).  pose: [B,3,4]
    or [B,4,4] ground truth (src -> tgt), passed through.
    Returns the collate_pair dict RegTR.forward and Trainer.train_step read: 'src_xyz' / 'tgt_xyz' (lists of [m_i, 3],
    views of one packed tensor), 'pose', and 'src_index' / 'tgt_index' (lists of int64 [m_i]: each kept point's row in
    its raw scan, to take reflectance or labels along).  A scan of which nothing survives raises ValueError.
    intensity=True (needs [n, 4] scans) adds 'src_point_feats' / 'tgt_point_feats': [m_i, 2] float32 = [1, reflectance]
    per kept point, column 3 of the raw scan gathered by the returned index -- the in_feats_dim = 2 input of RegTR
    (ones first, so that KPConv's neighbour count, which counts rows of positive feature sum, keeps its meaning).
    normals_radius (metres; None: no normals) appends the surface normal of every kept point, estimated over its
    normals_limit nearest kept points within that radius (normals.estimate) and oriented towards the sensor, the
    scan's origin: 'src_point_feats' / 'tgt_point_feats' are then [1, nx, ny, nz], or [1, reflectance, nx, ny, nz]
    with intensity=True -- direction_cols (1,) or (2,) for the augmentation.  A point with fewer than 3 kept points
    in range has the zero normal.
    refine_pose=True (needs `pose`): point-to-point ICP from `pose` on the RAW scans' xyz, before the voxel filter, as
    the loader does it (icp.icp_pairs with max_dist icp_distance, at most icp_max_iter steps); 'pose' is then the
    refined pose [B,3,4] float32 and 'icp_fitness' / 'icp_rmse' ([B] float64) tell how well it fits.  Everything else
    in the dict is what it is without the flag.
    icp_method='point_to_plane' refines by point-to-plane ICP instead (icp_plane.icp_pairs, kernel icp_kernel = 'l2',
    'huber' or 'tukey' with parameter icp_kernel_k): the normals of the RAW target scans are estimated at
    icp_normals_radius (metres, required with this method; normals_limit nearest points) and face the sensor at the
    origin, like those of normals_radius."""
    src, tgt = list(src_scans), list(tgt_scans)
    B = len(src)
    if B < 1 or len(tgt) != B:
        raise ValueError(f"prepare_pairs: {B} source scans, {len(tgt)} target scans")
    scans = src + tgt
    widths = {tuple(s.shape[1:]) if isinstance(s, torch.Tensor) else None for s in scans}
    if len(widths) != 1 or next(iter(widths)) not in ((3,), (4,)):
        raise ValueError("prepare_pairs: scans must all be [n, 3] or all be [n, 4], got trailing shapes "
                         f"{sorted(map(str, widths))}")
    if intensity and next(iter(widths)) != (4,):
        raise ValueError("prepare_pairs: intensity=True needs [n, 4] scans (x y z reflectance)")
    if refine_pose and pose is None:
        raise ValueError("prepare_pairs: refine_pose=True needs the pose to refine")
    if icp_method not in ('point_to_point', 'point_to_plane'):
        raise ValueError(f"prepare_pairs: icp_method {icp_method!r}, expected 'point_to_point' or 'point_to_plane'")
    if refine_pose and icp_method == 'point_to_plane' and icp_normals_radius is None:
        raise ValueError("prepare_pairs: icp_method='point_to_plane' needs icp_normals_radius")
    lens = [int(s.shape[0]) for s in scans]
    if min(lens) < 1:
        b = lens.index(min(lens))
        raise ValueError(f"prepare_pairs: the {'source' if b < B else 'target'} scan of pair {b % B} is empty")
    dev = scans[0].device
    xyz, out_cu, idx = ops.prepare_scans(torch.cat([s.to(torch.float32) for s in scans]), ops.lengths_to_cu(lens, dev),
                                         float(cfg.first_subsampling_dl), float(cfg.get('crop_radius', 0.0)),
                                         bool(cfg.get('remove_ground', False)))
    out_lens = [b - a for a, b in zip(out_cu, out_cu[1:])]
    for b, m in enumerate(out_lens):
        if m == 0:
            raise ValueError(f"prepare_pairs: nothing of the {'source' if b < B else 'target'} scan of pair {b % B} "
                             f"survives the crop (crop_radius {cfg.get('crop_radius', 0.0)}, remove_ground "
                             f"{cfg.get('remove_ground', False)})")
    clouds: List[torch.Tensor] = list(torch.split(xyz, out_lens))
    index: List[torch.Tensor] = list(torch.split(idx.long(), out_lens))
    out = {'src_xyz': clouds[:B], 'tgt_xyz': clouds[B:], 'pose': pose, 'src_index': index[:B], 'tgt_index': index[B:]}
    feats = None
    if intensity:
        kept = [s[:, 3].index_select(0, i).to(torch.float32) for s, i in zip(scans, index)]
        feats = [torch.stack([torch.ones_like(v), v], dim=1) for v in kept]
    if normals_radius is not None:
        from . import normals
        nrm = normals.estimate(xyz, out_lens, float(normals_radius), int(normals_limit),
                               viewpoint=torch.zeros((2 * B, 3), dtype=torch.float32, device=dev))
        first = feats if feats is not None else [torch.ones((m, 1), dtype=torch.float32, device=dev) for m in out_lens]
        feats = [torch.cat([f, n], dim=1) for f, n in zip(first, torch.split(nrm, out_lens))]
    if feats is not None:
        out['src_point_feats'], out['tgt_point_feats'] = feats[:B], feats[B:]
    if refine_pose:
        raw = [s[:, :3].to(torch.float32).contiguous() for s in scans]
        if icp_method == 'point_to_plane':
            from . import icp_plane
            nrm = icp_plane.estimate_target_normals(raw[B:], float(icp_normals_radius), int(normals_limit),
                                                    viewpoint=torch.zeros((B, 3), dtype=torch.float32, device=dev))
            r = icp_plane.icp_pairs(raw[:B], raw[B:], nrm, pose, float(icp_distance), int(icp_max_iter),
                                    kernel=icp_kernel, kernel_k=icp_kernel_k)
        else:
            from . import icp
            r = icp.icp_pairs(raw[:B], raw[B:], pose, float(icp_distance), int(icp_max_iter))
        out['pose'], out['icp_fitness'], out['icp_rmse'] = r['pose'], r['fitness'], r['inlier_rmse']
    return out
