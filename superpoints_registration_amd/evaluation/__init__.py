"""Registration metrics for all pairs of a batch in one library call (csrc/evaluate.hip), and the evaluation the
reference runs at the end of every experiment (GenericRegModel.test_step / test_epoch_end) on top of it.

    eval_pairs(src_list, ref_list, pose_gt, pose_pred, raw_list=None, corr=None, acceptance_radius=None)
                                      every per-pair column of the contract, nearest neighbours included
    eval_pairs_raw(...)               the same with 'status' per pair instead of raising
    modelnet_metrics(...)             benchmark_modelnet.compute_metrics, for a whole batch: the RPMNet / DCP table
    inlier_ratio(...), feature_matching_recall(...)      compute_IR / compute_FMR
    summarize_metrics(metrics), format_metrics(summary)  benchmark_modelnet.summarize_metrics / print_metrics
    Evaluator(cfg)                    update(batch, pred) per batch, summary() / report() at the end

The contract -- a float64 definition per pair -- is include/spr.h's ("Registration metrics for all pairs").  The
Chamfer term is an exact brute-force nearest-neighbour search, O(n m) per pair: right for object-sized clouds.
A subpackage: the top-level modules never name its entry points.
"""
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _lib, formats, ops

# include/spr.h: SPR_EVAL_COLS, and the kernel's two tile constants SPR_EVAL_TILE / SPR_EVAL_QUERIES
COLUMNS = ('r_mse', 'r_mae', 't_mse', 't_mae', 'err_r_deg', 'err_t', 'trans_err', 'chamfer_src', 'chamfer_ref',
           'chamfer_dist', 'inlier_count', 'inlier_ratio')
TILE = 256        # targets per LDS tile
QUERIES = 128     # queries per workgroup
MODELNET_KEYS = ('r_mse', 'r_mae', 't_mse', 't_mae', 'err_r_deg', 'err_t', 'chamfer_dist')


def _clouds(clouds, name: str):
    clouds = list(clouds)
    for b, c in enumerate(clouds):
        if not isinstance(c, torch.Tensor) or c.dim() != 2 or c.shape[1] != 3:
            raise ValueError(f"evaluation: {name}[{b}] is {tuple(c.shape) if isinstance(c, torch.Tensor) else type(c)}, "
                             "expected an [n, 3] tensor")
        if c.dtype != torch.float32:
            raise ValueError(f"evaluation: {name}[{b}] is {c.dtype}, expected float32")
        if not c.is_cuda:
            raise ValueError(f"evaluation: {name}[{b}] is on {c.device}, expected the MI355X device (no CPU fallback)")
    return clouds


def _pose(pose, nb: int, name: str) -> torch.Tensor:
    """The [nb, 3, 4] part of a [nb, 3, 4] or [nb, 4, 4] floating-point tensor or array, checked."""
    if not isinstance(pose, torch.Tensor):
        pose = torch.from_numpy(np.ascontiguousarray(pose, dtype=np.float64))
    if pose.dim() != 3 or pose.shape[0] != nb or tuple(pose.shape[1:]) not in ((3, 4), (4, 4)):
        raise ValueError(f"evaluation: {name} {tuple(pose.shape)} for {nb} pairs, expected [{nb}, 3, 4] or [{nb}, 4, 4]")
    if not pose.is_floating_point():
        raise ValueError(f"evaluation: {name} is {pose.dtype}, expected a floating-point type")
    return pose[:, :3, :]


def _packed(clouds, dev):
    """(xyz [n,3] contiguous, cu, lengths): one cloud as it is, no copy."""
    lens = [int(c.shape[0]) for c in clouds]
    xyz = clouds[0] if len(clouds) == 1 else torch.cat(clouds)
    return xyz.contiguous(), ops.lengths_to_cu(lens, dev), lens


def eval_pairs_raw(src_list: Sequence[torch.Tensor], ref_list: Sequence[torch.Tensor], pose_gt, pose_pred,
                   raw_list: Optional[Sequence[torch.Tensor]] = None, corr=None,
                   acceptance_radius: Optional[float] = None) -> dict:
    """eval_pairs without the status check: the same dict with 'status' int32 [B] (0; -1 for a pair with a non-finite
    coordinate or pose: every column 0, d2 0, nn -1; -2 for a pair whose raw cloud is empty while its source or
    reference is not: the Chamfer columns 0), still on the device.  Reads nothing back."""
    src, ref = list(src_list), list(ref_list)
    nb = len(src)
    if nb < 1 or len(ref) != nb:                                      # everything is refused on the host, shapes first
        raise ValueError(f"evaluation: {nb} source clouds, {len(ref)} reference clouds")
    raw = None if raw_list is None else list(raw_list)
    if raw is not None and len(raw) != nb:
        raise ValueError(f"evaluation: {nb} source clouds, {len(raw)} raw clouds")
    if corr is not None:
        if not isinstance(corr, (tuple, list)) or len(corr) != 2:
            raise ValueError("evaluation: corr must be a pair (src_corr list, tgt_corr list)")
        corr_s, corr_t = list(corr[0]), list(corr[1])
        if len(corr_s) != nb or len(corr_t) != nb:
            raise ValueError(f"evaluation: {nb} source clouds, {len(corr_s)} / {len(corr_t)} correspondence sets")
        if acceptance_radius is None or not float(acceptance_radius) > 0.0 or not np.isfinite(float(acceptance_radius)):
            raise ValueError(f"evaluation: acceptance_radius must be > 0 with correspondences, got {acceptance_radius}")
    pose_gt, pose_pred = _pose(pose_gt, nb, "pose_gt"), _pose(pose_pred, nb, "pose_pred")
    src, ref = _clouds(src, "src_list"), _clouds(ref, "ref_list")
    every = src + ref
    if raw is not None:
        raw = _clouds(raw, "raw_list")
        every = every + raw
    if corr is not None:
        corr_s, corr_t = _clouds(corr_s, "corr[0]"), _clouds(corr_t, "corr[1]")
        for b, (s, t) in enumerate(zip(corr_s, corr_t)):
            if s.shape[0] != t.shape[0]:
                raise ValueError(f"evaluation: corr[0][{b}] has {s.shape[0]} rows, corr[1][{b}] has {t.shape[0]}")
        every = every + corr_s + corr_t
    dev = src[0].device
    if any(c.device != dev for c in every):
        raise ValueError("evaluation: the clouds of a call must be on one device")
    gt64 = pose_gt.to(device=dev, dtype=torch.float64).contiguous()
    pred64 = pose_pred.to(device=dev, dtype=torch.float64).contiguous()
    s_xyz, s_cu, s_lens = _packed(src, dev)
    t_xyz, t_cu, t_lens = _packed(ref, dev)
    ns, nt, nr, nc = sum(s_lens), sum(t_lens), 0, 0
    r_xyz = r_cu = cs_xyz = ct_xyz = c_cu = None
    if raw is not None:
        r_xyz, r_cu, r_lens = _packed(raw, dev)
        nr = sum(r_lens)
    if corr is not None:
        cs_xyz, c_cu, c_lens = _packed(corr_s, dev)
        ct_xyz = _packed(corr_t, dev)[0]
        nc = sum(c_lens)
    L = _lib.lib()
    ws = ops._workspace(L.spr_eval_pairs_workspace_size(ns, nt, nr, nc, nb), dev)
    metrics = torch.empty((nb, len(COLUMNS)), dtype=torch.float64, device=dev)
    status = torch.empty((nb,), dtype=torch.int32, device=dev)
    d2_src = nn_src = d2_ref = nn_ref = None
    if raw is not None:
        d2_src, nn_src = (torch.empty((ns,), dtype=torch.float64, device=dev),
                          torch.empty((ns,), dtype=torch.int32, device=dev))
        d2_ref, nn_ref = (torch.empty((nt,), dtype=torch.float64, device=dev),
                          torch.empty((nt,), dtype=torch.int32, device=dev))
    _lib.check(L.spr_eval_pairs(ops._ptr(s_xyz), ops._ptr(s_cu), ns, ops._ptr(t_xyz), ops._ptr(t_cu), nt,
                                ops._ptr(r_xyz), ops._ptr(r_cu), nr, ops._ptr(cs_xyz), ops._ptr(ct_xyz), ops._ptr(c_cu),
                                nc, ops._ptr(gt64), ops._ptr(pred64), nb,
                                float(acceptance_radius) if corr is not None else 0.0, ops._ptr(metrics),
                                ops._ptr(d2_src), ops._ptr(nn_src), ops._ptr(d2_ref), ops._ptr(nn_ref),
                                ops._ptr(status), ops._ptr(ws), ws.numel(), ops._stream(s_xyz)), "spr_eval_pairs")
    out = {'metrics': metrics, 'status': status}
    out.update({k: metrics[:, i] for i, k in enumerate(COLUMNS)})
    if raw is not None:
        out.update({'d2_src': list(torch.split(d2_src, s_lens)), 'nn_src': list(torch.split(nn_src, s_lens)),
                    'd2_ref': list(torch.split(d2_ref, t_lens)), 'nn_ref': list(torch.split(nn_ref, t_lens))})
    return out


def _named(status) -> str:
    bad = {b: s for b, s in enumerate(status) if s != 0}
    return ", ".join(f"pair {b}: " + ("a non-finite coordinate or pose" if s == -1 else
                                      "an empty raw cloud" if s == -2 else f"status {s}") for b, s in bad.items())


def eval_pairs(src_list: Sequence[torch.Tensor], ref_list: Sequence[torch.Tensor], pose_gt, pose_pred,
               raw_list: Optional[Sequence[torch.Tensor]] = None, corr=None,
               acceptance_radius: Optional[float] = None) -> dict:
    """src_list / ref_list: B clouds each, [n_i, 3] / [m_i, 3] float32 device tensors (empty ones are legal); pose_gt,
    pose_pred [B, 3, 4] or [B, 4, 4], src -> ref (tensors of any floating type on any device, or arrays; used in
    float64).  raw_list: per pair the clean raw shape in the reference's frame -- asks for the Chamfer columns and
    'd2_src' / 'nn_src' / 'd2_ref' / 'nn_ref' (lists: per query the squared distance to and the local index of its
    nearest neighbour).  corr = (src_corr list, tgt_corr list) of [k_i, 3] point sets with acceptance_radius -- asks
    for 'inlier_count' / 'inlier_ratio' under pose_gt (strict: d2 < acceptance_radius^2).
    Returns 'metrics' [B, 12] float64 and one [B] view per name of COLUMNS; a part that was not asked for is 0.
    A pair with a non-zero status raises ValueError naming it.  One device-to-host read here (the status)."""
    out = eval_pairs_raw(src_list, ref_list, pose_gt, pose_pred, raw_list, corr, acceptance_radius)
    status = out.pop('status').tolist()
    if any(status):
        raise ValueError("evaluation: " + _named(status))
    return out


def modelnet_metrics(src_list, ref_list, raw_list, pose_gt, pose_pred) -> dict:
    """benchmark_modelnet.compute_metrics for a whole batch: r_mse, r_mae, t_mse, t_mae (Euler 'xyz' angles in degrees
    and translations, the DCP convention), err_r_deg, err_t (isotropic) and chamfer_dist (the modified Chamfer distance
    against the clean raw shape), each [B] float64 on the device."""
    out = eval_pairs(src_list, ref_list, pose_gt, pose_pred, raw_list=raw_list)
    return {k: out[k] for k in MODELNET_KEYS}


def _no_clouds(nb: int, dev):
    return [torch.empty((0, 3), dtype=torch.float32, device=dev)] * nb


def inlier_ratio(src_corr, tgt_corr, pose_gt, acceptance_radius: float) -> torch.Tensor:
    """compute_IR per pair: the share of correspondences (src_corr[b][k], tgt_corr[b][k]) whose residual under pose_gt
    is below acceptance_radius (strict); [B] float64 on the device, 0 for an empty set."""
    src_corr = list(src_corr)
    if not src_corr or not isinstance(src_corr[0], torch.Tensor):
        raise ValueError("evaluation: inlier_ratio needs a non-empty list of [k, 3] tensors")
    empty = _no_clouds(len(src_corr), src_corr[0].device)
    return eval_pairs(empty, empty, pose_gt, pose_gt, corr=(src_corr, tgt_corr),
                      acceptance_radius=acceptance_radius)['inlier_ratio']


def feature_matching_recall(ir, tau: float = 0.05):
    """compute_FMR: the share of pairs whose inlier ratio is above tau (strict).  A tensor gives a 0-dim float64 tensor
    on its device (nothing is read back), anything else a float."""
    if isinstance(ir, torch.Tensor):
        if ir.numel() == 0:
            raise ValueError("evaluation: feature_matching_recall of no pairs")
        return (ir > tau).to(torch.float64).mean()
    ir = np.asarray(ir, dtype=np.float64)
    if ir.size == 0:
        raise ValueError("evaluation: feature_matching_recall of no pairs")
    return float((ir > tau).mean())


def summarize_metrics(metrics: dict) -> dict:
    """benchmark_modelnet.summarize_metrics, key for key: '*mse' -> sqrt(mean) under '*rmse'; 'err*' -> mean under
    '<key>_mean' and sqrt(mean of squares) under '<key>_rmse'; anything else -> mean.  Values: arrays or tensors [N]."""
    out = {}
    for k, v in metrics.items():
        v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        if k.endswith('mse'):
            out[k[:-3] + 'rmse'] = np.sqrt(np.mean(v))
        elif k.startswith('err'):
            out[k + '_mean'] = np.mean(v)
            out[k + '_rmse'] = np.sqrt(np.mean(v ** 2))
        else:
            out[k] = np.mean(v)
    return out


def format_metrics(summary: dict) -> list:
    """The four lines benchmark_modelnet.print_metrics logs under its title."""
    return [
        'DeepCP metrics:{:.4f}(rot-rmse) | {:.4f}(rot-mae) | {:.4g}(trans-rmse) | {:.4g}(trans-mae)'.format(
            summary['r_rmse'], summary['r_mae'], summary['t_rmse'], summary['t_mae']),
        'Rotation error {:.4f}(deg, mean) | {:.4f}(deg, rmse)'.format(summary['err_r_deg_mean'], summary['err_r_deg_rmse']),
        'Translation error {:.4g}(mean) | {:.4g}(rmse)'.format(summary['err_t_mean'], summary['err_t_rmse']),
        'Chamfer error: {:.7f}(mean-sq)'.format(summary['chamfer_dist']),
    ]


def summarize_kitti(rot_err_deg, trans_err, thresh_rot: float, thresh_trans: float) -> dict:
    """generic_reg_model.py:218-234, 289-292: the mean rotation and translation error over the pairs inside both
    thresholds (strict; NaN when there is none), and the share of such pairs."""
    rot, trans = np.asarray(rot_err_deg, dtype=np.float64), np.asarray(trans_err, dtype=np.float64)
    ok = (rot < thresh_rot) & (trans < thresh_trans)
    n = int(ok.sum())
    return {'rot_err_deg': float(rot[ok].mean()) if n else float('nan'),
            'trans_err': float(trans[ok].mean()) if n else float('nan'),
            'recall': n / rot.size, 'n_success': n, 'n_pairs': int(rot.size)}


class Evaluator:
    """The reference's test loop as an accumulator.  update(batch, pred) per batch: one library call, nothing read
    back; summary() at the end: one device-to-host read.  By cfg.dataset:
      'modelnet'  update reads batch['src_xyz'], ['tgt_xyz'], ['tgt_raw'] (the clean raw shape in the reference's
                  frame) and the poses; summary: the RPMNet / DCP table (summarize_metrics) and 'pred_transforms'
                  [N, 3, 4], what the reference saves as pred_transforms.npy; report: format_metrics' four lines
      'kitti'     update reads the poses only; summary: summarize_kitti at cfg.reg_success_thresh_rot / _trans
      '3dmatch'   update reads pred['src_corr'] / pred['tgt_corr'] (lists of [k, 3]) and the poses; summary: the mean
                  inlier ratio and the feature-matching recall at cfg.acceptance_radius; write_est_log hands every
                  predicted pose to formats.write_est_log (batch['src_path'] / ['tgt_path'] are then needed)
    batch['pose']: the ground truth [B, 3, 4]; pred['pose']: [B, 3, 4] or [L, B, 3, 4] (the last of L is used).
    A pair with a non-zero status makes summary() raise ValueError naming it (by its position in the run)."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.dataset = cfg.dataset
        if self.dataset not in ('modelnet', 'kitti', '3dmatch'):
            raise NotImplementedError(f"Evaluator: dataset {self.dataset!r}")
        self._rows = []      # per batch [B, 12 + 1 + 12] float64 on the device: metrics, status, predicted pose
        self._paths = []     # 3dmatch: (src_path, tgt_path) per pair
        self._table = None

    def update(self, batch: dict, pred: dict) -> None:
        pose = pred['pose']
        if isinstance(pose, torch.Tensor) and pose.dim() == 4:
            pose = pose[-1]
        gt = batch['pose']
        nb = len(batch['src_xyz'])
        dev = batch['src_xyz'][0].device
        if self.dataset == 'modelnet':
            out = eval_pairs_raw(batch['src_xyz'], batch['tgt_xyz'], gt, pose, raw_list=batch['tgt_raw'])
        elif self.dataset == 'kitti':
            out = eval_pairs_raw(_no_clouds(nb, dev), _no_clouds(nb, dev), gt, pose)
        else:
            out = eval_pairs_raw(_no_clouds(nb, dev), _no_clouds(nb, dev), gt, pose,
                                 corr=(pred['src_corr'], pred['tgt_corr']),
                                 acceptance_radius=float(self.cfg.acceptance_radius))
            if 'src_path' in batch:
                self._paths += list(zip(batch['src_path'], batch['tgt_path']))
        p64 = _pose(pose, nb, "pred['pose']").to(device=dev, dtype=torch.float64).reshape(nb, 12)
        self._rows.append(torch.cat([out['metrics'], out['status'].to(torch.float64)[:, None], p64], dim=1))
        self._table = None

    def _host(self) -> np.ndarray:
        if not self._rows:
            raise ValueError("Evaluator: no pairs")
        if self._table is None:
            self._table = torch.cat(self._rows).cpu().numpy()          # the one read
        return self._table

    def per_pair(self) -> dict:
        """Every column of COLUMNS as a host array [N], after the status check."""
        return self._summarize(self._host())[0]

    def _summarize(self, table: np.ndarray):
        status = table[:, len(COLUMNS)].astype(np.int64).tolist()
        if any(status):
            raise ValueError("Evaluator: " + _named(status))
        cols = {k: table[:, i] for i, k in enumerate(COLUMNS)}
        if self.dataset == 'modelnet':
            s = summarize_metrics({k: cols[k] for k in MODELNET_KEYS})
            s['pred_transforms'] = table[:, len(COLUMNS) + 1:].reshape(-1, 3, 4)
        elif self.dataset == 'kitti':
            s = summarize_kitti(cols['err_r_deg'], cols['trans_err'], self.cfg.reg_success_thresh_rot,
                                self.cfg.reg_success_thresh_trans)
        else:
            s = {'inlier_ratio': float(cols['inlier_ratio'].mean()),
                 'feature_matching_recall': feature_matching_recall(cols['inlier_ratio']),
                 'n_pairs': int(table.shape[0])}
        return cols, s

    def summary(self) -> dict:
        return self._summarize(self._host())[1]

    def report(self) -> list:
        s = self.summary()
        if self.dataset == 'modelnet':
            return format_metrics(s)
        if self.dataset == 'kitti':
            return [f"KITTI: rotation error {s['rot_err_deg']:.4f}(deg) | translation error {s['trans_err']:.4g} over "
                    f"{s['n_success']} of {s['n_pairs']} pairs (recall {s['recall']:.4f})"]
        return [f"3DMatch: inlier ratio {s['inlier_ratio']:.4f} | feature-matching recall "
                f"{s['feature_matching_recall']:.4f} over {s['n_pairs']} pairs"]

    def write_est_log(self, log_path: str, benchmark: str) -> None:
        """3dmatch: every accumulated pose in the est.log files formats.benchmark reads."""
        table = self._host()
        if len(self._paths) != table.shape[0]:
            raise ValueError("Evaluator: write_est_log needs batch['src_path'] / ['tgt_path'] for every pair")
        poses = table[:, len(COLUMNS) + 1:].reshape(-1, 3, 4)
        batch = {'src_xyz': [None] * len(self._paths), 'src_path': [p[0] for p in self._paths],
                 'tgt_path': [p[1] for p in self._paths]}
        formats.write_est_log(log_path, benchmark, batch, {'pose': poses})
