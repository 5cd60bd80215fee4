"""ModelNet training pairs, generated on the device.

In the reference a ModelNet training pair does not exist on disk: data_loaders/modelnet.py:102-109 builds it per sample
from one raw 2048-point shape with SplitSourceRef -> RandomCrop(partial) -> RandomTransformSE3_euler(rot_mag, trans_mag)
-> Resampler(num_points) -> RandomJitter() -> ShufflePoints() (data_loaders/modelnet_transforms.py), on the CPU and on
numpy's global generator.  Here all pairs of a step come from one library call (spr_modelnet_pairs,
csrc/modelnet_pairs.hip) and every draw is a pure function of (seed, pair_key): a pair is generated identically
whatever batch, position or rank it lands in.  The draw contract and the float64 apply contract are in include/spr.h
("8f-7").  Only noise_type 'crop' exists: the reference's 'clean' and 'jitter' chains never create src_overlap, which
ModelNetHdf.__getitem__ then reads.
"""
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, ops
from .ops import _dev, _ptr, _stream, lengths_to_cu

JITTER_SCALE, JITTER_CLIP = 0.01, 0.05        # RandomJitter()'s defaults: the loader passes none


def percentile_q(p_keep: float) -> float:
    """The percentile RandomCrop.crop hands numpy for p_keep: (1.0 - p_keep) * 100 with p_keep a float32 scalar,
    evaluated as numpy evaluates the reference's expression (30.000001907348633 for 0.7)."""
    return float((1.0 - np.float32(p_keep)) * 100)


def output_size(cfg) -> int:
    """Points per generated cloud: Resampler's sizes for a two-entry `partial` are both 717, whatever num_points says
    (modelnet_transforms.py:92-93, kept "to be consistent with Predator").  A one-entry `partial` gives the two clouds
    different sizes there; no shipped configuration has one."""
    if len(cfg.partial) != 2:
        raise NotImplementedError(f"make_pairs: partial {list(cfg.partial)}; only the two-entry form is built")
    return 717


def _pair_keys(pair_keys, nb: int, what: str) -> np.ndarray:
    pk = np.ascontiguousarray(pair_keys, dtype=np.uint64).reshape(-1)
    if pk.size != nb:
        raise ValueError(f"{what}: {pk.size} pair keys for {nb} pairs")
    return pk


def modelnet_draw(seed: int, pair_keys, rot_mag: float, trans_mag: float, cu: Optional[torch.Tensor] = None,
                  n_total: int = 0, k: int = 0):
    """8f-7.  The draws of pairs `pair_keys` under `seed` (spr_modelnet_draw; contract in include/spr.h).
    Returns (dirs [nb,2,3] f64, transform [nb,3,4] f32) as numpy arrays -- host data, no device needed.  With cu
    (device int32 [nb+1]), the packed size n_total and the output size k it also returns the device buffers
    (rkeys [2,n_total], extra [2,nb*k], noise [2,nb*k,3] f32, skeys [2,nb*k]; the uint32 draws as bit patterns in int32
    tensors) that modelnet_pairs generates inline when it is not handed them."""
    pk = np.ascontiguousarray(pair_keys, dtype=np.uint64).reshape(-1)
    nb = pk.size
    dirs = np.zeros((nb, 2, 3), dtype=np.float64)
    tf = np.zeros((nb, 3, 4), dtype=np.float32)
    L = _lib.lib()
    if cu is None:
        _lib.check(L.spr_modelnet_draw(int(seed), pk.ctypes.data, nb, float(rot_mag), float(trans_mag), dirs.ctypes.data,
                                       tf.ctypes.data, None, None, 0, 0, None, None, None, None, None), "spr_modelnet_draw")
        return dirs, tf
    cu = _dev(cu, "cu", torch.int32)
    if cu.numel() - 1 != nb:
        raise ValueError(f"modelnet_draw: {nb} pair keys, a cu array of {cu.numel() - 1} clouds")
    dev = cu.device
    pk_dev = torch.from_numpy(pk.view(np.int64)).to(dev)
    rkeys = torch.empty((2, n_total), dtype=torch.int32, device=dev)
    extra = torch.empty((2, nb * k), dtype=torch.int32, device=dev)
    noise = torch.empty((2, nb * k, 3), dtype=torch.float32, device=dev)
    skeys = torch.empty((2, nb * k), dtype=torch.int32, device=dev)
    _lib.check(L.spr_modelnet_draw(int(seed), pk.ctypes.data, nb, float(rot_mag), float(trans_mag), dirs.ctypes.data,
                                   tf.ctypes.data, _ptr(pk_dev), _ptr(cu), int(n_total), int(k), _ptr(rkeys), _ptr(extra),
                                   _ptr(noise), _ptr(skeys), _stream(cu)), "spr_modelnet_draw")
    return dirs, tf, rkeys, extra, noise, skeys


def modelnet_pairs(xyz: torch.Tensor, cu: torch.Tensor, max_len: int, p_keep: Sequence[float], k: int, transform,
                   dirs, scale: float = JITTER_SCALE, clip: float = JITTER_CLIP, seed: int = 0, pair_keys=None,
                   rkeys: Optional[torch.Tensor] = None, extra: Optional[torch.Tensor] = None,
                   noise: Optional[torch.Tensor] = None, skeys: Optional[torch.Tensor] = None) -> dict:
    """8f-7.  Crop -> transform -> resample -> jitter -> shuffle of all pairs of a batch in one call
    (spr_modelnet_pairs; the float64 contract is in include/spr.h).
    xyz [sum n,3] packed with cu int32 [B+1]; max_len: the longest cloud (host int, at most 8192); p_keep: (source,
    reference) keep fractions in (0, 1]; k: points per output cloud; transform [B,3,4] f32 and dirs [B,2,3] f64 as
    modelnet_draw returns them (host arrays or tensors).  The explicit draw buffers (layouts as modelnet_draw returns
    them) are generated inline from (seed, pair_keys) when None.
    Returns a dict of device tensors: src_xyz / tgt_xyz [B*k,3], pose [B,3,4], src_overlap / tgt_overlap [B*k] bool,
    src_index / tgt_index [B*k] int32 (raw local index of every output point), corr [2,B*k] int32 (pair b owns columns
    from b*k), corr_count [B] and status [B] (device: the only data-dependent values).  No device-to-host read
    happens here."""
    xyz = _dev(xyz, "xyz", torch.float32)
    cu = _dev(cu, "cu", torch.int32)
    dev = xyz.device
    n_total, nb, k = int(xyz.shape[0]), cu.numel() - 1, int(k)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"modelnet_pairs: xyz {tuple(xyz.shape)}, expected [n, 3]")
    p_src, p_tgt = (float(p) for p in p_keep)

    def host_or_dev(t, dtype, shape, name):
        if isinstance(t, torch.Tensor):
            t = t.to(device=dev, dtype=dtype).contiguous()
        else:
            t = torch.from_numpy(np.ascontiguousarray(t, dtype={torch.float32: np.float32, torch.float64: np.float64}[dtype])).to(dev)
        if tuple(t.shape) != shape:
            raise ValueError(f"modelnet_pairs: {name} {tuple(t.shape)} for {nb} pairs")
        return t
    transform = host_or_dev(transform, torch.float32, (nb, 3, 4), "transform")
    dirs = host_or_dev(dirs, torch.float64, (nb, 2, 3), "dirs")
    pk_dev = None
    if pair_keys is not None:
        pk_dev = torch.empty((nb,), dtype=torch.int64, device=dev)
        pk_dev.copy_(torch.from_numpy(_pair_keys(pair_keys, nb, "modelnet_pairs").view(np.int64)))
    elif rkeys is None or extra is None or noise is None or skeys is None:
        raise ValueError("modelnet_pairs: pair_keys are needed when draws are generated inline")
    nk = nb * max(k, 0)
    for name, t, numel in (("rkeys", rkeys, 2 * n_total), ("extra", extra, 2 * nk), ("noise", noise, 6 * nk),
                           ("skeys", skeys, 2 * nk)):
        if t is not None and t.numel() != numel:
            raise ValueError(f"modelnet_pairs: {name} holds {t.numel()} values, expected {numel}")
    rkeys = None if rkeys is None else _dev(rkeys, "rkeys", torch.int32)
    extra = None if extra is None else _dev(extra, "extra", torch.int32)
    noise = None if noise is None else _dev(noise, "noise", torch.float32)
    skeys = None if skeys is None else _dev(skeys, "skeys", torch.int32)
    L = _lib.lib()
    ws = ops._workspace(L.spr_modelnet_pairs_workspace_size(n_total, nb, k), dev)
    o_src = torch.empty((nk, 3), dtype=torch.float32, device=dev)
    o_tgt = torch.empty((nk, 3), dtype=torch.float32, device=dev)
    o_pose = torch.empty((nb, 3, 4), dtype=torch.float32, device=dev)
    o_sov = torch.empty((nk,), dtype=torch.uint8, device=dev)
    o_tov = torch.empty((nk,), dtype=torch.uint8, device=dev)
    o_sidx = torch.empty((nk,), dtype=torch.int32, device=dev)
    o_tidx = torch.empty((nk,), dtype=torch.int32, device=dev)
    o_corr = torch.empty((2, nk), dtype=torch.int32, device=dev)
    o_cnt = torch.zeros((nb,), dtype=torch.int32, device=dev)
    status = torch.zeros((nb,), dtype=torch.int32, device=dev)
    _lib.check(L.spr_modelnet_pairs(
        _ptr(xyz), _ptr(cu), n_total, nb, int(max_len), p_src, p_tgt, percentile_q(p_src), percentile_q(p_tgt), k,
        float(scale), float(clip), _ptr(transform), _ptr(dirs), int(seed), _ptr(pk_dev), _ptr(rkeys), _ptr(extra),
        _ptr(noise), _ptr(skeys), _ptr(o_src), _ptr(o_tgt), _ptr(o_pose), _ptr(o_sov), _ptr(o_tov), _ptr(o_sidx),
        _ptr(o_tidx), _ptr(o_corr), _ptr(o_cnt), _ptr(status), _ptr(ws), ws.numel(), _stream(xyz)), "spr_modelnet_pairs")
    return {'src_xyz': o_src, 'tgt_xyz': o_tgt, 'pose': o_pose, 'src_overlap': o_sov.view(torch.bool),
            'tgt_overlap': o_tov.view(torch.bool), 'src_index': o_sidx, 'tgt_index': o_tidx, 'corr': o_corr,
            'corr_count': o_cnt, 'status': status}


def make_pairs(points, cfg, seed: int, keys, normals: bool = False) -> dict:
    """The reference's ModelNet training transform on a batch of raw shapes: points [B, n, 3|6] or a list of [n_i, 3|6]
    device tensors (columns 3:6, the dataset's normals, are ignored unless normals=True), cfg = get_config('modelnet')
    (partial, num_points, noise_type, rot_mag, trans_mag), keys [B] (ints below 2^63, e.g. dataset index + epoch *
    dataset size) and seed select the draws.
    Returns the collate_pair dict Trainer.train_step accepts: src_xyz / tgt_xyz (lists of [k,3]), pose [B,3,4]
    (source -> reference), src_overlap / tgt_overlap (lists of bool [k]), correspondences (list of [2,K] int64), idx
    (the keys) and src_index / tgt_index (lists: the raw row of every output point).  One library call for all pairs
    and one small device-to-host read (per-pair status and correspondence counts).
    normals=True (6-column shapes only) adds src_point_feats / tgt_point_feats, lists of [k, 4] = [1, nx, ny, nz] (the
    in_feats_dim = 4 input): the raw normals of rows src_index / tgt_index, the source's rotated by the rotation of the
    drawn transform as RandomTransformSE3.apply_transform does (modelnet_transforms.py:287-288), the reference's
    untouched; one normals.gather_rotate call per side.  Every other entry is what normals=False returns."""
    noise_type = cfg.get('noise_type', 'crop')
    if noise_type != 'crop':
        raise NotImplementedError(f"make_pairs: noise_type {noise_type!r}; only 'crop' builds a pair with overlap masks")
    raw_normals = None
    if isinstance(points, torch.Tensor):                     # [B, n, 3|6]: one slice, no per-shape work
        if points.dim() != 3:
            raise ValueError(f"make_pairs: points {tuple(points.shape)}, expected [B, n, 3|6]")
        if normals and points.shape[2] != 6:
            raise ValueError(f"make_pairs: normals=True needs [B, n, 6] shapes, got {tuple(points.shape)}")
        nb, lens = int(points.shape[0]), [int(points.shape[1])] * int(points.shape[0])
        xyz = _dev(points, "points")[:, :, :3].reshape(-1, 3).to(torch.float32)
        if normals:
            raw_normals = _dev(points, "points")[:, :, 3:6].reshape(-1, 3).to(torch.float32)
    else:
        clouds = list(points)
        if normals and any(c.dim() != 2 or c.shape[1] != 6 for c in clouds):
            raise ValueError("make_pairs: normals=True needs [n, 6] shapes")
        nb, lens = len(clouds), [int(c.shape[0]) for c in clouds]
        xyz = torch.cat([_dev(c, "points")[:, :3] for c in clouds]).to(torch.float32) if clouds else None
        if normals and clouds:
            raw_normals = torch.cat([_dev(c, "points")[:, 3:6] for c in clouds]).to(torch.float32)
    pk = _pair_keys(keys, nb, "make_pairs")
    if nb == 0:
        raise ValueError("make_pairs: no shapes")
    dev = xyz.device
    k = output_size(cfg)
    p_keep = (float(cfg.partial[0]), float(cfg.partial[0]))      # both crops take partial[0] (modelnet_transforms.py:217)
    dirs, tf = modelnet_draw(seed, pk, float(cfg.rot_mag), float(cfg.trans_mag))
    r = modelnet_pairs(xyz, lengths_to_cu(lens, dev), max(lens), p_keep, k, tf, dirs, seed=seed, pair_keys=pk)
    host = torch.cat([r['status'], r['corr_count']]).tolist()
    if any(host[:nb]):
        bad = {b: host[b] for b in range(nb) if host[b]}
        raise RuntimeError(f"spr_modelnet_pairs: pairs without points {bad} (status 1: non-finite input, 2: a side is "
                           "empty after the crop)")
    corr64 = r['corr'].long()
    feats = {}
    if normals:
        from . import normals as _normals
        packed = torch.cat([torch.ones((raw_normals.shape[0], 1), dtype=torch.float32, device=dev), raw_normals], dim=1)
        base = torch.from_numpy(np.repeat(np.concatenate([[0], np.cumsum(lens)])[:nb], k).astype(np.int32)).to(dev)
        cu_out = lengths_to_cu([k] * nb, dev)
        eye = np.broadcast_to(np.eye(3, dtype=np.float32), (nb, 3, 3))
        for side, rot in (('src', tf[:, :, :3]), ('tgt', eye)):
            moved = _normals.gather_rotate(packed, r[f'{side}_index'] + base, cu_out, rot, (1,))
            feats[f'{side}_point_feats'] = list(torch.split(moved, k))
    return {
        **feats,
        'src_xyz': list(torch.split(r['src_xyz'], k)), 'tgt_xyz': list(torch.split(r['tgt_xyz'], k)), 'pose': r['pose'],
        'src_overlap': list(torch.split(r['src_overlap'], k)), 'tgt_overlap': list(torch.split(r['tgt_overlap'], k)),
        'correspondences': [corr64[:, b * k:b * k + host[nb + b]] for b in range(nb)],
        'idx': torch.from_numpy(pk.view(np.int64).copy()),
        'src_index': list(torch.split(r['src_index'], k)), 'tgt_index': list(torch.split(r['tgt_index'], k)),
    }
