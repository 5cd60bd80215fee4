"""Grid subsampling that carries per-point features and labels through the voxel grid (include/spr.h, "a1 with
attributes"): the counterpart of cpp_subsampling.subsample_batch(points, batches, features=, classes=) behind
models/backbone_kpconv/kpconv.py:187-214.  Features come back as the voxel's float32 average, labels as its majority
vote with the reference's tie rule; points and lengths are those of ops.grid_subsample, bit for bit.

Labels with more than one column in a batch of more than one cloud: the reference slices its class vector wrongly
there (grid_subsampling.cpp:157-158, undefined behaviour); this module votes per cloud, row i of `labels` belonging to
point i."""
import torch

from .. import _lib, ops


def grid_subsample(points: torch.Tensor, cu: torch.Tensor, dl: float, max_p: int = 0, order: int = ops.ORDER_REFERENCE,
                   features: torch.Tensor = None, labels: torch.Tensor = None):
    """Returns (sub_points [M, 3] f32, sub_lens [nb] i32[, sub_features [M, fdim] f32][, sub_labels]) on the device.
    features [N, fdim] float32; labels [N] or [N, ldim], int32 or int64 (int64 values must fit int32, the reference's
    class type): sub_labels has the rank and dtype of `labels`.  One device->host read of the output size."""
    points = ops._dev(points, "points", torch.float32)
    cu = ops._dev(cu, "cu", torch.int32)
    n, nb = points.shape[0], cu.numel() - 1
    dev = points.device
    feat = lab = out_feat = out_lab = None
    fdim = ldim = 0
    if features is not None:
        feat = ops._dev(features, "features", torch.float32)
        if feat.dim() != 2 or feat.shape[0] != n:
            raise RuntimeError(f"features.shape is not (N, d): {tuple(feat.shape)} for {n} points")
        fdim = feat.shape[1]
        out_feat = torch.empty((max(n, 1), fdim), dtype=torch.float32, device=dev)
    if labels is not None:
        if not isinstance(labels, torch.Tensor) or labels.dtype not in (torch.int32, torch.int64):
            raise RuntimeError("labels must be an int32 or int64 tensor")
        lab = ops._dev(labels, "labels", torch.int32)
        if lab.dim() not in (1, 2) or lab.shape[0] != n:
            raise RuntimeError(f"labels.shape is not (N,) or (N, d): {tuple(lab.shape)} for {n} points")
        ldim = 1 if lab.dim() == 1 else lab.shape[1]
        out_lab = torch.empty((max(n, 1), ldim), dtype=torch.int32, device=dev)
    L = _lib.lib()
    ws = ops._workspace(L.spr_grid_subsample_attrs_workspace_size(n, nb, fdim, ldim), dev)
    out = torch.empty((max(n, 1), 3), dtype=torch.float32, device=dev)
    out_lens = torch.empty((nb,), dtype=torch.int32, device=dev)
    total = torch.empty((1,), dtype=torch.int32, device=dev)
    _lib.check(L.spr_grid_subsample_attrs(ops._ptr(points), ops._ptr(cu), n, nb, float(dl), int(max_p), int(order),
                                          ops._ptr(feat) if fdim else None, fdim, ops._ptr(lab) if ldim else None, ldim,
                                          ops._ptr(out), ops._ptr(out_feat) if fdim else None,
                                          ops._ptr(out_lab) if ldim else None, ops._ptr(out_lens), ops._ptr(total),
                                          ops._ptr(ws), ws.numel(), ops._stream(points)), "spr_grid_subsample_attrs")
    m = int(total.item())
    if m < 0:
        raise RuntimeError("spr_grid_subsample_attrs: voxel grid too large for 40-bit keys")
    res = [out[:m], out_lens]
    if features is not None:
        res.append(out_feat[:m])
    if labels is not None:
        sub = out_lab[:m, 0] if labels.dim() == 1 else out_lab[:m]
        res.append(sub.to(labels.dtype).contiguous())
    return tuple(res)
