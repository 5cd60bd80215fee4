"""Surface normals as per-point input features (include/spr.h, "surface normals"; csrc/normals.hip).

estimate / from_neighbors: PCA normals (and, on request, the surface variation l0 / trace) from the rows of a radius
search, oriented towards a per-cloud viewpoint or, without one, so that the component of largest magnitude is positive.
point_feats: the `in_feats_dim = 4` encoder input [1, nx, ny, nz] per cloud.
gather_rotate: a row gather over packed per-point features that rotates direction-valued column triples by the
rotation of the output row's cloud -- what augment.augment_batch and modelnet.make_pairs do to normals.
Everything runs in libspr_hip.so; the package's top-level modules call this subpackage only.
"""
import ctypes
from typing import Optional, Sequence

import numpy as np
import torch

from .. import _lib, ops

MAX_TRIPLES = 4
DEFAULT_LIMIT = 40


def _cu(cu_or_lens, n: int, dev) -> torch.Tensor:
    """cu int32 [nb+1] on the device from a cu tensor or from per-cloud lengths (a host sequence)."""
    if isinstance(cu_or_lens, torch.Tensor) and cu_or_lens.is_cuda:
        return ops._dev(cu_or_lens, "cu", torch.int32)
    lens = [int(x) for x in (cu_or_lens.tolist() if isinstance(cu_or_lens, torch.Tensor) else cu_or_lens)]
    if sum(lens) != n or any(x < 0 for x in lens):
        raise ValueError(f"normals: lengths {lens} do not add up to the {n} points")
    return ops.lengths_to_cu(lens, dev)


def _check_points(points) -> None:
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"normals: points {tuple(points.shape) if isinstance(points, torch.Tensor) else type(points)}, "
                         "expected [N, 3]")


def _viewpoints(viewpoint, nb: int, dev) -> Optional[torch.Tensor]:
    if viewpoint is None:
        return None
    v = viewpoint if isinstance(viewpoint, torch.Tensor) else torch.as_tensor(np.asarray(viewpoint, dtype=np.float32))
    if v.numel() != 3 * nb:
        raise ValueError(f"normals: {v.numel() / 3:g} viewpoints for {nb} clouds")
    return None if dev is None else v.to(device=dev, dtype=torch.float32).reshape(-1, 3).contiguous()


def from_neighbors(points: torch.Tensor, nbr: torch.Tensor, cu: Optional[torch.Tensor] = None, viewpoint=None,
                   curvature: bool = False):
    """spr_estimate_normals on a neighbour matrix the caller already has.  points [N, 3] f32 packed; nbr [N, K] int32,
    global rows of `points`, any entry outside [0, N) a shadow (the matrix ops.radius_neighbors(points, points, cu, cu,
    r, limit) returns; a column slice of a wider matrix is taken as it is, without a copy); viewpoint [nb, 3] with
    cu int32 [nb+1], or None.  Returns normals [N, 3] f32, or (normals, curvature [N] f32).  No device-to-host read."""
    _check_points(points)
    if not isinstance(nbr, torch.Tensor) or nbr.dim() != 2 or nbr.shape[0] != points.shape[0]:
        raise ValueError(f"normals: nbr {tuple(nbr.shape) if isinstance(nbr, torch.Tensor) else type(nbr)} for "
                         f"{points.shape[0]} points, expected [N, K]")
    if viewpoint is not None and cu is None:
        raise ValueError("normals: a viewpoint per cloud needs cu")
    points = ops._dev(points, "points", torch.float32)
    n, dev = int(points.shape[0]), points.device
    if not nbr.is_cuda or nbr.dtype != torch.int32:
        raise RuntimeError("normals: nbr must be an int32 tensor on the MI355X device; the HIP path has no CPU fallback")
    kmax = int(nbr.shape[1])
    if n and kmax and (nbr.stride(1) != 1 or nbr.stride(0) < kmax):
        nbr = nbr.contiguous()
    stride = int(nbr.stride(0)) if n and kmax else kmax
    view = None
    if viewpoint is not None:
        cu = ops._dev(cu, "cu", torch.int32)
        view = _viewpoints(viewpoint, cu.numel() - 1, dev)
    nb = 0 if cu is None else cu.numel() - 1
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    curv = torch.empty((n,), dtype=torch.float32, device=dev) if curvature else None
    _lib.check(_lib.lib().spr_estimate_normals(ops._ptr(points), ops._ptr(cu), n, nb, ops._ptr(nbr), stride, kmax,
                                               ops._ptr(view), ops._ptr(out), ops._ptr(curv), ops._stream(points)),
               "spr_estimate_normals")
    return (out, curv) if curvature else out


def estimate(points: torch.Tensor, cu_or_lens, radius: float, limit: int = DEFAULT_LIMIT, viewpoint=None,
             curvature: bool = False):
    """Normals of packed clouds from their own radius search: ops.radius_neighbors(points, points, cu, cu, radius,
    limit) -- the `limit` nearest in range, the point itself among them; its one device-to-host read, the max count,
    is the only one, and is kept because it also carries the search's status (a geometry its cell table cannot hold
    is searched again by the other algorithm) -- then from_neighbors on the rows as they come back.  cu_or_lens: cu int32 [nb+1] on the device or
    the per-cloud lengths.  A point with fewer than 3 neighbours in range (itself included) gets the zero normal."""
    _check_points(points)
    nb = (cu_or_lens.numel() - 1) if isinstance(cu_or_lens, torch.Tensor) and cu_or_lens.is_cuda else len(cu_or_lens)
    if viewpoint is not None:                                         # refused before anything touches the device
        _viewpoints(viewpoint, nb, None)
    points = ops._dev(points, "points", torch.float32)
    n = int(points.shape[0])
    cu = _cu(cu_or_lens, n, points.device)
    view = _viewpoints(viewpoint, nb, points.device)
    if n == 0:
        nbr = torch.empty((0, int(limit)), dtype=torch.int32, device=points.device)
    else:
        nbr, _ = ops.radius_neighbors(points, points, cu, cu, float(radius), int(limit))
    return from_neighbors(points, nbr, cu, view, curvature)


def point_feats(clouds: Sequence[torch.Tensor], radius: float, limit: int = DEFAULT_LIMIT, viewpoints=None,
                extra: Optional[Sequence[torch.Tensor]] = None):
    """The encoder's per-point input for `in_feats_dim = 4 (+ E)`: one [n_i, 4 + E] tensor [1, extra.., nx, ny, nz] per
    cloud ([n_i, 3] device tensors).  extra: one [n_i, E] (or [n_i]) tensor of scalar columns per cloud; they go before
    the normal, so the normal's triple starts at column 1 + E.  One radius search and one kernel for all clouds."""
    clouds = list(clouds)
    if not clouds:
        return []
    lens = [int(c.shape[0]) for c in clouds]
    pts = torch.cat([ops._dev(c, "clouds", torch.float32).reshape(-1, 3) for c in clouds])
    nrm = estimate(pts, lens, radius, limit, viewpoints)
    cols = [torch.ones((pts.shape[0], 1), dtype=torch.float32, device=pts.device)]
    if extra is not None:
        extra = list(extra)
        if len(extra) != len(clouds) or any(int(e.shape[0]) != n for e, n in zip(extra, lens)):
            raise ValueError("normals.point_feats: extra must be one [n, E] tensor per cloud, row-aligned with it")
        cols.append(torch.cat([ops._dev(e, "extra", torch.float32).reshape(n, -1) for e, n in zip(extra, lens)]))
    return list(torch.split(torch.cat(cols + [nrm], dim=1), lens))


def check_direction_cols(direction_cols, c: int) -> list:
    """The start columns of the direction triples of a [., c] feature matrix, validated: at most MAX_TRIPLES, each
    inside the row, none overlapping."""
    cols = [int(x) for x in direction_cols]
    if len(cols) > MAX_TRIPLES:
        raise ValueError(f"direction_cols: {len(cols)} triples, at most {MAX_TRIPLES}")
    for i, s in enumerate(cols):
        if s < 0 or s + 3 > c:
            raise ValueError(f"direction_cols: the triple at column {s} runs past the {c} feature columns")
        if any(abs(s - t) < 3 for t in cols[:i]):
            raise ValueError(f"direction_cols: overlapping triples in {cols}")
    return cols


def gather_rotate(feats: torch.Tensor, rows: torch.Tensor, cu_out: torch.Tensor, rot, direction_cols=()) -> torch.Tensor:
    """spr_feats_gather_rotate: out[r] = feats[rows[r]] with every triple of columns (s, s+1, s+2), s in direction_cols,
    rotated by rot[b], b the cloud of output row r under cu_out (int32 [nb+1] over the output rows).  feats [n_in, C]
    f32; rows [n_out] integer, global rows of feats; rot [nb, 3, 3] (tensor or host array).  Component k of a rotated
    triple is f32((R_k0 x + R_k1 y) + R_k2 z) evaluated in float64; directions are not renormalised.  With no triple
    listed this is feats.index_select(0, rows), bit for bit."""
    if not isinstance(feats, torch.Tensor) or feats.dim() != 2 or feats.shape[1] < 1:
        raise ValueError(f"gather_rotate: feats {tuple(feats.shape) if isinstance(feats, torch.Tensor) else type(feats)}, "
                         "expected [n, C]")
    cols = check_direction_cols(direction_cols, int(feats.shape[1]))
    feats = ops._dev(feats, "feats", torch.float32)
    dev, c = feats.device, int(feats.shape[1])
    rows = ops._dev(rows, "rows", torch.int32).reshape(-1)
    cu_out = ops._dev(cu_out, "cu_out", torch.int32)
    nb, n_out = cu_out.numel() - 1, int(rows.shape[0])
    if not isinstance(rot, torch.Tensor):
        rot = torch.from_numpy(np.ascontiguousarray(rot, dtype=np.float32))
    rot = rot.to(device=dev, dtype=torch.float32).contiguous()
    if tuple(rot.shape) != (nb, 3, 3):
        raise ValueError(f"gather_rotate: rot {tuple(rot.shape)} for {nb} clouds, expected [{nb}, 3, 3]")
    out = torch.empty((n_out, c), dtype=torch.float32, device=dev)
    host_cols = (ctypes.c_int * MAX_TRIPLES)(*cols)
    _lib.check(_lib.lib().spr_feats_gather_rotate(ops._ptr(feats), int(feats.shape[0]), c, ops._ptr(rows), n_out,
                                                  ops._ptr(cu_out), nb, ops._ptr(rot), host_cols, len(cols),
                                                  ops._ptr(out), ops._stream(feats)), "spr_feats_gather_rotate")
    return out
