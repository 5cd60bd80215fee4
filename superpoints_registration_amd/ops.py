"""Tensor-level wrappers over the C ABI (include/spr.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream;
every computation below happens in libspr_hip.so.  Inputs must be CUDA(HIP)
tensors -- a CPU tensor raises, there is no fallback.
"""
import ctypes
import math
import threading
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2
ORDER_REFERENCE, ORDER_CANONICAL = 0, 1
# which `limit` supports in range a neighbour row keeps (SPR_SELECT_*): the nearest (the reference's CPU Preprocessor)
# or the lowest indices (its PreprocessorGPU: pytorch3d.ops.ball_query)
SELECT_NEAREST, SELECT_INDEX = 0, 1


def _stream(t: torch.Tensor):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(t: torch.Tensor, name: str, dtype=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a tensor on the MI355X device (got "
                           f"{t.device if isinstance(t, torch.Tensor) else type(t)}); "
                           "the HIP path has no CPU fallback")
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


_ws_cache = {}


# ---- operand-range hand-over (include/spr.h, "Operand-range hand-over") ------------------------
# A producer kernel that has just written a tensor can publish max |x| as a few per-workgroup
# partials; the consuming GEMM then scales its operand without a measuring pass over x.  The
# range rides on the Python tensor object as an attribute and is honoured only while the tensor
# is untouched (same storage pointer, same version counter): views, copies and in-place edits drop it.
_range_epoch = [0]


def invalidate_ranges() -> None:
    """Drops every cached / published operand range.  Needed only after mutating a tensor behind
    autograd's back (`w.data.copy_(...)`, raw pointer writes): such edits do not move the version
    counter the ranges are keyed on."""
    _range_epoch[0] += 1


def _ident(t: torch.Tensor):
    """What everything derived from a tensor is keyed on: the derived value holds while the tensor keeps its
    storage pointer and version counter and invalidate_ranges() has not been called."""
    return (t.data_ptr(), t._version, _range_epoch[0])


def _set_range(t: torch.Tensor, parts: torch.Tensor, n: int, guard=None) -> None:
    if n > 0:     # ONE attribute store: a reader on another thread sees the range and its guard together
        ptr, version, epoch = _ident(t)
        t._spr_range = (parts, int(n), version, ptr, epoch, guard)


def _get_range(t):
    r = getattr(t, '_spr_range', None)
    if r is None or (r[3], r[2], r[4]) != _ident(t):
        return None, 0
    if r[5] is not None:
        r[5].acquire()
    return r[0], r[1]


def share_range(src: torch.Tensor, alias: torch.Tensor) -> None:
    """Hands the range attached to src to `alias`, a detached view of it: with the same storage and version
    counter the measurement still holds, and _get_range(alias) drops it like src's own once either is edited."""
    r = getattr(src, '_spr_range', None)
    if r is not None and alias is not src:
        alias._spr_range = r


_RANGE_CAP = 4096   # partials a GEMM may publish (one per workgroup)
_STREAM_SLOTS = 512  # atomic-max slots of the streaming producers (InstanceNorm apply, max-pool)
_zero_pool = {}


def _stream_key(device):
    """Key of the per-(device, current stream) pools: their buffers are reused in stream order."""
    return (device, torch.cuda.current_stream(device).cuda_stream)


def _zero_slots(n: int, device) -> torch.Tensor:
    """n zero-initialised floats from a per-(device, stream) pool: one memset per 256 K slots instead
    of one per LayerNorm call (its range slots are combined with atomic max and must start at 0)."""
    key = _stream_key(device)
    pool = _zero_pool.get(key)
    if pool is None or pool[1] + n > pool[0].numel():
        pool = [torch.zeros(1 << 18, dtype=torch.float32, device=device), 0]
        _zero_pool[key] = pool
    out = pool[0][pool[1]:pool[1] + n]
    pool[1] += n
    return out


class _StreamGuard:
    """Ordering of a cached, weight-side measurement against consumers on OTHER streams.  The
    measuring kernel runs on the stream of the thread that first needed it; the cache lives on the
    shared Parameter, and StreamedForward threads / the side streams of one forward read it from
    their own streams.  The producing stream records an event behind the measurement; the first
    consumer on any other stream waits for it (and registers the buffer with its stream)."""

    def __init__(self, buf: torch.Tensor):
        self.stream = torch.cuda.current_stream(buf.device)
        self.event = torch.cuda.Event()
        self.event.record(self.stream)
        self.buf = buf
        self.seen = {self.stream.cuda_stream}

    def acquire(self):
        cur = torch.cuda.current_stream(self.buf.device)
        if cur.cuda_stream not in self.seen:
            cur.wait_event(self.event)
            self.buf.record_stream(cur)
            self.seen.add(cur.cuda_stream)


def _derived(src: torch.Tensor, slot: str, extra, build):
    """The one cache rule of this file.  The value derived from `src` and kept on it as attribute `slot` is returned
    while `src` is untouched (_ident) and `extra`, the call arguments it depends on, is the same; otherwise build()
    launches it on the current stream and returns (value, tensor to guard).  Readers on other streams wait for that
    launch (_StreamGuard).  Stored as (key, value, guard) in ONE attribute store, like _set_range."""
    key = (_ident(src), extra)
    c = getattr(src, slot, None)
    if c is not None and c[0] == key:
        c[2].acquire()
        return c[1]
    value, buf = build()
    setattr(src, slot, (key, value, _StreamGuard(buf)))
    return value


def _measure_range(t: torch.Tensor, guarded: bool):
    """Measures max |t| over the rows of t (spr_absmax) and attaches it like a published range; guarded for readers
    on other streams when t outlives the call on a shared object (a weight)."""
    L = _lib.lib()
    n = L.spr_range_parts()
    flat = t.reshape(-1, t.shape[-1])
    parts = torch.empty((n,), dtype=torch.float32, device=t.device)
    _lib.check(L.spr_absmax(_ptr(flat), flat.shape[0], flat.shape[1], flat.shape[1], _ptr(parts), _stream(t)),
               "spr_absmax")
    _set_range(t, parts, n, _StreamGuard(parts) if guarded else None)
    return parts, n


def _static_range(w: torch.Tensor):
    """Range partials of a tensor that rarely changes (weights): measured once per (storage,
    version) with spr_absmax and kept on the tensor like a published range -- an optimizer step
    bumps the version counter and the next call measures again."""
    r, n = _get_range(w)
    return (r, n) if r is not None else _measure_range(w, True)


_PRIME_PARTS = 16


def prime_weight_ranges(params) -> int:
    """Measures the ranges of all (float32, contiguous, device) parameters whose cached range is stale in ONE launch
    (spr_absmax_multi) and attaches them like _static_range would: after an optimizer step every weight's version
    counter has moved, and ~150 separate measuring launches (16 us each) opened every training forward.  Returns the
    number of tensors measured."""
    todo = [p for p in params if isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.float32
            and p.dim() >= 2 and p.is_contiguous() and p.numel() > 0 and _get_range(p)[0] is None]
    if not todo:
        return 0
    dev = todo[0].device
    todo = [p for p in todo if p.device == dev]
    rec = np.zeros((len(todo), 2), dtype=np.int64)
    for i, p in enumerate(todo):
        rec[i, 0] = p.data_ptr()
        rec[i, 1] = p.numel()
    jobs = torch.from_numpy(rec).to(dev)
    parts = torch.empty((len(todo), _PRIME_PARTS), dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().spr_absmax_multi(_ptr(jobs), len(todo), _PRIME_PARTS, _ptr(parts), _stream(parts)),
               "spr_absmax_multi")
    guard = _StreamGuard(parts)
    for i, p in enumerate(todo):
        _set_range(p, parts[i], _PRIME_PARTS, guard)
    return len(todo)


def weight_transposed(w: torch.Tensor) -> torch.Tensor:
    """Contiguous W^T of a [n, k] weight, kept on the tensor per (storage, version) like its range (the
    backward's dX = g W runs as the forward's NT product on it); guarded for readers on other streams."""
    def build():
        wt = w.detach().t().contiguous()
        # max |W^T| = max |W|: the copy shares the weight's measured range, and that measurement's guard, unscanned
        r, n = _static_range(w)
        _set_range(wt, r, n, w._spr_range[5])
        return wt, wt
    return _derived(w, '_spr_wt', None, build)


def ensure_range(t: torch.Tensor) -> torch.Tensor:
    """Measures max |t| once (spr_absmax) and publishes it on the tensor like a producer kernel would, unless a
    valid range is already attached: a gradient that feeds two products (dX and dW of a projection) is then
    scanned once instead of once per product."""
    if t.dim() == 2 and t.is_contiguous() and _get_range(t)[0] is None:
        _measure_range(t, False)
    return t


def _workspace(nbytes: int, device) -> torch.Tensor:
    """Grow-only scratch buffer per device+stream (stream-ordered reuse)."""
    key = _stream_key(device)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def lengths_to_cu(lengths, device) -> torch.Tensor:
    """int32 [nb+1] exclusive prefix of the per-cloud lengths."""
    if isinstance(lengths, torch.Tensor):
        l = lengths.to(device=device, dtype=torch.int32)
        cu = torch.zeros(l.numel() + 1, dtype=torch.int32, device=device)
        cu[1:] = torch.cumsum(l, 0)
        return cu
    arr = np.zeros(len(lengths) + 1, dtype=np.int32)
    arr[1:] = np.cumsum(np.asarray(lengths, dtype=np.int64))
    return torch.from_numpy(arr).to(device)


# --------------------------------------------------------------------------- #
def selftest() -> None:
    st = ctypes.c_int(-1)
    _lib.check(_lib.lib().spr_selftest(ctypes.byref(st)), "spr_selftest")


def grid_subsample(points: torch.Tensor, cu: torch.Tensor, dl: float, max_p: int = 0,
                   order: int = ORDER_REFERENCE) -> Tuple[torch.Tensor, torch.Tensor]:
    """a1.  Returns (sub_points [N',3] f32, lengths [nb] i32 on device).
    One device->host read of the output size (the reference returns exact
    shapes too)."""
    points = _dev(points, "points", torch.float32)
    cu = _dev(cu, "cu", torch.int32)
    n, nb = points.shape[0], cu.numel() - 1
    L = _lib.lib()
    ws = _workspace(L.spr_grid_subsample_workspace_bytes(n, nb), points.device)
    out = torch.empty((max(n, 1), 3), dtype=torch.float32, device=points.device)
    out_lens = torch.empty((nb,), dtype=torch.int32, device=points.device)
    total = torch.empty((1,), dtype=torch.int32, device=points.device)
    _lib.check(L.spr_grid_subsample(_ptr(points), _ptr(cu), n, nb, float(dl), int(max_p), int(order),
                                    _ptr(out), _ptr(out_lens), _ptr(total), _ptr(ws), ws.numel(),
                                    _stream(points)), "spr_grid_subsample")
    m = int(total.item())
    if m < 0:
        raise RuntimeError("spr_grid_subsample: voxel grid too large for 40-bit keys")
    return out[:m], out_lens


def voxel_downsample(points: torch.Tensor, voxel_size: float) -> torch.Tensor:
    """One point per voxel (the first one, voxel = trunc(p / voxel_size)): the GPU counterpart of
    the KITTI loader's kiss_icp pre-downsampling (kitti_pred.py:12-14, :203-204).  Returns the kept
    points in ascending original index (one device->host read of the count)."""
    points = _dev(points, "points", torch.float32)
    n = points.shape[0]
    L = _lib.lib()
    ws = _workspace(L.spr_voxel_downsample_workspace_bytes(n), points.device)
    idx = torch.empty((n,), dtype=torch.int32, device=points.device)
    cnt = torch.empty((1,), dtype=torch.int32, device=points.device)
    _lib.check(L.spr_voxel_downsample(_ptr(points), n, float(voxel_size), _ptr(idx), _ptr(cnt), _ptr(ws), ws.numel(),
                                      _stream(points)), "spr_voxel_downsample")
    m = int(cnt.item())
    if m < 0:
        raise RuntimeError("spr_voxel_downsample: coordinates exceed 2^20 voxels")
    return points[idx[:m].long()]


def prepare_scans(points: torch.Tensor, cu: torch.Tensor, voxel_size: float, crop_radius: float = 0.0,
                  remove_ground: bool = False) -> Tuple[torch.Tensor, list, torch.Tensor]:
    """The KITTI loader's point path (kitti_pred.py:203-230) for all raw scans of a batch in one call
    (spr_prepare_scans; the contract is in include/spr.h): first point of every voxel, then the crop to crop_radius
    (<= 0: none) and, with remove_ground, the cut z > -1, both on the filter's output.  points [n, 3 | 4] float32
    packed by cu int32 [nb+1] on the device (4 columns: raw Velodyne records, the 4th is never read).
    Returns (xyz [m,3], out_cu, idx [m] int32): the kept points in ascending original index per cloud, the output's
    cloud boundaries as a host list of nb+1 ints (a cloud may come out empty) and each kept point's index inside its
    own input cloud.  One device->host copy for the whole batch (status and out_cu together)."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] not in (3, 4):
        raise ValueError(f"prepare_scans: points must be [n, 3] or [n, 4], got "
                         f"{tuple(points.shape) if isinstance(points, torch.Tensor) else type(points)}")
    points = _dev(points, "points", torch.float32)
    cu = _dev(cu, "cu", torch.int32).reshape(-1)
    n, stride, nb = points.shape[0], points.shape[1], cu.numel() - 1
    if n < 1 or nb < 1 or nb > n:
        raise ValueError(f"prepare_scans: {n} points in {nb} clouds; every cloud holds at least one point")
    L = _lib.lib()
    dev = points.device
    # scratch by torch.empty, not the shared workspace: the table alone is 8 bytes per point of the whole batch
    scratch = torch.empty((L.spr_prepare_scans_scratch_len(n, nb),), dtype=torch.int32, device=dev)
    xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
    idx = torch.empty((n,), dtype=torch.int32, device=dev)
    tail = torch.empty((nb + 2,), dtype=torch.int32, device=dev)      # out_cu [nb+1], then the status word
    _lib.check(L.spr_prepare_scans(_ptr(points), stride, _ptr(cu), n, nb, float(voxel_size), float(crop_radius),
                                   int(bool(remove_ground)), _ptr(scratch), scratch.numel(), _ptr(xyz), _ptr(idx),
                                   _ptr(tail), ctypes.c_void_p(tail.data_ptr() + 4 * (nb + 1)), _stream(points)),
               "spr_prepare_scans")
    host = tail.tolist()
    out_cu, status = host[:nb + 1], host[nb + 1]
    if status == -1:
        raise RuntimeError("spr_prepare_scans: coordinates exceed 2^20 voxels (or are not finite)")
    if status != 0:
        raise RuntimeError("spr_prepare_scans: " + ("a point found no slot in its cloud's table" if status == -2 else
                                                    "cu is not an ascending prefix from 0 to the number of points")
                           + f" (status {status})")
    m = out_cu[nb]
    return xyz[:m], out_cu, idx[:m]


def radius_neighbors(queries: torch.Tensor, supports: torch.Tensor, q_cu: torch.Tensor,
                     s_cu: torch.Tensor, radius: float, limit: int,
                     exact_width: bool = True, algo: int = 0,
                     select: int = SELECT_NEAREST, tie_order: str = 'index') -> Tuple[torch.Tensor, int]:
    """a2.  int32 [Nq, W] neighbour indices (shadow = Ns) and the untruncated
    max count.  exact_width=True slices to W = min(max_count, limit) like the
    reference (one device->host read); False keeps W = limit (no sync).
    select=SELECT_INDEX keeps the `limit` lowest support indices in range, ascending, instead of the `limit`
    nearest (the reference's batch_neighbors_kpconv_gpu, kpconv.py:265-292): W = limit always, and a search
    without a single neighbour is not an error there.
    tie_order='reference' (nearest rule, exact_width only): equal-d2 runs in the order the reference's kd-tree search
    and std::sort leave them in instead of by index (tie_order.py); the default rows, bits and launches are unchanged."""
    if tie_order != 'index':
        from . import tie_order as _tie
        _tie.check(tie_order, select)
        if not exact_width:
            raise ValueError("tie_order='reference' needs exact_width=True (the fix-up is sized by the max count)")
    queries = _dev(queries, "queries", torch.float32)
    supports = _dev(supports, "supports", torch.float32)
    q_cu = _dev(q_cu, "q_cu", torch.int32)
    s_cu = _dev(s_cu, "s_cu", torch.int32)
    nq, ns, nb = queries.shape[0], supports.shape[0], q_cu.numel() - 1
    L = _lib.lib()
    ws = _workspace(L.spr_radius_neighbors_workspace_bytes(nq, ns, nb), queries.device)
    out = torch.empty((nq, limit), dtype=torch.int32, device=queries.device)
    mc = torch.empty((1,), dtype=torch.int32, device=queries.device)
    _lib.check(L.spr_radius_neighbors(_ptr(queries), _ptr(q_cu), nq, _ptr(supports), _ptr(s_cu), ns,
                                      nb, float(radius), int(limit), int(algo), int(select), _ptr(out),
                                      _ptr(mc), _ptr(ws), ws.numel(), _stream(queries)), "spr_radius_neighbors")
    if not exact_width:
        return out, -1
    m = int(mc.item())
    if m == -2 and algo == 0:   # cell table too small for this geometry: exact same result, slower path
        return radius_neighbors(queries, supports, q_cu, s_cu, radius, limit, exact_width, algo=1, select=select,
                                tie_order=tie_order)
    if m < 0:
        raise RuntimeError("spr_radius_neighbors: cloud extent / radius exceeds 8191 cells per axis")
    if select == SELECT_INDEX:  # kpconv.py:284-292: K columns whatever the counts, no emptiness check
        return out, m
    if m < 1:  # cpp_neighbors/wrapper.cpp:201-205
        raise RuntimeError("Error")
    if tie_order != 'index':
        _tie.apply(out[:, :min(m, limit)], queries, q_cu, supports, s_cu, radius, m)
    return out[:, :min(m, limit)], m


def gt_overlap(src_xyz: torch.Tensor, src_cu: torch.Tensor, tgt_xyz: torch.Tensor, tgt_cu: torch.Tensor,
               pose: torch.Tensor, radius: float):
    """8f-5.  Ground-truth overlap labels of all pairs of a batch in one call (spr_gt_overlap; the reference's
    compute_overlap, utils/pointcloud.py:8-65, as a float64 definition -- see include/spr.h).
    src_xyz [sum N,3] / tgt_xyz [sum M,3] packed, src_cu / tgt_cu int32 [B+1], pose [B,3,4] (src -> tgt).
    Returns (src_corr [sum N] i32, tgt_corr [sum M] i32, src_mask [sum N] bool, tgt_mask [sum M] bool,
    corr [2, sum N] i32, corr_count: list of B ints): corr indices are local to the pair, pair b owns columns
    [src_cu[b], src_cu[b] + corr_count[b]).  One device->host read (the counts)."""
    src_xyz = _dev(src_xyz, "src_xyz", torch.float32)
    tgt_xyz = _dev(tgt_xyz, "tgt_xyz", torch.float32)
    src_cu = _dev(src_cu, "src_cu", torch.int32)
    tgt_cu = _dev(tgt_cu, "tgt_cu", torch.int32)
    pose = _dev(pose, "pose", torch.float32)
    ns, nt, nb = src_xyz.shape[0], tgt_xyz.shape[0], src_cu.numel() - 1
    if tgt_cu.numel() - 1 != nb or tuple(pose.shape) != (nb, 3, 4):
        raise ValueError(f"gt_overlap: {nb} source clouds, {tgt_cu.numel() - 1} target clouds, pose {tuple(pose.shape)}")
    dev = src_xyz.device
    L = _lib.lib()
    ws = _workspace(L.spr_gt_overlap_workspace_bytes(ns, nt, nb), dev)
    src_corr = torch.empty((ns,), dtype=torch.int32, device=dev)
    tgt_corr = torch.empty((nt,), dtype=torch.int32, device=dev)
    src_mask = torch.empty((ns,), dtype=torch.uint8, device=dev)
    tgt_mask = torch.empty((nt,), dtype=torch.uint8, device=dev)
    corr = torch.empty((2, ns), dtype=torch.int32, device=dev)
    count = torch.zeros((max(nb, 1),), dtype=torch.int32, device=dev)
    _lib.check(L.spr_gt_overlap(_ptr(src_xyz), _ptr(src_cu), ns, _ptr(tgt_xyz), _ptr(tgt_cu), nt, _ptr(pose), nb,
                                float(radius), _ptr(src_corr), _ptr(tgt_corr), _ptr(src_mask), _ptr(tgt_mask),
                                _ptr(corr), _ptr(count), _ptr(ws), ws.numel(), _stream(src_xyz)), "spr_gt_overlap")
    counts = count[:nb].tolist()
    if any(c < 0 for c in counts):
        raise RuntimeError("spr_gt_overlap: non-finite coordinates or pose")
    return src_corr, tgt_corr, src_mask.view(torch.bool), tgt_mask.view(torch.bool), corr, counts


AUG_MODES = {'none': 0, 'small': 1, 'large': 2}


def philox4x32(counter, key) -> np.ndarray:
    """One Philox4x32-10 block through the library's host path (spr_philox4x32_host): uint32 [4]."""
    c = np.ascontiguousarray(counter, dtype=np.uint32).reshape(4)
    k = np.ascontiguousarray(key, dtype=np.uint32).reshape(2)
    out = np.zeros(4, dtype=np.uint32)
    _lib.check(_lib.lib().spr_philox4x32_host(c.ctypes.data, k.ctypes.data, out.ctypes.data), "spr_philox4x32_host")
    return out


def augment_draw(seed: int, pair_keys, mode: str, src_cu: Optional[torch.Tensor] = None,
                 tgt_cu: Optional[torch.Tensor] = None, ns: int = 0, nt: int = 0):
    """8f-6.  The augmentation draws of pairs `pair_keys` under `seed` (spr_augment_draw; contract in include/spr.h).
    Returns (perturb_src [nb] bool, swap [nb] bool, perturb [nb,3,4] f32) as numpy arrays -- the per-pair
    decisions are host data and need no device.  With src_cu / tgt_cu (device int32 [nb+1]) and the packed sizes ns,
    nt it also returns the device buffers (noise [ns+nt,3] f32, keys [ns+nt] int32 holding the uint32 bit patterns)
    that augment_pairs generates inline when it is not handed them."""
    pk = np.ascontiguousarray(pair_keys, dtype=np.uint64).reshape(-1)
    nb = pk.size
    psrc = np.zeros(nb, dtype=np.uint8)
    swap = np.zeros(nb, dtype=np.uint8)
    perturb = np.zeros((nb, 3, 4), dtype=np.float32)
    L = _lib.lib()
    if src_cu is None:
        _lib.check(L.spr_augment_draw(int(seed), pk.ctypes.data, nb, AUG_MODES[mode], psrc.ctypes.data, swap.ctypes.data,
                                      perturb.ctypes.data, None, None, 0, None, 0, None, None, None), "spr_augment_draw")
        return psrc.astype(bool), swap.astype(bool), perturb
    src_cu = _dev(src_cu, "src_cu", torch.int32)
    tgt_cu = _dev(tgt_cu, "tgt_cu", torch.int32)
    if src_cu.numel() - 1 != nb or tgt_cu.numel() - 1 != nb:
        raise ValueError(f"augment_draw: {nb} pair keys, cu arrays of {src_cu.numel() - 1} / {tgt_cu.numel() - 1} clouds")
    dev = src_cu.device
    pk_dev = torch.from_numpy(pk.view(np.int64)).to(dev)
    noise = torch.empty((ns + nt, 3), dtype=torch.float32, device=dev)
    keys = torch.empty((ns + nt,), dtype=torch.int32, device=dev)
    _lib.check(L.spr_augment_draw(int(seed), pk.ctypes.data, nb, AUG_MODES[mode], psrc.ctypes.data, swap.ctypes.data,
                                  perturb.ctypes.data, _ptr(pk_dev), _ptr(src_cu), int(ns), _ptr(tgt_cu), int(nt),
                                  _ptr(noise), _ptr(keys), _stream(src_cu)), "spr_augment_draw")
    return psrc.astype(bool), swap.astype(bool), perturb, noise, keys


def augment_pairs(src_xyz: torch.Tensor, src_cu: torch.Tensor, tgt_xyz: torch.Tensor, tgt_cu: torch.Tensor,
                  pose: torch.Tensor, perturb_src, swap, perturb, mode: str, scale: float, max_pts: int = 30000,
                  seed: int = 0, pair_keys=None, src_mask: Optional[torch.Tensor] = None,
                  tgt_mask: Optional[torch.Tensor] = None, corr: Optional[torch.Tensor] = None, corr_off=None,
                  corr_count=None, noise: Optional[torch.Tensor] = None, keys: Optional[torch.Tensor] = None,
                  out_lens=None) -> dict:
    """8f-6.  RigidPerturb -> Jitter -> ShufflePoints -> RandomSwap of all pairs of a batch in one call
    (spr_augment_pairs; the float64 contract is in include/spr.h).
    src_xyz [sum N,3] / tgt_xyz [sum M,3] packed with src_cu / tgt_cu int32 [B+1]; pose [B,3,4]; the decisions
    perturb_src / swap ([B] bool) and perturb ([B,3,4] f32) as augment_draw returns them (host arrays or tensors);
    optional masks (bool or uint8, both or neither) and corr [2, W] int32 with per-pair column offsets corr_off and
    counts corr_count ([B] ints; ops.gt_overlap's layout is corr_off = src_cu[:-1]).  noise [sum N + sum M, 3] f32 and
    keys [sum N + sum M] (uint32 patterns in an int32 tensor) are generated inline from (seed, pair_keys) when None.
    out_lens = (src_lens, tgt_lens) of the OUTPUT when the caller has them on the host (see augment.output_lengths).
    Returns a dict of device tensors: src_xyz, tgt_xyz, src_cu, tgt_cu, pose, src_perm, tgt_perm, status [B] and, when
    given, src_mask, tgt_mask (bool), corr [2, W], corr_count [B] (device: the only data-dependent sizes).  No
    device-to-host read happens here."""
    src_xyz = _dev(src_xyz, "src_xyz", torch.float32)
    tgt_xyz = _dev(tgt_xyz, "tgt_xyz", torch.float32)
    src_cu = _dev(src_cu, "src_cu", torch.int32)
    tgt_cu = _dev(tgt_cu, "tgt_cu", torch.int32)
    pose = _dev(pose, "pose", torch.float32)
    dev = src_xyz.device
    ns, nt, nb = src_xyz.shape[0], tgt_xyz.shape[0], src_cu.numel() - 1
    if tgt_cu.numel() - 1 != nb or tuple(pose.shape) != (nb, 3, 4):
        raise ValueError(f"augment_pairs: {nb} source clouds, {tgt_cu.numel() - 1} target clouds, pose {tuple(pose.shape)}")
    flags_h = (np.asarray(perturb_src, dtype=bool).reshape(-1).astype(np.uint8)
               | (np.asarray(swap, dtype=bool).reshape(-1).astype(np.uint8) << 1))
    if flags_h.size != nb:
        raise ValueError(f"augment_pairs: {flags_h.size} decisions for {nb} pairs")
    flags = torch.from_numpy(flags_h).to(dev)
    if isinstance(perturb, torch.Tensor):
        perturb_d = perturb.to(device=dev, dtype=torch.float32).contiguous()
    else:
        perturb_d = torch.from_numpy(np.ascontiguousarray(perturb, dtype=np.float32)).to(dev)
    if tuple(perturb_d.shape) != (nb, 3, 4):
        raise ValueError(f"augment_pairs: perturb {tuple(perturb_d.shape)} for {nb} pairs")
    pk_dev = None
    if pair_keys is not None:
        pk = np.ascontiguousarray(pair_keys, dtype=np.uint64).reshape(-1)
        if pk.size != nb:
            raise ValueError(f"augment_pairs: {pk.size} pair keys for {nb} pairs")
        pk_dev = torch.from_numpy(pk.view(np.int64)).to(dev)
    elif noise is None or keys is None:
        raise ValueError("augment_pairs: pair_keys are needed when noise or keys are generated inline")
    if (src_mask is None) != (tgt_mask is None):
        raise ValueError("augment_pairs: masks come for both clouds or for neither")
    if src_mask is not None:
        src_mask = _dev(src_mask, "src_mask").to(torch.uint8).contiguous()
        tgt_mask = _dev(tgt_mask, "tgt_mask").to(torch.uint8).contiguous()
        if src_mask.numel() != ns or tgt_mask.numel() != nt:
            raise ValueError("augment_pairs: mask length differs from the cloud's")
    if noise is not None:
        noise = _dev(noise, "noise", torch.float32)
        if tuple(noise.shape) != (ns + nt, 3):
            raise ValueError(f"augment_pairs: noise {tuple(noise.shape)}, expected {(ns + nt, 3)}")
    if keys is not None:
        keys = _dev(keys, "keys", torch.int32)
        if keys.numel() != ns + nt:
            raise ValueError(f"augment_pairs: {keys.numel()} keys for {ns + nt} points")
    stride = 0
    off_d = cnt_d = out_corr = out_cnt = None
    if corr is not None:
        corr = _dev(corr, "corr", torch.int32)
        stride = int(corr.shape[1])
        off_d = torch.from_numpy(np.ascontiguousarray(corr_off, dtype=np.int32).reshape(-1)).to(dev) \
            if not isinstance(corr_off, torch.Tensor) else _dev(corr_off, "corr_off", torch.int32)
        cnt_d = torch.from_numpy(np.ascontiguousarray(corr_count, dtype=np.int32).reshape(-1)).to(dev) \
            if not isinstance(corr_count, torch.Tensor) else _dev(corr_count, "corr_count", torch.int32)
        if off_d.numel() != nb or cnt_d.numel() != nb:
            raise ValueError("augment_pairs: corr_off / corr_count need one entry per pair")
        out_corr = torch.empty((2, stride), dtype=torch.int32, device=dev)
        out_cnt = torch.zeros((nb,), dtype=torch.int32, device=dev)
    if out_lens is not None:
        n_os, n_ot = int(sum(out_lens[0])), int(sum(out_lens[1]))
    else:
        n_os = n_ot = ns + nt
    L = _lib.lib()
    ws = _workspace(L.spr_augment_workspace_bytes(ns, nt, nb, stride), dev)
    o_src = torch.empty((n_os, 3), dtype=torch.float32, device=dev)
    o_tgt = torch.empty((n_ot, 3), dtype=torch.float32, device=dev)
    o_scu = torch.empty((nb + 1,), dtype=torch.int32, device=dev)
    o_tcu = torch.empty((nb + 1,), dtype=torch.int32, device=dev)
    o_pose = torch.empty((nb, 3, 4), dtype=torch.float32, device=dev)
    o_sperm = torch.empty((n_os,), dtype=torch.int32, device=dev)
    o_tperm = torch.empty((n_ot,), dtype=torch.int32, device=dev)
    o_smask = torch.empty((n_os,), dtype=torch.uint8, device=dev) if src_mask is not None else None
    o_tmask = torch.empty((n_ot,), dtype=torch.uint8, device=dev) if src_mask is not None else None
    status = torch.zeros((max(nb, 1),), dtype=torch.int32, device=dev)
    _lib.check(L.spr_augment_pairs(
        _ptr(src_xyz), _ptr(src_cu), ns, _ptr(tgt_xyz), _ptr(tgt_cu), nt, _ptr(pose), nb, _ptr(src_mask), _ptr(tgt_mask),
        _ptr(corr), stride, _ptr(off_d), _ptr(cnt_d), _ptr(perturb_d), _ptr(flags), AUG_MODES[mode], float(scale),
        int(max_pts), int(seed), _ptr(pk_dev), _ptr(noise), _ptr(keys), _ptr(o_src), _ptr(o_tgt), _ptr(o_scu),
        _ptr(o_tcu), _ptr(o_pose), _ptr(o_smask), _ptr(o_tmask), _ptr(o_sperm), _ptr(o_tperm), _ptr(out_corr),
        _ptr(out_cnt), _ptr(status), _ptr(ws), ws.numel(), _stream(src_xyz)), "spr_augment_pairs")
    out = {'src_xyz': o_src, 'tgt_xyz': o_tgt, 'src_cu': o_scu, 'tgt_cu': o_tcu, 'pose': o_pose, 'src_perm': o_sperm,
           'tgt_perm': o_tperm, 'status': status[:nb]}
    if src_mask is not None:
        out['src_mask'], out['tgt_mask'] = o_smask.view(torch.bool), o_tmask.view(torch.bool)
    if corr is not None:
        out['corr'], out['corr_count'] = out_corr, out_cnt
    return out


class RadiusTable:
    """Cell table of one support set at one radius (spr_radius_table_build), queried by several neighbour
    searches.  The pyramid builds one per level: the conv search, the pool search and the previous level's
    up-sampling search share supports and radius (reference kpconv.py:352, :377, :384)."""

    def __init__(self, supports: torch.Tensor, s_cu: torch.Tensor, radius: float):
        self.supports = _dev(supports, "supports", torch.float32)
        self.s_cu = _dev(s_cu, "s_cu", torch.int32)
        self.radius = float(radius)
        self.ns, self.nb = self.supports.shape[0], self.s_cu.numel() - 1
        L = _lib.lib()
        self.blob = torch.empty((L.spr_radius_table_bytes(self.ns, self.nb),), dtype=torch.uint8, device=supports.device)
        ws = _workspace(L.spr_radius_table_build_workspace_bytes(self.ns, self.nb), supports.device)
        _lib.check(L.spr_radius_table_build(_ptr(self.supports), _ptr(self.s_cu), self.ns, self.nb, self.radius,
                                            _ptr(self.blob), self.blob.numel(), _ptr(ws), ws.numel(),
                                            _stream(self.supports)), "spr_radius_table_build")
        self._slot = 0
        self._slots = L.spr_radius_table_slots()
        self._built = (_ident(self.supports), _ident(self.s_cu))        # the table is stale after an in-place edit

    def matches(self, supports: torch.Tensor, s_cu: torch.Tensor, radius: float) -> bool:
        """True when this table was built from exactly these tensors (same storage, shape AND content: an
        in-place update of the supports bumps their version counter) at this radius and has a result slot left."""
        return ((_ident(supports), _ident(s_cu)) == self._built
                and (_ident(self.supports), _ident(self.s_cu)) == self._built
                and supports.shape[0] == self.ns and float(radius) == self.radius and self._slot < self._slots)

    def query(self, queries: torch.Tensor, q_cu: torch.Tensor, limit: int,
              dense: Optional[bool] = None, select: int = SELECT_NEAREST) -> Tuple[torch.Tensor, int]:
        """int32 [Nq, min(max_count, limit)] and the untruncated max count, like radius_neighbors
        (select=SELECT_INDEX: [Nq, limit], the lowest indices in range; one table serves both rules).
        dense: True -> one wave per query (one pass, no scratch: faster when more supports lie in range than
        `limit`), False -> one thread per query (cheaper for sparse rows), None -> the library's default.  Same rows."""
        queries = _dev(queries, "queries", torch.float32)
        q_cu = _dev(q_cu, "q_cu", torch.int32)
        nq = queries.shape[0]
        self_search = int(queries.data_ptr() == self.supports.data_ptr() and nq == self.ns
                          and q_cu.data_ptr() == self.s_cu.data_ptr())
        L = _lib.lib()
        ws = _workspace(L.spr_radius_table_query_workspace_bytes(nq), queries.device)
        out = torch.empty((nq, limit), dtype=torch.int32, device=queries.device)
        mc = torch.empty((1,), dtype=torch.int32, device=queries.device)
        slot, self._slot = self._slot, self._slot + 1
        _lib.check(L.spr_radius_table_query(_ptr(queries), _ptr(q_cu), nq, self_search, self.ns, self.nb, self.radius,
                                            int(limit), slot, _ptr(self.blob), _ptr(out), _ptr(mc),
                                            -1 if dense is None else int(bool(dense)), int(select), _ptr(ws),
                                            ws.numel(), _stream(queries)), "spr_radius_table_query")
        m = int(mc.item())
        if m == -2:     # cell table too small for this geometry: exact same result, slower path
            return radius_neighbors(queries, self.supports, q_cu, self.s_cu, self.radius, limit, True, algo=1,
                                    select=select)
        if m < 0:
            raise RuntimeError("spr_radius_neighbors: cloud extent / radius exceeds 8191 cells per axis")
        if select == SELECT_INDEX:
            return out, m
        if m < 1:  # cpp_neighbors/wrapper.cpp:201-205
            raise RuntimeError("Error")
        return out[:, :min(m, limit)], m

    def count(self, queries: torch.Tensor, q_cu: torch.Tensor, hist_n: Optional[int] = None, *,
              counts: bool = True, hist: Optional[torch.Tensor] = None):
        """(int32 [Nq] untruncated counts of supports in range, int32 [nb, hist_n] per-cloud histogram of them or
        None) without building a row (spr_radius_table_count): the candidates are those of query(), uncut -- no 128
        columns, no hist_n.  A query with hist_n or more supports in range is not binned.  Takes no result slot and
        no workspace; one device->host read of the status.
        counts=False skips the per-query output (returns None for it); hist= an int32 [nb, hist_n] tensor to ADD the
        histogram to instead of a fresh zeroed one (hist_n is then its width)."""
        queries = _dev(queries, "queries", torch.float32)
        q_cu = _dev(q_cu, "q_cu", torch.int32)
        nq = queries.shape[0]
        self_search = int(queries.data_ptr() == self.supports.data_ptr() and nq == self.ns
                          and q_cu.data_ptr() == self.s_cu.data_ptr())
        if hist is not None:
            if (not hist.is_cuda or hist.dtype != torch.int32 or not hist.is_contiguous()
                    or hist.dim() != 2 or hist.shape[0] != self.nb or hist_n not in (None, hist.shape[1])):
                raise ValueError("RadiusTable.count: hist must be a contiguous int32 [nb, hist_n] device tensor")
            hist_n = hist.shape[1]
        elif hist_n is not None:    # at least one element, so that a refused width reaches the library as a width
            hist = torch.zeros((self.nb * max(int(hist_n), 1),), dtype=torch.int32,
                               device=queries.device).view(self.nb, -1)
        out = torch.empty((nq,), dtype=torch.int32, device=queries.device) if counts else None
        st = torch.empty((1,), dtype=torch.int32, device=queries.device)
        _lib.check(_lib.lib().spr_radius_table_count(_ptr(queries), _ptr(q_cu), nq, self_search, self.ns, self.nb,
                                                     self.radius, _ptr(self.blob), _ptr(out), _ptr(hist),
                                                     0 if hist_n is None else int(hist_n), _ptr(st),
                                                     _stream(queries)), "spr_radius_table_count")
        s = int(st.item())
        if s == -2:     # no count through the sorted-key search (algo 1): rows of hist_n indices are what this avoids
            raise RuntimeError("spr_radius_table_count: the clouds' bounding boxes need more cells at this radius than "
                               "the table holds (64 per support point + 2^20); voxelise or split the cloud")
        if s < 0:
            raise RuntimeError("spr_radius_table_count: cloud extent / radius exceeds 8191 cells per axis")
        return out, hist


def _wants_grad(*tensors) -> bool:
    """True when the call must go through autograd.py (gradients enabled and asked for)."""
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def kpconv(q_pts, s_pts, nbr, x, weights, kernel_points, kp_extent: float, rows_sorted: bool = False,
           impl: int = 0) -> torch.Tensor:
    """a4.  nbr may be int32 or int64 [Nq, K] (possibly a column slice).  Differentiable in x and
    weights (autograd.KPConvFn)."""
    if _wants_grad(x, weights):
        from .autograd import KPConvFn
        return KPConvFn.apply(_dev(q_pts, "q_pts", torch.float32), _dev(s_pts, "s_pts", torch.float32), nbr,
                              _dev(x, "x", torch.float32), weights, kernel_points, float(kp_extent),
                              bool(rows_sorted), int(impl))
    return kpconv_raw(q_pts, s_pts, nbr, x, weights, kernel_points, kp_extent, rows_sorted, impl)


def kpconv_raw(q_pts, s_pts, nbr, x, weights, kernel_points, kp_extent: float, rows_sorted: bool = False,
               impl: int = 0, order: Optional[torch.Tensor] = None) -> torch.Tensor:
    """order: optional int32 permutation of the queries (the tile walk of the ring kernel, e.g. a
    spatial order so that the workgroups of an XCD share neighbour rows in its L2); the output is
    bitwise independent of it."""
    q_pts = _dev(q_pts, "q_pts", torch.float32)
    s_pts = _dev(s_pts, "s_pts", torch.float32)
    x = _dev(x, "x", torch.float32)
    weights = _dev(weights, "weights", torch.float32)
    kernel_points = _dev(kernel_points, "kernel_points", torch.float32)
    if not nbr.is_cuda:
        raise RuntimeError("neighb_inds must be on the device")
    if nbr.dtype != torch.int32:
        nbr = nbr.to(torch.int32)
    stride = nbr.stride(0) if nbr.stride(1) == 1 and nbr.shape[1] > 0 else None
    if stride is None:
        nbr = nbr.contiguous()
        stride = nbr.shape[1]
    nq, ns, kmax = q_pts.shape[0], s_pts.shape[0], nbr.shape[1]
    n_kp, cin, cout = weights.shape
    assert x.shape == (ns, cin), (x.shape, ns, cin)
    L = _lib.lib()
    ws = _workspace(L.spr_kpconv_workspace_bytes(nq, ns, cin, cout), x.device)
    out = torch.empty((nq, cout), dtype=torch.float32, device=x.device)
    xr, xr_n = _get_range(x)
    wr, wr_n = _static_range(weights)
    plan = wplanes = None
    if impl == 0 and n_kp == 15 and cin % 32 == 0 and cout % 32 == 0 and cout <= 256:
        if cin in (32, 64) and cin * cout <= 4096 and kmax <= 128:
            plan = _kpconv_plan(nbr, nq, ns, int(stride), kmax, bool(rows_sorted), order)
        if wr is not None:
            wplanes = _kpconv_wplanes(weights, wr, wr_n)
    _lib.check(L.spr_kpconv_fwd(_ptr(q_pts), nq, _ptr(s_pts), ns, _ptr(nbr), int(stride), kmax,
                                int(bool(rows_sorted)), _ptr(x), cin, _ptr(weights), cout,
                                _ptr(kernel_points), n_kp, float(kp_extent), _ptr(out), int(impl),
                                _ptr(xr), int(xr_n), _ptr(wr), int(wr_n), _ptr(plan), _ptr(wplanes),
                                _ptr(ws), ws.numel(), _stream(x)), "spr_kpconv_fwd")
    return out


def _kpconv_plan(nbr: torch.Tensor, nq: int, ns: int, stride: int, kmax: int, rows_sorted: bool,
                 order: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Tile descriptors of a neighbour matrix for the ring KPConv (spr_kpconv_plan), cached on the
    index tensor: the pyramid hands the same int32 tensor to every block of a level, and training
    re-uses it for the recomputation in the backward.  Keyed like a published range (storage pointer
    + version counter), with the arguments the plan depends on; guarded for readers on other streams."""
    if order is not None:
        order = _dev(order, "order", torch.int32)
        assert order.shape == (nq,)

    def build():
        L = _lib.lib()
        nbytes = L.spr_kpconv_plan_bytes(nq)
        plan = torch.empty((nbytes,), dtype=torch.uint8, device=nbr.device)
        _lib.check(L.spr_kpconv_plan(_ptr(nbr), nq, ns, stride, kmax, int(rows_sorted), _ptr(order), _ptr(plan),
                                     nbytes, _stream(nbr)), "spr_kpconv_plan")
        return plan, plan
    return _derived(nbr, '_spr_kp_plan', (nq, ns, stride, kmax, rows_sorted, None if order is None else _ident(order)),
                    build)


def kpconv_plan_prefetch(nbr: torch.Tensor, ns: int, rows_sorted: bool = True) -> None:
    """Builds (and caches on the tensor) the ring KPConv's tile plan of a neighbour matrix on the CURRENT
    stream: the pyramid builder calls it right behind each radius search on its side stream, so the plan
    kernel runs beside the encoder instead of in front of the first convolution that uses the matrix."""
    if nbr is None or not nbr.is_cuda or nbr.dtype != torch.int32 or nbr.dim() != 2 or nbr.shape[1] < 1:
        return
    if nbr.stride(1) != 1 or nbr.shape[1] > 128 or nbr.shape[0] < 1:
        return
    _kpconv_plan(nbr, nbr.shape[0], int(ns), int(nbr.stride(0)), nbr.shape[1], bool(rows_sorted))


def _kpconv_wplanes(weights: torch.Tensor, wr: torch.Tensor, wr_n: int) -> torch.Tensor:
    """Split-fp16 fragment-order planes of a KPConv weight tensor (spr_kpconv_prep_weights), cached per
    weight version next to its range."""
    def build():
        L = _lib.lib()
        n_kp, cin, cout = weights.shape
        nbytes = L.spr_kpconv_wplanes_bytes(cin, cout)
        planes = torch.empty((nbytes,), dtype=torch.uint8, device=weights.device)
        _lib.check(L.spr_kpconv_prep_weights(_ptr(weights), n_kp, cin, cout, _ptr(wr), int(wr_n), _ptr(planes),
                                             nbytes, _stream(weights)), "spr_kpconv_prep_weights")
        return planes, planes
    return _derived(weights, '_spr_kp_wplanes', wr.data_ptr(), build)


def instnorm(x, cu, eps: float = 1e-5, norm: bool = True, add=None, slope: float = 1.0,
             out=None, max_len: Optional[int] = None) -> torch.Tensor:
    """a5.  out = lrelu(InstanceNorm_per_cloud(x) + add, slope).  max_len: host
    upper bound of the longest cloud (defaults to n: correct, just a larger
    statistics grid).  Differentiable in x and add (autograd.InstNormFn)."""
    if _wants_grad(x, add):
        from .autograd import InstNormFn
        return InstNormFn.apply(_dev(x, "x", torch.float32), _dev(cu, "cu", torch.int32), float(eps), bool(norm),
                                None if add is None else _dev(add, "add", torch.float32), float(slope), max_len)
    return instnorm_raw(x, cu, eps, norm, add, slope, out, max_len)


def instnorm_raw(x, cu, eps: float = 1e-5, norm: bool = True, add=None, slope: float = 1.0,
                 out=None, max_len: Optional[int] = None) -> torch.Tensor:
    x = _dev(x, "x", torch.float32)
    cu = _dev(cu, "cu", torch.int32)
    n, c = x.shape
    nb = cu.numel() - 1
    if add is not None:
        add = _dev(add, "add", torch.float32)
        assert add.shape == x.shape
    if out is None:
        out = torch.empty_like(x)
    L = _lib.lib()
    max_len = n if max_len is None else max(1, min(int(max_len), n))
    ws = _workspace(L.spr_instnorm_workspace_bytes(max_len, nb, c), x.device)
    cnt = _STREAM_SLOTS
    rng = _zero_slots(cnt, x.device)
    _lib.check(L.spr_instnorm(_ptr(x), _ptr(cu), n, nb, max_len, c, float(eps), int(bool(norm)), _ptr(add),
                              float(slope), _ptr(out), _ptr(rng), cnt, _ptr(ws), ws.numel(), _stream(x)),
               "spr_instnorm")
    _set_range(out, rng, cnt)
    return out


def block_tail_tile_rows(ka: int, kb: int, n_out: int) -> int:
    """Rows per statistics tile of the fused block tail for this shape; 0 = no kernel (use the separate
    operators).  Also 0 outside the split-fp16 product mode."""
    if _modes["gemm"] != 1:
        return 0
    return int(_lib.lib().spr_block_tail_tile_rows(int(ka), int(kb), int(n_out)))


def _tail_tiles(cu: torch.Tensor, n: int, tr: int) -> torch.Tensor:
    """tile table of spr_block_tail for a cu_seqlens tensor, cached on it (one per pyramid level and tile
    height; the pyramid hands the same cu tensor to every block of a level) and guarded for readers on
    other streams like the KPConv plans."""
    def build():
        L = _lib.lib()
        t = torch.empty((L.spr_block_tail_tiles_len(n, cu.numel() - 1, tr),), dtype=torch.int32, device=cu.device)
        _lib.check(L.spr_block_tail_tiles(_ptr(cu), n, cu.numel() - 1, tr, _ptr(t), _stream(cu)), "spr_block_tail_tiles")
        return t, t
    return _derived(cu, f'_spr_tail_tiles_{tr}', (n, tr), build)       # one slot per tile height


def instnorm_stats(x, cu, eps: float = 1e-5, max_len: Optional[int] = None):
    """(mean, rstd), each [nb, c]: the statistics passes of `instnorm` alone, for a consumer that normalises on
    load (block_tail(..., xa_stats=...))."""
    x = _dev(x, "x", torch.float32)
    cu = _dev(cu, "cu", torch.int32)
    n, c = x.shape
    nb = cu.numel() - 1
    L = _lib.lib()
    max_len = n if max_len is None else max(1, min(int(max_len), n))
    ws = _workspace(L.spr_instnorm_workspace_bytes(max_len, nb, c), x.device)
    st = torch.empty((2, nb, c), dtype=torch.float32, device=x.device)
    _lib.check(L.spr_instnorm_stats(_ptr(x), _ptr(cu), n, nb, max_len, c, float(eps), _ptr(st[0]), _ptr(st[1]),
                                    _ptr(ws), ws.numel(), _stream(x)), "spr_instnorm_stats")
    return st[0], st[1]


_NORM_BOUNDS = {}


def _norm_bound(max_len: int, device) -> torch.Tensor:
    """One-slot operand range holding sqrt(max_len): |x - mean| <= sqrt(n - 1) sigma for any n values, so an
    instance-normalised (and LeakyReLU'd, slope <= 1) column of a cloud of at most max_len points is bounded by it."""
    key = (int(max_len), str(device))
    t = _NORM_BOUNDS.get(key)
    if t is None:
        t = torch.full((1,), float(max(1, int(max_len))) ** 0.5, dtype=torch.float32, device=device)
        _NORM_BOUNDS[key] = t
    return t


def block_tail(xa, wa, cu, xb=None, wb=None, add=None, eps: float = 1e-5, slope: float = 0.1,
               xa_stats=None, xa_slope: float = 0.1, xa_max_len: Optional[int] = None) -> torch.Tensor:
    """a5, inference: lrelu(IN(xa wa^T) + (IN(xb wb^T) | add), slope) without the un-normalised
    projections ever being written (spr_block_tail).  The caller checks block_tail_tile_rows first.
    xa_stats = (mean, rstd) of instnorm_stats(xa): xa is then the RAW input of a per-cloud InstanceNorm +
    LeakyReLU(xa_slope) that runs while the tiles are staged -- the bottleneck block's norm
    behind its KPConv costs no pass of its own."""
    xa = _dev(xa, "xa", torch.float32)
    wa = _dev(wa, "wa", torch.float32)
    cu = _dev(cu, "cu", torch.int32)
    n, ka = xa.shape
    n_out = wa.shape[0]
    assert wa.shape[1] == ka
    kb = 0
    if xb is not None:
        xb = _dev(xb, "xb", torch.float32)
        wb = _dev(wb, "wb", torch.float32)
        kb = xb.shape[1]
        assert xb.shape[0] == n and wb.shape == (n_out, kb) and add is None
    if add is not None:
        add = _dev(add, "add", torch.float32)
        assert add.shape == (n, n_out)
    nb = cu.numel() - 1
    L = _lib.lib()
    tr = L.spr_block_tail_tile_rows(ka, kb, n_out)
    if tr <= 0:
        raise RuntimeError(f"block_tail: no kernel for ka={ka} kb={kb} n_out={n_out}")
    tiles = _tail_tiles(cu, n, tr)
    out = torch.empty((n, n_out), dtype=torch.float32, device=xa.device)
    ws = _workspace(L.spr_block_tail_workspace_bytes(n, nb, kb, n_out, tr), xa.device)
    if xa_stats is not None:
        xar, xar_n = _norm_bound(n if xa_max_len is None else xa_max_len, xa.device), 1
    else:
        xar, xar_n = _get_range(xa)
    war, war_n = _static_range(wa)
    xbr, xbr_n, wbr, wbr_n = None, 0, None, 0
    if kb > 0:
        xbr, xbr_n = _get_range(xb)
        wbr, wbr_n = _static_range(wb)
    cnt = _STREAM_SLOTS
    rng = _zero_slots(cnt, xa.device)
    mean = rstd = None
    if xa_stats is not None:
        mean, rstd = xa_stats
        assert mean.shape == (nb, ka) and rstd.shape == (nb, ka) and mean.is_contiguous() and rstd.is_contiguous()
    _lib.check(L.spr_block_tail(_ptr(xa), ka, _ptr(wa), _ptr(xb), kb, _ptr(wb), _ptr(add), _ptr(cu), _ptr(tiles),
                                n, nb, n_out, float(eps), float(slope), _ptr(out), _ptr(xar), int(xar_n),
                                _ptr(war), int(war_n), _ptr(xbr), int(xbr_n), _ptr(wbr), int(wbr_n),
                                _ptr(rng), cnt, _ptr(mean), _ptr(rstd), float(xa_slope), _ptr(ws), ws.numel(),
                                _stream(xa)), "spr_block_tail")
    _set_range(out, rng, cnt)
    return out


def cell_order(points: torch.Tensor, cu: torch.Tensor, cell: float) -> torch.Tensor:
    """int32 [N]: the points of every cloud sorted by the Morton code of their `cell`-sized grid cell -- a spatial WALK
    order for gather operators (maxpool(order=...)); results never depend on it."""
    points = _dev(points, "points", torch.float32)
    cu = _dev(cu, "cu", torch.int32)
    n, nb = points.shape[0], cu.numel() - 1
    L = _lib.lib()
    out = torch.empty((n,), dtype=torch.int32, device=points.device)
    ws = _workspace(L.spr_cell_order_workspace_bytes(n), points.device)
    _lib.check(L.spr_cell_order(_ptr(points), _ptr(cu), n, nb, float(cell), _ptr(out), _ptr(ws), ws.numel(),
                                _stream(points)), "spr_cell_order")
    return out


def maxpool(x, idx, order=None) -> torch.Tensor:
    if _wants_grad(x):
        from .autograd import MaxPoolFn
        return MaxPoolFn.apply(_dev(x, "x", torch.float32), idx)
    return maxpool_raw(x, idx, order)


def maxpool_raw(x, idx, order=None) -> torch.Tensor:
    x = _dev(x, "x", torch.float32)
    if idx.dtype != torch.int32:
        idx = idx.to(torch.int32)
    stride = idx.stride(0) if idx.stride(1) == 1 else None
    if stride is None:
        idx = idx.contiguous()
        stride = idx.shape[1]
    ns, c = x.shape
    nq, k = idx.shape
    out = torch.empty((nq, c), dtype=torch.float32, device=x.device)
    L = _lib.lib()
    cnt = _STREAM_SLOTS
    rng = _zero_slots(cnt, x.device)
    if order is not None and (order.dtype != torch.int32 or order.numel() != nq or not order.is_contiguous()):
        raise ValueError("maxpool: order must be a contiguous int32 permutation of the query rows")
    _lib.check(L.spr_maxpool_gather(_ptr(x), ns, c, _ptr(idx), nq, int(stride), k, _ptr(order), _ptr(out),
                                    _ptr(rng), cnt, _stream(x)), "spr_maxpool_gather")
    _set_range(out, rng, cnt)
    return out


def linear(x, weight, bias=None, residual=None, act: int = ACT_NONE) -> torch.Tensor:
    """act(x W^T + bias + residual).  Differentiable in all four tensors (autograd.LinearFn)."""
    if _wants_grad(x, weight, bias, residual):
        from .autograd import LinearFn
        return LinearFn.apply(_dev(x, "x", torch.float32), weight, bias, residual, int(act))
    return linear_raw(x, weight, bias, residual, act)


def linear_raw(x, weight, bias=None, residual=None, act: int = ACT_NONE) -> torch.Tensor:
    x = _dev(x, "x", torch.float32)
    weight = _dev(weight, "weight", torch.float32)
    m, k = x.shape
    n = weight.shape[0]
    assert weight.shape[1] == k
    if bias is not None:
        bias = _dev(bias, "bias", torch.float32)
    if residual is not None:
        residual = _dev(residual, "residual", torch.float32)
        assert residual.shape == (m, n)
    out = torch.empty((m, n), dtype=torch.float32, device=x.device)
    L = _lib.lib()
    ws = _workspace(L.spr_linear_workspace_bytes(), x.device)
    xr, xr_n = _get_range(x)
    wr, wr_n = _static_range(weight)
    # outputs that go on into another GEMM (no residual: FFN hidden, projections) publish their range
    orng = torch.empty((_RANGE_CAP,), dtype=torch.float32, device=x.device) if residual is None else None
    on = ctypes.c_int(0)
    _lib.check(L.spr_linear(_ptr(x), m, k, _ptr(weight), n, _ptr(bias), _ptr(residual), int(act), _ptr(out),
                            _ptr(xr), int(xr_n), _ptr(wr), int(wr_n), _ptr(orng),
                            _RANGE_CAP if orng is not None else 0, ctypes.byref(on),
                            _ptr(ws), ws.numel(), _stream(x)), "spr_linear")
    if orng is not None:
        _set_range(out, orng, on.value)
    return out


# the attention arithmetic a fresh process runs (csrc/attention.hip, g_attn_mode): split-fp16 scores, split-fp16
# probabilities where a 32-key block holds a weight of at least 2^-5 of the running row sum, one rounded plane elsewhere
DEFAULT_ATTN_MODE = 4

_modes = {"gemm": 1, "attn": DEFAULT_ATTN_MODE}   # host mirror of the library's arithmetic switches


def set_gemm_mode(mode: int) -> None:
    """1 = split-fp16 MFMA (default), 0 = exact f32 MFMA."""
    _lib.check(_lib.lib().spr_set_gemm_mode(int(mode)), "spr_set_gemm_mode")
    _modes["gemm"] = int(mode)


def layernorm(x, gamma, beta, eps: float = 1e-5, pos=None, want_norm: bool = True):
    """Returns (LN(x) or None, LN(x)+pos or None).  Differentiable in x, gamma, beta and pos
    (autograd.LayerNormFn)."""
    if _wants_grad(x, gamma, beta, pos):
        from .autograd import LayerNormFn
        n, p = LayerNormFn.apply(_dev(x, "x", torch.float32), gamma, beta, float(eps), pos, bool(want_norm))
        return (n if (want_norm or pos is None) else None), (p if pos is not None else None)
    return layernorm_raw(x, gamma, beta, eps, pos, want_norm)


def layernorm_raw(x, gamma, beta, eps: float = 1e-5, pos=None, want_norm: bool = True):
    x = _dev(x, "x", torch.float32)
    m, c = x.shape
    out_norm = torch.empty_like(x) if want_norm else None
    out_pos = None
    if pos is not None:
        pos = _dev(pos, "pos", torch.float32)
        out_pos = torch.empty_like(x)
    L = _lib.lib()
    cnt = L.spr_layernorm_range_count(m)
    rn = _zero_slots(cnt, x.device) if out_norm is not None else None
    rp = _zero_slots(cnt, x.device) if out_pos is not None else None
    _lib.check(L.spr_layernorm(_ptr(x), m, c, _ptr(_dev(gamma, "gamma", torch.float32)),
                               _ptr(_dev(beta, "beta", torch.float32)), float(eps), _ptr(pos),
                               _ptr(out_norm), _ptr(out_pos), _ptr(rn), _ptr(rp), _stream(x)), "spr_layernorm")
    if out_norm is not None:
        _set_range(out_norm, rn, cnt)
    if out_pos is not None:
        _set_range(out_pos, rp, cnt)
    return out_norm, out_pos


def posemb_sine(xyz, d_model: int, scale: float = 1.0, temperature: float = 10000.0) -> torch.Tensor:
    xyz = _dev(xyz, "xyz", torch.float32)
    n = xyz.shape[0]
    out = torch.empty((n, d_model), dtype=torch.float32, device=xyz.device)
    _lib.check(_lib.lib().spr_posemb_sine(_ptr(xyz), n, d_model, float(scale * 2 * math.pi),
                                          float(temperature), _ptr(out), _stream(xyz)),
               "spr_posemb_sine")
    return out


POSEMB_MLP_WIDTHS = (3, 32, 64, 128, 256, 256)   # PositionEmbeddingLearned: fixed in the kernel (csrc/posemb_mlp.hip)


def _posemb_mlp_params(params, device):
    """The ten tensors mlp.{0,2,4,6,8}.{weight,bias} checked against the fixed widths, as a ctypes pointer array
    (plus the tensors themselves, which must stay alive across the call)."""
    params = list(params)
    if len(params) != 10:
        raise ValueError(f"posemb_mlp: ten parameters (five weights and biases) expected, got {len(params)}")
    keep = []
    for i, t in enumerate(params):
        t = _dev(t.detach() if isinstance(t, torch.Tensor) else t, f"params[{i}]", torch.float32)
        l = i // 2
        want = (POSEMB_MLP_WIDTHS[l + 1], POSEMB_MLP_WIDTHS[l]) if i % 2 == 0 else (POSEMB_MLP_WIDTHS[l + 1],)
        if tuple(t.shape) != want:
            raise ValueError(f"posemb_mlp: params[{i}] has shape {tuple(t.shape)}, the kernel is built for {want} "
                             "(n_dim 3, d_model 256)")
        if t.device != device:
            raise RuntimeError(f"posemb_mlp: params[{i}] is on {t.device}, xyz on {device}")
        keep.append(t)
    return (ctypes.c_void_p * 10)(*[t.data_ptr() for t in keep]), keep


def posemb_mlp(xyz, params) -> torch.Tensor:
    """a7, pos_emb_type 'learned': the MLP 3 -> 32 -> 64 -> 128 -> 256 -> 256 (ReLU between the layers) of xyz [T, 3] in
    one fused kernel.  params: mlp.{0,2,4,6,8}.{weight,bias} in that order.  Differentiable in the parameters
    (autograd.PosEmbMLPFn); coordinates are never differentiated."""
    params = list(params)
    if _wants_grad(*params):
        from .autograd import PosEmbMLPFn
        return PosEmbMLPFn.apply(_dev(xyz, "xyz", torch.float32), *params)
    return posemb_mlp_raw(xyz, params)


def posemb_mlp_raw(xyz, params) -> torch.Tensor:
    xyz = _dev(xyz, "xyz", torch.float32)
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"posemb_mlp: xyz must be [T, 3], got {tuple(xyz.shape)}")
    ptrs, keep = _posemb_mlp_params(params, xyz.device)
    t = xyz.shape[0]
    out = torch.empty((t, 256), dtype=torch.float32, device=xyz.device)
    _lib.check(_lib.lib().spr_posemb_mlp(_ptr(xyz), ptrs, t, 256, _ptr(out), _stream(xyz)), "spr_posemb_mlp")
    return out


def posemb_mlp_bwd(xyz, params, dpe):
    """The ten parameter gradients of sum(posemb_mlp(xyz, params) * dpe), in the order of params."""
    xyz = _dev(xyz, "xyz", torch.float32)
    dpe = _dev(dpe, "dpe", torch.float32)
    t = xyz.shape[0]
    if xyz.dim() != 2 or xyz.shape[1] != 3 or tuple(dpe.shape) != (t, 256):
        raise ValueError(f"posemb_mlp_bwd: xyz [T, 3] and dpe [T, 256] expected, got {tuple(xyz.shape)}, {tuple(dpe.shape)}")
    ptrs, keep = _posemb_mlp_params(params, xyz.device)
    grads = [torch.empty_like(p) for p in keep]
    gptrs = (ctypes.c_void_p * 10)(*[g.data_ptr() for g in grads])
    L = _lib.lib()
    ws = _workspace(L.spr_posemb_mlp_bwd_workspace_bytes(t), xyz.device)
    _lib.check(L.spr_posemb_mlp_bwd(_ptr(xyz), ptrs, _ptr(dpe), t, 256, gptrs, _ptr(ws), ws.numel(), _stream(xyz)),
               "spr_posemb_mlp_bwd")
    return grads


def attention(q, k, v, cu, kv_seg, max_len: int, nhead: int, out=None, lens_host=None,
              kv_seg_host=None) -> torch.Tensor:
    """a9.  q,k,v: [T, nhead*32] views (row stride may exceed the width, e.g.
    slices of a fused [T, 3*d] projection).  Differentiable in q, k, v (autograd.AttentionFn;
    needs the host-side segment lengths / kv map, read back from the device if not given)."""
    if _wants_grad(q, k, v):
        from .autograd import AttentionFn
        if lens_host is None:
            c = cu.cpu().tolist()
            lens_host = [c[i + 1] - c[i] for i in range(len(c) - 1)]
        if kv_seg_host is None:
            kv_seg_host = kv_seg.cpu().tolist()
        return AttentionFn.apply(q, k, v, _dev(cu, "cu", torch.int32), _dev(kv_seg, "kv_seg", torch.int32),
                                 int(max_len), int(nhead), list(lens_host), list(kv_seg_host))
    return attention_raw(q, k, v, cu, kv_seg, max_len, nhead, out)


def attention_raw(q, k, v, cu, kv_seg, max_len: int, nhead: int, out=None, want_lse: bool = False):
    """want_lse: returns (out, lse) with lse [T, nhead] = the per-query log2-sum-exp the backward can reuse
    (spr_attn_varlen_fwd's lse), or (out, None) when the configured core does not produce it."""
    for t, nm in ((q, "q"), (k, "k"), (v, "v")):
        if not t.is_cuda or t.dtype != torch.float32 or t.stride(1) != 1:
            raise RuntimeError(f"attention: {nm} must be a float32 device tensor with unit inner stride")
    T, d = q.shape
    hd = d // nhead
    cu = _dev(cu, "cu", torch.int32)
    kv_seg = _dev(kv_seg, "kv_seg", torch.int32)
    nseg = cu.numel() - 1
    if out is None:
        out = torch.empty((T, d), dtype=torch.float32, device=q.device)
    L = _lib.lib()
    ws = _workspace(L.spr_attn_workspace_bytes(T, nseg, nhead, hd), q.device)
    lse = torch.empty((T, nhead), dtype=torch.float32, device=q.device) if want_lse else None
    written = ctypes.c_int(0)
    _lib.check(L.spr_attn_varlen_fwd(_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0),
                                     _ptr(cu), _ptr(kv_seg), T, nseg, int(max_len), nhead, hd,
                                     1.0 / math.sqrt(hd), _ptr(out), out.stride(0), _ptr(lse),
                                     ctypes.byref(written), _ptr(ws), ws.numel(), _stream(q)),
               "spr_attn_varlen_fwd")
    if want_lse:
        return out, (lse if written.value else None)
    return out


def attention_probs(q, k, cu, kv_seg, max_len: int, nhead: int, average: bool = True, out=None, place=None,
                    max_rows: Optional[int] = None, max_cols: Optional[int] = None) -> torch.Tensor:
    """The softmax attention maps of the varlen core (spr_attn_probs): softmax_j(q_i,h . k_j,h / sqrt(32)) for the
    queries of segment s over the keys of segment kv_seg[s], averaged over the heads (average=True, what
    nn.MultiheadAttention returns by default) or per head.  q, k: [T, nhead*32] views as for attention().
    Always detached (the maps are not differentiable); independent of set_attn_mode.

    Without `out`: a zero-padded [nseg, max_len, max_len] (or [nseg, nhead, max_len, max_len]) tensor.
    With `out`: any float32 device tensor, and `place` = int64 [nseg, 5] rows {element offset into out, row
    stride, head stride, rows, cols} (host or device; max_rows / max_cols = the largest rows / cols, required for a
    device `place`).  Every segment's rows x cols entries are written -- the probabilities in the top-left Lq x Lk
    corner, exact zeros elsewhere -- and nothing else of `out`."""
    for t, nm in ((q, "q"), (k, "k")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"attention_probs: {nm} must be a tensor on the MI355X device; the HIP path has no "
                               "CPU fallback")
        if t.dtype != torch.float32 or t.stride(1) != 1:
            raise RuntimeError(f"attention_probs: {nm} must be float32 with unit inner stride")
    q, k = q.detach(), k.detach()
    T, d = q.shape
    hd = d // nhead
    cu = _dev(cu, "cu", torch.int32)
    kv_seg = _dev(kv_seg, "kv_seg", torch.int32)
    nseg = cu.numel() - 1
    L = int(max_len)
    if out is None:
        if place is not None:
            raise RuntimeError("attention_probs: `place` needs `out`")
        shape = (nseg, L, L) if average else (nseg, nhead, L, L)
        out = torch.empty(shape, dtype=torch.float32, device=q.device)
        per = L * L * (1 if average else nhead)
        pl = np.zeros((nseg, 5), dtype=np.int64)
        pl[:, 0] = np.arange(nseg, dtype=np.int64) * per
        pl[:, 1], pl[:, 2], pl[:, 3], pl[:, 4] = L, L * L, L, L
        place, max_rows, max_cols = pl, L, L
    else:
        if not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous():
            raise RuntimeError("attention_probs: out must be a contiguous float32 device tensor")
        if place is None:
            raise RuntimeError("attention_probs: `out` needs `place`")
    if isinstance(place, np.ndarray) or (isinstance(place, torch.Tensor) and not place.is_cuda):
        pl = np.asarray(place.cpu().numpy() if isinstance(place, torch.Tensor) else place, dtype=np.int64)
        if pl.shape != (nseg, 5):
            raise RuntimeError(f"attention_probs: place must be [nseg={nseg}, 5] (got {pl.shape})")
        nh = 1 if average else nhead
        last = pl[:, 0] + (nh - 1) * pl[:, 2] + (pl[:, 3] - 1) * pl[:, 1] + pl[:, 4]
        if (pl[:, 0] < 0).any() or (pl[:, 3] < 1).any() or (pl[:, 4] < 1).any() or (pl[:, 4] > pl[:, 1]).any() \
                or int(last.max()) > out.numel():
            raise RuntimeError("attention_probs: place describes entries outside `out`")
        max_rows, max_cols = int(pl[:, 3].max()), int(pl[:, 4].max())
        place = torch.from_numpy(pl).to(q.device)
    elif max_rows is None or max_cols is None:
        raise RuntimeError("attention_probs: a device `place` needs max_rows and max_cols")
    Lb = _lib.lib()
    ws = _workspace(Lb.spr_attn_probs_workspace_bytes(T, nhead, hd), q.device)
    _lib.check(Lb.spr_attn_probs(_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(cu), _ptr(kv_seg), T, nseg, L,
                                 nhead, hd, 1.0 / math.sqrt(hd), 0 if average else 1, _ptr(out), _ptr(place),
                                 int(max_rows), int(max_cols), _ptr(ws), ws.numel(), _stream(q)), "spr_attn_probs")
    return out


_seg_perm_cache = {}


def _segment_perms(kv_seg_host, device):
    """(kv_seg, inverse) as int32 device tensors for a host-side permutation (cached: a model uses two --
    the identity for self attention and the src <-> tgt swap for cross attention)."""
    key = (tuple(int(x) for x in kv_seg_host), str(device))
    c = _seg_perm_cache.get(key)
    if c is None:
        kv = np.asarray(key[0], dtype=np.int32)
        inv = np.empty_like(kv)
        inv[kv] = np.arange(kv.size, dtype=np.int32)
        c = (torch.from_numpy(kv).to(device), torch.from_numpy(inv).to(device))
        _seg_perm_cache[key] = c
    return c


def attention_bwd(q, k, v, out, dout, cu, kv_seg_host, max_len: int, nhead: int, lse=None):
    """Gradients (dq, dk, dv) of attention_raw (spr_attn_varlen_bwd: flash-style; the arithmetic follows
    set_attn_mode: split-fp16 like the forward, or exact f32 MFMA in mode 0)."""
    for t, nm in ((q, "q"), (k, "k"), (v, "v"), (out, "out"), (dout, "dout")):
        if not t.is_cuda or t.dtype != torch.float32 or t.stride(1) != 1:
            raise RuntimeError(f"attention_bwd: {nm} must be a float32 device tensor with unit inner stride")
    T, d = q.shape
    hd = d // nhead
    cu = _dev(cu, "cu", torch.int32)
    nseg = cu.numel() - 1
    kv, inv = _segment_perms(kv_seg_host, q.device)
    dq = torch.empty((T, d), dtype=torch.float32, device=q.device)
    dk = torch.empty_like(dq)
    dv = torch.empty_like(dq)
    L = _lib.lib()
    ws = _workspace(L.spr_attn_bwd_workspace_bytes(T, nseg, nhead), q.device)      # with room for the operand planes
    _lib.check(L.spr_attn_varlen_bwd(_ptr(q), q.stride(0), _ptr(k), k.stride(0), _ptr(v), v.stride(0), _ptr(out),
                                     out.stride(0), _ptr(dout), dout.stride(0), _ptr(lse), _ptr(cu), _ptr(kv),
                                     _ptr(inv), T, nseg, int(max_len), nhead, hd, 1.0 / math.sqrt(hd), _ptr(dq),
                                     _ptr(dk), _ptr(dv), _ptr(ws), ws.numel(), _stream(q)), "spr_attn_varlen_bwd")
    return dq, dk, dv


def inproj_prepare(w_in: torch.Tensor):
    """Weight-side inputs of the fused in-projection (max |w| partials + row L1 norms), measured
    once per weight version and cached on the tensor like _static_range."""
    def build():
        L = _lib.lib()
        d = w_in.shape[1]
        buf = torch.empty((L.spr_range_parts() + 3 * d,), dtype=torch.float32, device=w_in.device)
        _lib.check(L.spr_attn_inproj_prepare(_ptr(w_in), d, _ptr(buf), _stream(w_in)), "spr_attn_inproj_prepare")
        return buf, buf
    return _derived(w_in, '_spr_inproj', None, build)


def attention_inproj(x_qk, x_v, w_in, b_in, cu, kv_seg, max_len: int, nhead: int, w_prep=None) -> torch.Tensor:
    """In-projection (packed [3d, d] weight, q/k from x_qk, v from x_v) + attention core.
    w_prep: inproj_prepare(weight) of the SAME weight (callers that hold the parameter object
    pass it so that the measurement is cached across calls)."""
    x_qk = _dev(x_qk, "x_qk", torch.float32)
    x_v = x_qk if x_v is x_qk else _dev(x_v, "x_v", torch.float32)
    w_in = _dev(w_in, "w_in", torch.float32)
    b_in = _dev(b_in, "b_in", torch.float32)
    T, d = x_qk.shape
    assert x_v.shape == (T, d) and w_in.shape == (3 * d, d) and b_in.shape == (3 * d,)
    hd = d // nhead
    cu = _dev(cu, "cu", torch.int32)
    kv_seg = _dev(kv_seg, "kv_seg", torch.int32)
    nseg = cu.numel() - 1
    out = torch.empty((T, d), dtype=torch.float32, device=x_qk.device)
    L = _lib.lib()
    ws = _workspace(L.spr_attn_inproj_workspace_bytes(T, nseg, nhead, hd), x_qk.device)
    fused = _modes["attn"] != 0 and _modes["gemm"] == 1 and T >= 256     # the route that can take / publish ranges
    qr, qn = _get_range(x_qk) if fused else (None, 0)
    vr, vn = (qr, qn) if x_v is x_qk else (_get_range(x_v) if fused else (None, 0))
    orng = torch.empty((1,), dtype=torch.float32, device=x_qk.device) if fused else None
    _lib.check(L.spr_attn_inproj_varlen_fwd(_ptr(x_qk), _ptr(x_v), T, _ptr(w_in), _ptr(b_in), _ptr(cu),
                                            _ptr(kv_seg), nseg, int(max_len), nhead, hd, 1.0 / math.sqrt(hd),
                                            _ptr(out), out.stride(0), _ptr(qr), int(qn), _ptr(vr), int(vn),
                                            _ptr(orng), _ptr(w_prep if fused else None), _ptr(ws), ws.numel(),
                                            _stream(x_qk)),
               "spr_attn_inproj_varlen_fwd")
    if orng is not None:
        _set_range(out, orng, 1)
    return out


# ---- fused cross-encoder stack (csrc/xenc.hip) ---------------------------------------------------
_xenc_lock = threading.Lock()
XENC_PTRS_PER_LAYER = 18                                # SPR_XENC_PTRS_PER_LAYER of include/spr.h


class XencPlan:
    """Prepared weights of a cross-encoder stack: split-fp16 fragment streams on the device + the
    host-side plan (spr_xenc_prepare).  Valid while the parameters it was built from are untouched
    (storage pointers and version counters are part of `key`)."""

    def __init__(self, key, prepared, plan, keep):
        self.key, self.prepared, self.plan, self.keep = key, prepared, plan, keep

    # The host plan holds device addresses inside `prepared`: a copy must not outlive the original.  A copied or
    # unpickled module simply has no plan and builds its own on first use (copy.deepcopy(model), torch.save(model)).
    def __deepcopy__(self, memo):
        return None

    def __reduce__(self):
        return (_no_plan, ())


def _no_plan():
    return None


def xenc_available() -> bool:
    return _modes["gemm"] == 1 and _modes["attn"] in (1, 2, 3, 4)


def xenc_prepare(layer_params, layer_eps, final, nhead: int, d_ff: int, pos_bound: float, cached=None) -> XencPlan:
    """layer_params: per layer the 18 parameter tensors in the order of include/spr.h
    (SPR_XENC_PTRS_PER_LAYER); layer_eps: per layer (eps1, eps2, eps3); final: (weight, bias, eps) of
    the stack's last LayerNorm or None.  `cached`: a previous XencPlan, returned as is when nothing changed."""
    flat = [t for lp in layer_params for t in lp] + ([final[0], final[1]] if final is not None else [])
    key = (tuple(_ident(t) for t in flat), tuple(float(e) for le in layer_eps for e in le),
           None if final is None else float(final[2]), int(nhead), int(d_ff), float(pos_bound))
    if cached is not None and cached.key == key:
        return cached
    with _xenc_lock:
        L = _lib.lib()
        n_layers = len(layer_params)
        keep = [_dev(t.detach(), "parameter", torch.float32) for t in flat]
        per = XENC_PTRS_PER_LAYER
        assert all(len(lp) == per for lp in layer_params)
        ptrs = (ctypes.c_void_p * (n_layers * per))(*[t.data_ptr() for t in keep[:n_layers * per]])
        eps = (ctypes.c_float * (3 * n_layers))(*[float(e) for le in layer_eps for e in le])
        dev = keep[0].device
        nbytes = L.spr_xenc_prepared_bytes(n_layers, int(d_ff))
        if nbytes == 0:
            raise RuntimeError("xenc_prepare: unsupported stack shape")
        prepared = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        plan = ctypes.create_string_buffer(L.spr_xenc_plan_bytes())
        fg = keep[-2] if final is not None else None
        fb = keep[-1] if final is not None else None
        _lib.check(L.spr_xenc_prepare(ptrs, eps, n_layers, 256, int(nhead), int(d_ff), _ptr(fg), _ptr(fb),
                                      float(final[2]) if final is not None else 0.0, float(pos_bound),
                                      _ptr(prepared), nbytes, plan, len(plan), _stream(prepared)), "spr_xenc_prepare")
        return XencPlan(key, prepared, plan, keep)


def xenc_forward(plan: XencPlan, x, pos, cu, seg_self, seg_cross, max_len: int) -> torch.Tensor:
    x = _dev(x, "x", torch.float32)
    pos = _dev(pos, "pos", torch.float32)
    cu = _dev(cu, "cu", torch.int32)
    seg_self = _dev(seg_self, "seg_self", torch.int32)
    seg_cross = _dev(seg_cross, "seg_cross", torch.int32)
    T, d = x.shape
    assert d == 256 and pos.shape == (T, d)
    nseg = cu.numel() - 1
    out = torch.empty_like(x)
    L = _lib.lib()
    ws = _workspace(L.spr_xenc_workspace_bytes(T, nseg), x.device)
    plan.prepared.record_stream(torch.cuda.current_stream(x.device))
    _lib.check(L.spr_xenc_forward(plan.plan, _ptr(x), _ptr(pos), _ptr(cu), _ptr(seg_self), _ptr(seg_cross), T, nseg,
                                  int(max_len), _ptr(out), _ptr(ws), ws.numel(), _stream(x)), "spr_xenc_forward")
    return out


def set_attn_mode(mode: int) -> None:
    """4 = split-fp16 MFMA with the lo plane of the probabilities only on tiles that hold a weight of at least 2^-5 of
    the running row sum (default, DEFAULT_ATTN_MODE), 1 = split-fp16 MFMA everywhere, 0 = exact f32 MFMA, 2 =
    single-pass fp16 MFMA, 3 = split-fp16 scores with ONE probability plane (weights rounded to 11 bits, row sum from
    the rounded plane) (csrc/attention.hip, k_attn_s; accuracy table in DESIGN.md section 4)."""
    _lib.check(_lib.lib().spr_set_attn_mode(int(mode)), "spr_set_attn_mode")
    _modes["attn"] = int(mode)


def _cu_host_arr(cu_host: Sequence[int]):
    arr = (ctypes.c_int * len(cu_host))(*[int(v) for v in cu_host])
    return arr


def match_dualsoftmax(feat, cu, cu_host: Sequence[int], npairs: int):
    """a11.  Returns (val [T] f32, ind [T] i32) -- see include/spr.h.  val is differentiable in
    feat (autograd.MatchDualSoftmaxFn)."""
    if _wants_grad(feat):
        from .autograd import MatchDualSoftmaxFn
        return MatchDualSoftmaxFn.apply(_dev(feat, "feat", torch.float32), _dev(cu, "cu", torch.int32),
                                        list(cu_host), int(npairs))
    return match_dualsoftmax_raw(feat, cu, cu_host, npairs)


def match_dualsoftmax_top2(feat, cu, cu_host: Sequence[int], npairs: int):
    """(val, val2, ind): the best and the runner-up dual-softmax value of every match (Lowe ratio
    test of RegTR.ratio_test, qk_regtr_full.py:370-384).  Inference only."""
    val, val2, ind, _, _ = _match_head(feat, None, cu, cu_host, npairs, None, None, 0, match=True, top2=True,
                                       sinkhorn=False)
    return val, val2, ind


def pose_residuals(pose, a, b, pair_cu) -> torch.Tensor:
    """res[i] = ||b_i - T_s a_i|| with one pose [3,4] per set of pair_cu (LGR re-weighting,
    qk_regtr_full.py:386-398)."""
    a, b = _dev(a, "a", torch.float32), _dev(b, "b", torch.float32)
    pose = _dev(pose, "pose", torch.float32)
    pair_cu = _dev(pair_cu, "pair_cu", torch.int32)
    n = a.shape[0]
    res = torch.empty((n,), dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().spr_pose_residuals(_ptr(pose), _ptr(a), _ptr(b), _ptr(pair_cu), pair_cu.numel() - 1, n,
                                             _ptr(res), _stream(a)), "spr_pose_residuals")
    return res


def pose_scores(poses, a, b) -> torch.Tensor:
    """score[h] = mean_i ||b_i - T_h a_i|| for H hypotheses [H,3,4] over one point set (RANSAC
    scoring, qk_regtr_full.py:400-421)."""
    a, b = _dev(a, "a", torch.float32), _dev(b, "b", torch.float32)
    poses = _dev(poses, "poses", torch.float32)
    h = poses.shape[0]
    out = torch.empty((h,), dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().spr_pose_scores(_ptr(poses), h, _ptr(a), _ptr(b), a.shape[0], _ptr(out), _stream(a)),
               "spr_pose_scores")
    return out


REFINE_FLAGS = {'ratio': 1, 'median': 2, 'overlap': 4, 'overlap_as_weights': 8, 'topk': 16, 'lgr': 32, 'sinkhorn': 64}
REFINE_MAX_N = 16384          # SPR_REFINE_MAX_N of include/spr.h
REFINE_BAD_INDEX, REFINE_BAD_LAYOUT = 1, 2


def refine_pairs(val, val2, ind, overlap, xyz, cu, cu_host: Sequence[int], npairs: int, k=None, *, ratio: bool = False,
                 median: bool = False, overlap_prune: bool = False, overlap_as_weights: bool = False,
                 lgr_steps: int = 0, lowe_thres: float = 0.0, acceptance_radius: float = 0.0, pose_in=None,
                 sinkhorn: bool = False) -> dict:
    """8f-3.  The config-off refinements of RegTR.softmax_correlation (ratio test, median threshold, overlap weighting,
    top-k pruning, pose, LGR) for all pairs in one call (spr_refine_pairs; the order of operations is in include/spr.h).
    val / val2 / ind [T] as match_dualsoftmax(_top2) returns them (val2 None unless `ratio`), overlap [T] or [T,1],
    xyz [T,3], cu int32 [2B+1] with its host copy cu_host.  k: entries kept per pair ([B] ints, top-k pruning), None
    keeps all min(N, M) entries in token order.  pose_in [B,3,4]: the pose stands (no solve) and LGR starts from it;
    `sinkhorn`: the point sets are the src / tgt points at the entry's position (needs pose_in).
    Returns a dict: pose [B,3,4]; val, ind (int64), src_pts, tgt_pts packed at out_cu (host list, [B+1]); status [B]
    int32 on the device (0, REFINE_BAD_INDEX, REFINE_BAD_LAYOUT) -- nothing here reads it back."""
    B = int(npairs)
    cu_h = [int(c) for c in cu_host]
    if B < 1 or len(cu_h) != 2 * B + 1 or cu_h[0] != 0 or any(b < a for a, b in zip(cu_h, cu_h[1:])):
        raise ValueError(f"refine_pairs: cu_host of {len(cu_h)} entries does not describe {B} pairs")
    n_own = [min(cu_h[b + 1] - cu_h[b], cu_h[B + b + 1] - cu_h[B + b]) for b in range(B)]
    k_h = list(n_own) if k is None else [int(x) for x in k]
    if len(k_h) != B or any(not 0 <= kk <= n for kk, n in zip(k_h, n_own)):
        raise ValueError(f"refine_pairs: k {k_h} for pairs of {n_own} entries")
    if overlap_as_weights and not overlap_prune:
        raise ValueError("refine_pairs: overlap_as_weights needs overlap_prune")
    if max(n_own) > REFINE_MAX_N:
        raise ValueError(f"refine_pairs: a pair of {max(n_own)} entries, the cap is {REFINE_MAX_N}")
    if sinkhorn and pose_in is None:
        raise ValueError("refine_pairs: sinkhorn needs pose_in")
    if ratio and val2 is None:
        raise ValueError("refine_pairs: the ratio test needs val2")
    val = _dev(val, "val", torch.float32)
    val2 = _dev(val2, "val2", torch.float32) if ratio else None
    ind = _dev(ind, "ind", torch.int32)
    overlap = _dev(overlap, "overlap", torch.float32).reshape(-1)
    xyz = _dev(xyz, "xyz", torch.float32)
    cu = _dev(cu, "cu", torch.int32)
    if pose_in is not None:
        pose_in = _dev(pose_in, "pose_in", torch.float32)
    T = cu_h[-1]
    sizes = (val.numel(), ind.numel(), overlap.numel(), xyz.shape[0], T if val2 is None else val2.numel())
    if any(n != T for n in sizes) or xyz.dim() != 2 or xyz.shape[1] != 3 or cu.numel() != 2 * B + 1:
        raise ValueError(f"refine_pairs: val / ind / overlap / xyz rows / val2 = {sizes}, cu {cu.numel()}; expected {T} "
                         f"tokens and {2 * B + 1} prefix entries")
    if pose_in is not None and tuple(pose_in.shape) != (B, 3, 4):
        raise ValueError(f"refine_pairs: pose_in {tuple(pose_in.shape)} for {B} pairs")
    dev = val.device
    out_cu = [0]
    for kk in k_h:
        out_cu.append(out_cu[-1] + kk)

    def build():    # k_b and out_cu: one upload, kept on cu while the same pairs are refined again
        t = torch.from_numpy(np.asarray(k_h + out_cu, dtype=np.int32)).to(dev)
        return t, t
    meta = _derived(cu, '_spr_refine_meta', tuple(k_h), build)
    flags = ((REFINE_FLAGS['ratio'] if ratio else 0) | (REFINE_FLAGS['median'] if median else 0)
             | (REFINE_FLAGS['overlap'] if overlap_prune else 0)
             | (REFINE_FLAGS['overlap_as_weights'] if overlap_as_weights else 0)
             | (REFINE_FLAGS['topk'] if k is not None else 0) | (REFINE_FLAGS['lgr'] if lgr_steps > 0 else 0)
             | (REFINE_FLAGS['sinkhorn'] if sinkhorn else 0))
    S = out_cu[-1]
    L = _lib.lib()
    need = L.spr_refine_pairs_workspace_bytes(B, max(n_own))
    ws = _workspace(need, dev) if need else None
    pose = torch.empty((B, 3, 4), dtype=torch.float32, device=dev)
    rows = max(S, 1)              # k = 0 everywhere is legal; the library wants real pointers
    o_val = torch.empty((rows,), dtype=torch.float32, device=dev)
    o_ind = torch.empty((rows,), dtype=torch.int64, device=dev)
    o_src = torch.empty((rows, 3), dtype=torch.float32, device=dev)
    o_tgt = torch.empty((rows, 3), dtype=torch.float32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    _lib.check(L.spr_refine_pairs(_ptr(val), _ptr(val2), _ptr(ind), _ptr(overlap), _ptr(xyz), _ptr(cu), B, T,
                                  _ptr(meta[:B]), _ptr(meta[B:]), flags, float(lowe_thres), float(acceptance_radius),
                                  int(lgr_steps), _ptr(pose_in), max(n_own), _ptr(pose), _ptr(o_val), _ptr(o_ind),
                                  _ptr(o_src), _ptr(o_tgt), _ptr(status), _ptr(ws), ws.numel() if ws is not None else 0,
                                  _stream(val)), "spr_refine_pairs")
    return {'pose': pose, 'val': o_val[:S], 'ind': o_ind[:S], 'src_pts': o_src[:S], 'tgt_pts': o_tgt[:S],
            'out_cu': out_cu, 'out_cu_dev': meta[B:], 'status': status}


RANSAC_EMPTY, RANSAC_BAD_INDEX, RANSAC_BAD_LAYOUT = 1, 2, 4


def _ransac_sizes(what: str, n_hyp, sample):
    n_hyp, sample = int(n_hyp), int(sample)
    if n_hyp < 1 or sample < 1:
        raise ValueError(f"{what}: n_hyp {n_hyp} and sample {sample} must be at least 1")
    if n_hyp * ((sample + 3) // 4) >= 2 ** 32:
        raise ValueError(f"{what}: n_hyp * ceil(sample / 4) = {n_hyp * ((sample + 3) // 4)} does not fit the 32-bit "
                         "block counter")
    return n_hyp, sample


def _pair_keys(what: str, pair_keys, B: int) -> np.ndarray:
    if isinstance(pair_keys, torch.Tensor):
        pair_keys = pair_keys.tolist()
    keys = list(range(B)) if pair_keys is None else [int(k) for k in np.asarray(pair_keys, dtype=object).reshape(-1)]
    if len(keys) != B:
        raise ValueError(f"{what}: {len(keys)} pair keys for {B} pairs")
    if any(not 0 <= k < 2 ** 63 for k in keys):
        raise ValueError(f"{what}: pair keys must lie in [0, 2^63)")
    return np.asarray(keys, dtype=np.uint64)


def ransac_draw(seed: int, pair_keys, n, n_hyp: int, sample: int) -> np.ndarray:
    """The sample indices ransac_pairs draws for pairs `pair_keys` of `n` entries each under `seed`, through the
    library's host path (spr_ransac_draw; the draw contract is in include/spr.h): int32 [B, n_hyp, sample].  Needs no
    device."""
    n_hyp, sample = _ransac_sizes("ransac_draw", n_hyp, sample)
    n_h = [int(x) for x in np.asarray(n).reshape(-1)]
    pk = _pair_keys("ransac_draw", pair_keys, len(n_h))
    if any(not 0 <= x < 2 ** 31 for x in n_h):
        raise ValueError(f"ransac_draw: n {n_h} must lie in [0, 2^31)")
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError("ransac_draw: seed must lie in [0, 2^64)")
    n_arr = np.asarray(n_h, dtype=np.int32)
    out = np.zeros((len(n_h), n_hyp, sample), dtype=np.int32)
    _lib.check(_lib.lib().spr_ransac_draw(int(seed), pk.ctypes.data, n_arr.ctypes.data, len(n_h), n_hyp, sample,
                                          out.ctypes.data), "spr_ransac_draw")
    return out


def ransac_pairs(a, b, w, set_cu, set_cu_host: Sequence[int], *, n_hyp: int = 500, sample: int = 100, seed: int = 0,
                 pair_keys=None, idx=None) -> dict:
    """RANSAC (RegTR.ransac, qk_regtr_full.py:400-421) for all pairs of a batch in one call (spr_ransac_pairs; the
    contract -- draws, summation order, arg-min rule -- is in include/spr.h).  a, b [T,3] and w [T] packed by set_cu
    int32 [B+1] with its host copy set_cu_host: what refine_pairs returns as src_pts, tgt_pts, val, out_cu_dev and
    out_cu.  Per pair n_hyp hypotheses of `sample` entries drawn with replacement from Philox blocks keyed on
    (seed, pair key); pair_keys None = the position in the batch.  idx int32 [B, n_hyp, sample] replaces the draws.
    Returns a dict of device tensors: pose [B,3,4], best [B] int32 (-1 for an empty pair), score [B, n_hyp],
    hyp_pose [B, n_hyp, 3, 4], status [B] int32 (0, RANSAC_EMPTY, RANSAC_BAD_INDEX, RANSAC_BAD_LAYOUT) -- nothing here
    reads it back."""
    n_hyp, sample = _ransac_sizes("ransac_pairs", n_hyp, sample)
    cu_h = [int(c) for c in set_cu_host]
    B = len(cu_h) - 1
    if B < 1 or cu_h[0] != 0 or any(y < x for x, y in zip(cu_h, cu_h[1:])):
        raise ValueError(f"ransac_pairs: set_cu_host {cu_h[:8]}{'...' if len(cu_h) > 8 else ''} is not an ascending "
                         "prefix from 0 over at least one pair")
    if B > 65535:
        raise ValueError(f"ransac_pairs: {B} pairs, at most 65535 per call")
    T = cu_h[-1]
    shapes = tuple(tuple(t.shape) if isinstance(t, torch.Tensor) else None for t in (a, b, w, set_cu))
    if shapes[0] != (T, 3) or shapes[1] != (T, 3) or shapes[2] not in ((T,), (T, 1)) or shapes[3] != (B + 1,):
        raise ValueError(f"ransac_pairs: a / b / w / set_cu of shapes {shapes}; set_cu_host describes {T} entries in "
                         f"{B} pairs")
    pk = _pair_keys("ransac_pairs", pair_keys, B)
    if not 0 <= int(seed) < 2 ** 64:
        raise ValueError("ransac_pairs: seed must lie in [0, 2^64)")
    if idx is not None and (not isinstance(idx, torch.Tensor) or tuple(idx.shape) != (B, n_hyp, sample)):
        raise ValueError(f"ransac_pairs: idx {tuple(idx.shape) if isinstance(idx, torch.Tensor) else type(idx)}, "
                         f"expected {(B, n_hyp, sample)}")
    a, b = _dev(a, "a", torch.float32), _dev(b, "b", torch.float32)
    w = _dev(w, "w", torch.float32).reshape(-1)
    set_cu = _dev(set_cu, "set_cu", torch.int32)
    dev = a.device
    if T == 0:                    # every pair empty: the library wants real pointers
        a, b, w = a.new_zeros((1, 3)), b.new_zeros((1, 3)), w.new_zeros((1,))
    pk_dev = None
    if idx is None:
        pk_dev = torch.from_numpy(pk.view(np.int64)).to(dev)
    else:
        idx = _dev(idx, "idx", torch.int32)
    pose = torch.empty((B, 3, 4), dtype=torch.float32, device=dev)
    best = torch.empty((B,), dtype=torch.int32, device=dev)
    score = torch.empty((B, n_hyp), dtype=torch.float32, device=dev)
    hyp_pose = torch.empty((B, n_hyp, 3, 4), dtype=torch.float32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().spr_ransac_pairs(_ptr(a), _ptr(b), _ptr(w), _ptr(set_cu), B, n_hyp, sample, int(seed),
                                           _ptr(pk_dev), _ptr(idx), _ptr(pose), _ptr(best), _ptr(score),
                                           _ptr(hyp_pose), _ptr(status), _stream(a)), "spr_ransac_pairs")
    return {'pose': pose, 'best': best, 'score': score, 'hyp_pose': hyp_pose, 'status': status}


def _match_head(feat, xyz, cu, cu_host: Sequence[int], npairs: int, alpha, beta, n_iters: int, *, match: bool,
                top2: bool, sinkhorn: bool):
    """The one marshalling of the matching head's three entry points (csrc/match_pose.hip, match_head).
    Returns (val, val2, ind, w, t_hat) with None for what was not asked for."""
    feat = _dev(feat, "feat", torch.float32)
    cu = _dev(cu, "cu", torch.int32)
    dev = feat.device
    T, d = feat.shape
    arr = _cu_host_arr(cu_host)
    L = _lib.lib()
    ws = _workspace(L.spr_match_workspace_bytes(arr, npairs), dev)
    val = val2 = ind = w = that = None
    if match:
        val = torch.zeros((T,), dtype=torch.float32, device=dev)
        val2 = torch.zeros((T,), dtype=torch.float32, device=dev) if top2 else None
        ind = torch.zeros((T,), dtype=torch.int32, device=dev)
    if sinkhorn:
        alpha_t, beta_t = _dev_scalar(alpha, dev), _dev_scalar(beta, dev)
        xyz = _dev(xyz, "xyz", torch.float32)
        tsrc = int(cu_host[npairs])
        w = torch.empty((tsrc,), dtype=torch.float32, device=dev)
        that = torch.empty((tsrc, 3), dtype=torch.float32, device=dev)
    tail = (_ptr(ws), ws.numel(), _stream(feat))
    if not sinkhorn:
        _lib.check(L.spr_match_dualsoftmax(_ptr(feat), d, _ptr(cu), arr, npairs, _ptr(val), _ptr(val2), _ptr(ind),
                                           *tail), "spr_match_dualsoftmax")
    elif not match:
        _lib.check(L.spr_sinkhorn_correspondences(_ptr(feat), d, _ptr(xyz), _ptr(cu), arr, npairs, _ptr(alpha_t),
                                                  _ptr(beta_t), int(n_iters), 1, _ptr(w), _ptr(that), *tail),
                   "spr_sinkhorn_correspondences")
    else:
        _lib.check(L.spr_match_sinkhorn(_ptr(feat), d, _ptr(xyz), _ptr(cu), arr, npairs, _ptr(alpha_t), _ptr(beta_t),
                                        int(n_iters), _ptr(val), _ptr(val2), _ptr(ind), _ptr(w), _ptr(that), *tail),
                   "spr_match_sinkhorn")
    return val, val2, ind, w, that


def match_dualsoftmax_raw(feat, cu, cu_host: Sequence[int], npairs: int):
    val, _, ind, _, _ = _match_head(feat, None, cu, cu_host, npairs, None, None, 0, match=True, top2=False,
                                    sinkhorn=False)
    return val, ind


def _dev_scalar(v, device) -> torch.Tensor:
    """A 0-d / 1-element float32 device tensor for a learnable scalar (device tensors are
    passed through without a host read; Python numbers are uploaded)."""
    if isinstance(v, torch.Tensor):
        return v.detach().to(device=device, dtype=torch.float32).reshape(1).contiguous()
    return torch.tensor([float(v)], dtype=torch.float32, device=device)


def sinkhorn_correspondences(feat, xyz, cu, cu_host: Sequence[int], npairs: int, alpha,
                             beta, n_iters: int, slack: bool = True):
    """a13.  Returns (w [Tsrc] f32, t_hat [Tsrc,3] f32) for the src tokens.  alpha / beta:
    device tensors (the model's parameters -- read on the device, no sync) or floats.
    Differentiable in feat, alpha, beta (autograd.SinkhornFn)."""
    if _wants_grad(feat, alpha, beta):
        from .autograd import SinkhornFn
        dev = feat.device
        a = alpha if isinstance(alpha, torch.Tensor) else torch.tensor(float(alpha), device=dev)
        b = beta if isinstance(beta, torch.Tensor) else torch.tensor(float(beta), device=dev)
        return SinkhornFn.apply(_dev(feat, "feat", torch.float32), _dev(xyz, "xyz", torch.float32),
                                _dev(cu, "cu", torch.int32), list(cu_host), int(npairs), a, b, int(n_iters),
                                bool(slack))
    return sinkhorn_correspondences_raw(feat, xyz, cu, cu_host, npairs, alpha, beta, n_iters, slack)


def sinkhorn_correspondences_raw(feat, xyz, cu, cu_host: Sequence[int], npairs: int, alpha,
                                 beta, n_iters: int, slack: bool = True):
    # (slack: the library always pads the slack row / column, like the reference's sinkhorn())
    return _match_head(feat, xyz, cu, cu_host, npairs, alpha, beta, n_iters, match=False, top2=False,
                       sinkhorn=True)[3:]


def match_and_sinkhorn(feat, xyz, cu, cu_host: Sequence[int], npairs: int, alpha, beta, n_iters: int,
                       top2: bool = False):
    """match_dualsoftmax(_top2) and sinkhorn_correspondences of the same features in one call
    (spr_match_sinkhorn: the correlation matrices are computed and stored once).  Inference only -- with gradients
    wanted use the two operators.  Returns (val, val2 or None, ind, w, t_hat), bit for bit the separate results."""
    if _wants_grad(feat, alpha, beta):
        raise RuntimeError("match_and_sinkhorn is an inference operator (use match_dualsoftmax + sinkhorn_correspondences)")
    return _match_head(feat, xyz, cu, cu_host, npairs, alpha, beta, n_iters, match=True, top2=top2, sinkhorn=True)


def weighted_procrustes(a, b, w, pair_cu) -> torch.Tensor:
    """a12.  a,b [T,3], w [T] or None, pair_cu int32 [P+1] -> [P,3,4].  Differentiable in a, b, w
    (autograd.ProcrustesFn)."""
    if _wants_grad(a, b, w):
        from .autograd import ProcrustesFn
        return ProcrustesFn.apply(_dev(a, "a", torch.float32), _dev(b, "b", torch.float32),
                                  None if w is None else _dev(w, "w", torch.float32), _dev(pair_cu, "pair_cu", torch.int32))
    return weighted_procrustes_raw(a, b, w, pair_cu)


def weighted_procrustes_raw(a, b, w, pair_cu) -> torch.Tensor:
    a = _dev(a, "a", torch.float32)
    b = _dev(b, "b", torch.float32)
    if w is not None:
        w = _dev(w, "w", torch.float32)
    pair_cu = _dev(pair_cu, "pair_cu", torch.int32)
    p = pair_cu.numel() - 1
    out = torch.empty((p, 3, 4), dtype=torch.float32, device=a.device)
    _lib.check(_lib.lib().spr_weighted_procrustes(_ptr(a), _ptr(b), _ptr(w), _ptr(pair_cu), p,
                                                  _ptr(out), _stream(a)), "spr_weighted_procrustes")
    return out


# ---- losses (forward), SURVEY 8f row 1 -------------------------------------------
def overlap_pool(ov_prev, pool_idx, ns_prev: int):
    """One level of compute_overlaps (kpconv.py:552-578).  pool_idx int32 [Nq, W]."""
    ov_prev = _dev(ov_prev, "ov_prev", torch.float32)
    pool_idx = _dev(pool_idx, "pool_idx", torch.int32)
    nq, w = pool_idx.shape
    out = torch.empty((nq,), dtype=torch.float32, device=ov_prev.device)
    _lib.check(_lib.lib().spr_overlap_pool(_ptr(ov_prev), int(ns_prev), _ptr(pool_idx), pool_idx.stride(0), w,
                                           nq, _ptr(out), _stream(ov_prev)), "spr_overlap_pool")
    return out


def _loss_ws(n, m, d, device):
    return _workspace(_lib.lib().spr_loss_workspace_bytes(int(n), int(m), int(d)), device)


def bce_logits_mean(x, y):
    if _wants_grad(x):
        from .autograd import BCELogitsMeanFn
        return BCELogitsMeanFn.apply(_dev(x, "x", torch.float32), _dev(y, "y", torch.float32))
    return bce_logits_mean_raw(x, y)


def bce_logits_mean_raw(x, y):
    x = _dev(x, "x", torch.float32)
    y = _dev(y, "y", torch.float32)
    assert x.shape == y.shape and x.dim() == 1
    out = torch.empty((1,), dtype=torch.float32, device=x.device)
    ws = _loss_ws(x.numel(), 1, 32, x.device)
    _lib.check(_lib.lib().spr_bce_logits_mean(_ptr(x), _ptr(y), x.numel(), _ptr(out), _ptr(ws), ws.numel(),
                                              _stream(x)), "spr_bce_logits_mean")
    return out[0]


def infonce_pair(anchor_feat, positive_feat, anchor_xyz, pose_gt, positive_xyz, W, r_p: float, r_n: float):
    """InfoNCELossFull.compute_infonce for one pair; anchor_xyz is transformed by pose_gt [3,4] inside.
    Differentiable in the two feature sets and W (autograd.InfoNCEFn)."""
    if _wants_grad(anchor_feat, positive_feat, W):
        from .autograd import InfoNCEFn
        return InfoNCEFn.apply(_dev(anchor_feat, "anchor_feat", torch.float32),
                               _dev(positive_feat, "positive_feat", torch.float32), anchor_xyz, pose_gt, positive_xyz,
                               W, float(r_p), float(r_n))
    return infonce_pair_raw(anchor_feat, positive_feat, anchor_xyz, pose_gt, positive_xyz, W, r_p, r_n)


def infonce_pair_raw(anchor_feat, positive_feat, anchor_xyz, pose_gt, positive_xyz, W, r_p: float, r_n: float):
    a = _dev(anchor_feat, "anchor_feat", torch.float32)
    p = _dev(positive_feat, "positive_feat", torch.float32)
    n, d = a.shape
    m = p.shape[0]
    out = torch.empty((1,), dtype=torch.float32, device=a.device)
    ws = _loss_ws(n, m, d, a.device)
    _lib.check(_lib.lib().spr_infonce_pair(_ptr(a), n, _ptr(p), m, d, _ptr(_dev(anchor_xyz, "anchor_xyz", torch.float32)),
                                           _ptr(_dev(pose_gt, "pose_gt", torch.float32)),
                                           _ptr(_dev(positive_xyz, "positive_xyz", torch.float32)),
                                           _ptr(_dev(W, "W", torch.float32)), float(r_p), float(r_n), _ptr(out),
                                           _ptr(ws), ws.numel(), _stream(a)), "spr_infonce_pair")
    return out[0]


def circle_loss(src_feat, tgt_feat, src_kp, pose_gt, tgt_kp, r_p: float, r_n: float):
    """CircleLossFull(dist_type='euclidean') (feature_loss.py:160-243) of every pair of a step in one
    batched call.  Lists over the pairs: src_feat [N_b, D], tgt_feat [M_b, D], src_kp [N_b, 3] (transformed
    by pose_gt [B, 3, 4] inside), tgt_kp [M_b, 3].  Returns the per-pair losses [B]; the reference's loss
    is their mean (:236-243).  Differentiable in the features (autograd.CircleLossFn)."""
    B = len(src_feat)
    if not (len(tgt_feat) == len(src_kp) == len(tgt_kp) == B >= 1):
        raise ValueError("circle_loss: src_feat, tgt_feat, src_kp and tgt_kp need one entry per pair")
    for name, ts in (("src_feat", src_feat), ("tgt_feat", tgt_feat), ("src_kp", src_kp), ("tgt_kp", tgt_kp)):
        for t in ts:
            _dev(t, name)
    src_lens = [int(t.shape[0]) for t in src_feat]
    tgt_lens = [int(t.shape[0]) for t in tgt_feat]
    cat = lambda ts: ts[0] if len(ts) == 1 else torch.cat(list(ts))   # noqa: E731
    return circle_loss_packed(cat(src_feat), cat(tgt_feat), cat(src_kp), pose_gt, cat(tgt_kp), src_lens, tgt_lens,
                              r_p, r_n)


def circle_loss_packed(src_feat, tgt_feat, src_kp, pose_gt, tgt_kp, src_lens, tgt_lens, r_p: float, r_n: float):
    """circle_loss on packed rows: pair b owns src_lens[b] consecutive rows of src_feat / src_kp and
    tgt_lens[b] of tgt_feat / tgt_kp (host lengths, each >= 1)."""
    if _wants_grad(src_feat, tgt_feat):
        from .autograd import CircleLossFn
        return CircleLossFn.apply(_dev(src_feat, "src_feat", torch.float32), _dev(tgt_feat, "tgt_feat", torch.float32),
                                  src_kp, pose_gt, tgt_kp, tuple(src_lens), tuple(tgt_lens), float(r_p), float(r_n))
    return circle_loss_raw(src_feat, tgt_feat, src_kp, pose_gt, tgt_kp, src_lens, tgt_lens, r_p, r_n)


def _circle_args(src_feat, tgt_feat, src_kp, pose_gt, tgt_kp, src_lens, tgt_lens):
    a = _dev(src_feat, "src_feat", torch.float32)
    b = _dev(tgt_feat, "tgt_feat", torch.float32)
    xa = _dev(src_kp, "src_kp", torch.float32)
    xb = _dev(tgt_kp, "tgt_kp", torch.float32)
    pose = _dev(pose_gt, "pose_gt", torch.float32)
    src_lens, tgt_lens = [int(n) for n in src_lens], [int(m) for m in tgt_lens]
    B = len(src_lens)
    d = a.shape[1] if a.dim() == 2 else -1
    if not (B >= 1 and len(tgt_lens) == B and min(src_lens) >= 1 and min(tgt_lens) >= 1):
        raise ValueError(f"circle_loss: every pair needs >= 1 row on both sides (got {src_lens}, {tgt_lens})")
    if a.shape != (sum(src_lens), d) or b.shape != (sum(tgt_lens), d) or d < 4 or d % 4:
        raise ValueError(f"circle_loss: features {tuple(a.shape)} / {tuple(b.shape)} do not match the lengths, "
                         "or D is not a multiple of 4")
    if xa.shape != (sum(src_lens), 3) or xb.shape != (sum(tgt_lens), 3) or pose.numel() != 12 * B:
        raise ValueError("circle_loss: keypoints or pose_gt do not match the lengths")
    return a, b, xa, pose, xb, src_lens, tgt_lens


def circle_loss_raw(src_feat, tgt_feat, src_kp, pose_gt, tgt_kp, src_lens, tgt_lens, r_p: float, r_n: float):
    a, b, xa, pose, xb, src_lens, tgt_lens = _circle_args(src_feat, tgt_feat, src_kp, pose_gt, tgt_kp, src_lens,
                                                          tgt_lens)
    B, max_n, max_m = len(src_lens), max(src_lens), max(tgt_lens)
    L = _lib.lib()
    out = torch.empty((B,), dtype=torch.float32, device=a.device)
    ws = _workspace(L.spr_circle_loss_workspace_bytes(B, max_n, max_m), a.device)
    cu_a, cu_b = lengths_to_cu(src_lens, a.device), lengths_to_cu(tgt_lens, a.device)   # both alive until the launch
    _lib.check(L.spr_circle_loss(_ptr(a), _ptr(b), a.shape[1], _ptr(xa), _ptr(pose), _ptr(xb), _ptr(cu_a), _ptr(cu_b), B,
                                 max_n, max_m, float(r_p), float(r_n), _ptr(out), _ptr(ws), ws.numel(), _stream(a)),
               "spr_circle_loss")
    return out


def transform_l1_pair(pose_gt, pose_pred, xyz):
    if _wants_grad(pose_pred):
        from .autograd import TransformL1Fn
        return TransformL1Fn.apply(_dev(pose_gt, "pose_gt", torch.float32), pose_pred, _dev(xyz, "xyz", torch.float32))
    return transform_l1_pair_raw(pose_gt, pose_pred, xyz)


def transform_l1_pair_raw(pose_gt, pose_pred, xyz):
    xyz = _dev(xyz, "xyz", torch.float32)
    out = torch.empty((1,), dtype=torch.float32, device=xyz.device)
    ws = _loss_ws(xyz.shape[0], 1, 32, xyz.device)
    _lib.check(_lib.lib().spr_transform_l1_pair(_ptr(_dev(pose_gt, "pose_gt", torch.float32)),
                                                _ptr(_dev(pose_pred, "pose_pred", torch.float32)), _ptr(xyz),
                                                xyz.shape[0], _ptr(out), _ptr(ws), ws.numel(), _stream(xyz)),
               "spr_transform_l1_pair")
    return out[0]


def sum_scaled(values, scale: float = 1.0):
    values = _dev(values, "values", torch.float32)
    out = torch.empty((1,), dtype=torch.float32, device=values.device)
    _lib.check(_lib.lib().spr_sum_scaled(_ptr(values), values.numel(), float(scale), _ptr(out), _stream(values)),
               "spr_sum_scaled")
    return out[0]


def gather_rows(x, idx) -> torch.Tensor:
    if _wants_grad(x):
        from .autograd import GatherRowsFn
        return GatherRowsFn.apply(_dev(x, "x", torch.float32), _dev(idx, "idx", torch.int32))
    return gather_rows_raw(x, idx)


def gather_rows_raw(x, idx) -> torch.Tensor:
    x = _dev(x, "x", torch.float32)
    idx = _dev(idx, "idx", torch.int32)
    n_src, c = x.shape
    n = idx.numel()
    out = torch.empty((n, c), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().spr_gather_rows(_ptr(x), n_src, c, _ptr(idx), n, _ptr(out), _stream(x)),
               "spr_gather_rows")
    return out


def pair_gather(x, cu, src_idx, tgt_idx, cu_out, out=None, rows: Optional[int] = None) -> torch.Tensor:
    """Pair assembly (spr_pair_gather): x [T, C] holds the packed rows of the clouds described by cu [U+1]; the result
    [T_out, C] stacks 2P segments [src_0..src_{P-1}, tgt_0..tgt_{P-1}], segment s a copy of cloud src_idx[s] (s < P) or
    tgt_idx[s - P].  cu_out [2P+1]: the prefix of the output segment lengths, built on the host from the host-side
    cloud lengths (lengths_to_cu).  T_out is taken from `out`, else from `rows`; only when neither is given is it read
    back from cu_out (a device->host read).  One launch for all pairs, any C (tokens: 256, coordinates: 3)."""
    x = _dev(x, "x", torch.float32)
    cu = _dev(cu, "cu", torch.int32)
    src_idx = _dev(src_idx, "src_idx", torch.int32)
    tgt_idx = _dev(tgt_idx, "tgt_idx", torch.int32)
    cu_out = _dev(cu_out, "cu_out", torch.int32)
    npairs = src_idx.numel()
    if x.dim() != 2 or tgt_idx.numel() != npairs or cu_out.numel() != 2 * npairs + 1 or cu.numel() < 2:
        raise ValueError("pair_gather: x [T, C], cu [U+1], src_idx [P], tgt_idx [P], cu_out [2P+1]")
    t_in, c = x.shape
    if out is not None:
        t_out = int(out.shape[0])
    else:
        t_out = int(rows) if rows is not None else int(cu_out[-1])
        out = torch.empty((t_out, c), dtype=torch.float32, device=x.device)
    if (not out.is_cuda or out.device != x.device or out.dtype != torch.float32 or not out.is_contiguous()
            or tuple(out.shape) != (t_out, c)):
        raise ValueError("pair_gather: out must be a contiguous float32 [T_out, C] tensor on x's device")
    _lib.check(_lib.lib().spr_pair_gather(_ptr(x), t_in, c, _ptr(cu), cu.numel() - 1, _ptr(src_idx), _ptr(tgt_idx),
                                          npairs, _ptr(cu_out), t_out, _ptr(out), _stream(x)), "spr_pair_gather")
    return out
