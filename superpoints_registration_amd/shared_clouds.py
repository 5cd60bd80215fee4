"""Training over shared clouds: a step's pairs drawn from one scene or one drive reuse clouds, and a cloud that k pairs
use need not go k times through the pyramid, the KPConv encoder and their backward.

RegTR.forward accepts, instead of `src_xyz` / `tgt_xyz`,

    batch = {"clouds": [Tensor(N_i, 3), ...],          # device, float32
             "pairs":  [(src_index, tgt_index), ...],   # P pairs into clouds
             "pose":   Tensor(P, 3, 4)}                 # src -> tgt, one per pair (training / validation)

encodes the clouds once (with gradients when training), lays tokens and points out per pair with spr_pair_gather and runs
the unchanged per-pair half.  What that needs beside the inference route (RegTR.encode / register) lives here:

  * PairLayout        the host bookkeeping of a pair list over one encode call: the cloud every segment copies, the use
                      list of every cloud in CSR form (ascending segment index) and the per-level cu_out, from the host
                      lengths of the pyramid -- one upload, no device->host read;
  * pair_gather       ops.pair_gather on the tape: the backward (spr_pair_gather_bwd) sums, per cloud row, the gradient
                      rows of every segment that copied it, in the stored order;
  * overlap_pyramid   compute_overlaps for per-pair masks over the encode call's pool matrices, which index the cloud
                      layout (spr_overlap_pool_pairs per level).
"""
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from .ops import _dev, _ptr, _stream


def _index(i, n: int) -> int:
    if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= i < n:
        raise ValueError(f"cloud index {i!r} is not an index in range({n})")
    return int(i)


def check_batch(batch) -> Tuple[list, List[int], List[int]]:
    """(clouds, src indices, tgt indices) of a cloud / pair batch; everything that can be refused is refused here, on
    the host, before any launch."""
    if 'pairs' not in batch:
        raise ValueError("a batch of 'clouds' needs 'pairs': a list of (src_index, tgt_index)")
    clouds = list(batch['clouds'])
    if not clouds:
        raise ValueError("empty cloud list")
    pairs = [tuple(p) for p in batch['pairs']]
    if not pairs:
        raise ValueError("empty pair list")
    if any(len(p) != 2 for p in pairs):
        raise ValueError("pairs are (src_index, tgt_index)")
    src = [_index(p[0], len(clouds)) for p in pairs]
    tgt = [_index(p[1], len(clouds)) for p in pairs]
    for side, idx in (('src_xyz', src), ('tgt_xyz', tgt)):
        if side in batch:   # the per-pair views an earlier forward of this batch left there are the only legal content
            views = list(batch[side])
            if len(views) != len(idx) or any(v is not clouds[i] for v, i in zip(views, idx)):
                raise ValueError(f"a batch holds either 'clouds' and 'pairs' or 'src_xyz' / 'tgt_xyz', not both "
                                 f"('{side}' is not the per-pair view of 'clouds')")
    pose = batch.get('pose')
    if pose is not None and (not isinstance(pose, torch.Tensor) or pose.dim() != 3 or pose.shape[0] != len(pairs)):
        raise ValueError(f"'pose' must hold one [3, 4] transform per pair: {len(pairs)} pairs, pose "
                         f"{tuple(pose.shape) if isinstance(pose, torch.Tensor) else type(pose)}")
    for key in ('src_overlap', 'tgt_overlap', 'pair_key'):
        if batch.get(key) is not None and len(batch[key]) != len(pairs):
            raise ValueError(f"'{key}' must hold one entry per pair: {len(pairs)} pairs, {len(batch[key])} entries")
    clouds = [_dev(c, f"clouds[{i}]", torch.float32) for i, c in enumerate(clouds)]      # CPU tensor: raises
    if any(c.dim() != 2 or c.shape[1] != 3 or c.shape[0] == 0 for c in clouds):
        raise ValueError("every cloud must be a non-empty [N, 3] tensor")
    return clouds, src, tgt


def pair_views(batch) -> Tuple[list, list]:
    """The per-pair lists [clouds[i] ...], [clouds[j] ...] of a checked batch: the cloud tensors themselves, no copy."""
    clouds, (src, tgt) = list(batch['clouds']), zip(*[tuple(p) for p in batch['pairs']])
    return [clouds[i] for i in src], [clouds[j] for j in tgt]


def use_list(seg_cloud: Sequence[int], n_clouds: int) -> Tuple[np.ndarray, np.ndarray]:
    """(use_ptr [U+1], use_seg [S]): use_seg[use_ptr[c]:use_ptr[c+1]] are the segments that copy cloud c, ascending."""
    seg_cloud = np.asarray(seg_cloud, dtype=np.int64)
    use_seg = np.argsort(seg_cloud, kind='stable').astype(np.int32)       # stable: ascending segment inside a cloud
    use_ptr = np.zeros(n_clouds + 1, dtype=np.int32)
    use_ptr[1:] = np.cumsum(np.bincount(seg_cloud, minlength=n_clouds))
    return use_ptr, use_seg


class PairLayout:
    """Where the rows of P pairs lie relative to one encode call of U clouds, on every level of its pyramid.  Segments
    are ordered [src_0..src_{P-1}, tgt_0..tgt_{P-1}].

      src, tgt     the pairs' cloud indices (host lists)
      seg_cloud    [2P]   the cloud each segment copies
      use_ptr      [U+1], use_seg [2P]   per cloud, the segments that copy it, in ascending segment index
      seg_lens[l]  [2P]   host: the segments' row counts on level l;   rows[l]: their sum
      cu_out[l]    [2P+1] the exclusive prefix of seg_lens[l]
    The device tensors (int32) are slices of ONE uploaded array, made when a device is given."""

    def __init__(self, src: Sequence[int], tgt: Sequence[int], lens_per_level: Sequence[Sequence[int]], device=None):
        self.src, self.tgt = [int(i) for i in src], [int(j) for j in tgt]
        if not self.src or len(self.src) != len(self.tgt):
            raise ValueError("PairLayout: src and tgt index lists of one non-zero length")
        self.npairs = len(self.src)
        self.n_clouds = len(lens_per_level[0])
        seg_cloud = np.asarray(self.src + self.tgt, dtype=np.int32)
        if seg_cloud.min() < 0 or seg_cloud.max() >= self.n_clouds:
            raise ValueError(f"PairLayout: a pair index lies outside range({self.n_clouds})")
        use_ptr, use_seg = use_list(seg_cloud, self.n_clouds)
        self.seg_lens, cu_out = [], []
        for lens in lens_per_level:
            if len(lens) != self.n_clouds:
                raise ValueError("PairLayout: every level lists one length per cloud")
            seg = [int(lens[c]) for c in seg_cloud]
            self.seg_lens.append(seg)
            cu = np.zeros(len(seg) + 1, dtype=np.int64)
            cu[1:] = np.cumsum(seg)
            if cu[-1] >= 2 ** 31:
                raise ValueError("PairLayout: more than 2^31 - 1 rows on one level")
            cu_out.append(cu.astype(np.int32))
        self.rows = [int(cu[-1]) for cu in cu_out]
        self.host = dict(seg_cloud=seg_cloud, use_ptr=use_ptr, use_seg=use_seg, cu_out=cu_out)
        self.seg_cloud = self.use_ptr = self.use_seg = self.cu_out = None
        if device is not None:
            parts = [seg_cloud, use_ptr, use_seg] + cu_out
            dev = torch.from_numpy(np.concatenate(parts)).to(device)          # the one copy
            cut = np.concatenate([[0], np.cumsum([p.size for p in parts])])
            views = [dev[cut[k]:cut[k + 1]] for k in range(len(parts))]
            self.seg_cloud, self.use_ptr, self.use_seg, self.cu_out = views[0], views[1], views[2], views[3:]

    @property
    def levels(self) -> int:
        return len(self.seg_lens)


# --------------------------------------------------------------------------------------------- #
def pair_gather_bwd(gy, cu, use_ptr, use_seg, cu_out, rows: int, out=None) -> torch.Tensor:
    """gx [rows, C] from gy [T_out, C] (spr_pair_gather_bwd): row i of cloud c is the sum, in the stored order of the use
    list, of rows cu_out[s] + i of gy over the segments s that copy c; rows of unused clouds are zeros.  Every row of
    the result is written."""
    gy = _dev(gy, "gy", torch.float32)
    cu = _dev(cu, "cu", torch.int32)
    use_ptr = _dev(use_ptr, "use_ptr", torch.int32)
    use_seg = _dev(use_seg, "use_seg", torch.int32)
    cu_out = _dev(cu_out, "cu_out", torch.int32)
    nseg = use_seg.numel()
    if (gy.dim() != 2 or nseg < 2 or nseg % 2 or cu_out.numel() != nseg + 1 or cu.numel() < 2
            or use_ptr.numel() != cu.numel()):
        raise ValueError("pair_gather_bwd: gy [T_out, C], cu [U+1], use_ptr [U+1], use_seg [2P], cu_out [2P+1]")
    t_out, c = gy.shape
    t_in = int(rows) if out is None else int(out.shape[0])
    if out is None:
        out = torch.empty((t_in, c), dtype=torch.float32, device=gy.device)
    if (not out.is_cuda or out.device != gy.device or out.dtype != torch.float32 or not out.is_contiguous()
            or tuple(out.shape) != (t_in, c)):
        raise ValueError("pair_gather_bwd: out must be a contiguous float32 [rows, C] tensor on gy's device")
    _lib.check(_lib.lib().spr_pair_gather_bwd(_ptr(gy), t_out, c, _ptr(cu), cu.numel() - 1, _ptr(use_ptr),
                                              _ptr(use_seg), nseg // 2, _ptr(cu_out), t_in, _ptr(out), _stream(gy)),
               "spr_pair_gather_bwd")
    return out


class PairGatherFn(torch.autograd.Function):
    """ops.pair_gather over the token rows; backward = spr_pair_gather_bwd (a cloud's gradient is the sum over every
    segment that copied it, in ascending segment order).  The index arguments carry no gradient."""

    @staticmethod
    def forward(ctx, x, cu, seg_cloud, use_ptr, use_seg, cu_out, rows):
        npairs = seg_cloud.numel() // 2
        with torch.no_grad():
            y = ops.pair_gather(x, cu, seg_cloud[:npairs], seg_cloud[npairs:], cu_out, rows=rows)
        # max |y| <= max |x| (all rows: equal): the published range of x still bounds y, and the consumer scales the
        # gathered tokens exactly as it scales the tokens of a forward on pair lists
        r, n = ops._get_range(x)
        if r is not None:
            ops._set_range(y, r, n)
        ctx.save_for_backward(cu, use_ptr, use_seg, cu_out)
        ctx.rows_in = int(x.shape[0])
        return y

    @staticmethod
    def backward(ctx, gy):
        cu, use_ptr, use_seg, cu_out = ctx.saved_tensors
        return (pair_gather_bwd(gy, cu, use_ptr, use_seg, cu_out, ctx.rows_in),) + (None,) * 6


def pair_gather(x, cu, layout: PairLayout, level: int = -1) -> torch.Tensor:
    """Rows of the clouds (x [T, C], packed by cu [U+1]) laid out per pair on `level` of the layout's pyramid:
    differentiable in x when gradients are enabled and x requires them, ops.pair_gather otherwise."""
    P = layout.npairs
    if torch.is_grad_enabled() and isinstance(x, torch.Tensor) and x.requires_grad:
        return PairGatherFn.apply(_dev(x, "x", torch.float32), _dev(cu, "cu", torch.int32), layout.seg_cloud,
                                  layout.use_ptr, layout.use_seg, layout.cu_out[level], layout.rows[level])
    return ops.pair_gather(x, cu, layout.seg_cloud[:P], layout.seg_cloud[P:], layout.cu_out[level],
                           rows=layout.rows[level])


# --------------------------------------------------------------------------------------------- #
def overlap_pool_pairs(ov_prev, pool_idx, cu_prev, cu_cur, seg_cloud, cu_out_prev, cu_out_cur, rows: int) -> torch.Tensor:
    """One level of compute_overlaps for labels in pair layout (spr_overlap_pool_pairs): ov_prev [sum of the segments'
    previous-level rows], pool_idx [N_p, W] the encode call's cloud-layout pool matrix, cu_prev / cu_cur [U+1] the
    clouds' prefixes on the two levels, seg_cloud [2P], cu_out_prev / cu_out_cur [2P+1]; returns [rows] values of this
    level in pair layout.  The arithmetic of ops.overlap_pool, bit for bit."""
    ov_prev = _dev(ov_prev, "ov_prev", torch.float32)
    pool_idx = _dev(pool_idx, "pool_idx", torch.int32)
    cu_prev, cu_cur = _dev(cu_prev, "cu_prev", torch.int32), _dev(cu_cur, "cu_cur", torch.int32)
    seg_cloud = _dev(seg_cloud, "seg_cloud", torch.int32)
    cu_out_prev = _dev(cu_out_prev, "cu_out_prev", torch.int32)
    cu_out_cur = _dev(cu_out_cur, "cu_out_cur", torch.int32)
    nseg = seg_cloud.numel()
    if (ov_prev.dim() != 1 or pool_idx.dim() != 2 or nseg < 2 or nseg % 2 or cu_out_prev.numel() != nseg + 1
            or cu_out_cur.numel() != nseg + 1 or cu_prev.numel() < 2 or cu_cur.numel() != cu_prev.numel()):
        raise ValueError("overlap_pool_pairs: ov_prev [n], pool_idx [N, W], cu_prev / cu_cur [U+1], seg_cloud [2P], "
                         "cu_out_prev / cu_out_cur [2P+1]")
    nq, w = int(rows), pool_idx.shape[1]
    out = torch.empty((nq,), dtype=torch.float32, device=ov_prev.device)
    _lib.check(_lib.lib().spr_overlap_pool_pairs(_ptr(ov_prev), ov_prev.numel(), _ptr(pool_idx), pool_idx.stride(0), w,
                                                 pool_idx.shape[0], _ptr(cu_prev), _ptr(cu_cur), cu_prev.numel() - 1,
                                                 _ptr(seg_cloud), nseg // 2, _ptr(cu_out_prev), _ptr(cu_out_cur), nq,
                                                 _ptr(out), _stream(ov_prev)), "spr_overlap_pool_pairs")
    return out


def overlap_pyramid(ov, meta, layout: PairLayout) -> dict:
    """compute_overlaps (kpconv.py:552-578) for per-point masks in pair layout (ov [sum of the pairs' points], ordered
    [src_0..src_{P-1}, tgt_0..tgt_{P-1}]) over the pyramid of an encode call of the shared clouds: {'pyr_l': values of
    level l in pair layout}.  With every cloud used once, in order, this is the pyramid RegTR.compute_loss builds."""
    levels = len(meta['points'])
    if layout.levels != levels:
        raise ValueError(f"overlap_pyramid: the layout describes {layout.levels} levels, the pyramid has {levels}")
    # masks longer than their clouds are read the way compute_loss reads them on pair lists: concatenated, by position
    if ov.numel() < layout.rows[0]:
        raise ValueError(f"overlap_pyramid: {ov.numel()} labels for {layout.rows[0]} points of the pairs")
    pyr = {'pyr_0': ov}
    for p in range(1, levels):
        ov = overlap_pool_pairs(ov, meta['_i32'][('pools', p - 1)], meta['_cu'][p - 1], meta['_cu'][p],
                                layout.seg_cloud, layout.cu_out[p - 1], layout.cu_out[p], layout.rows[p])
        pyr[f'pyr_{p}'] = ov
    return pyr
