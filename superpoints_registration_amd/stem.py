"""The encoder's first block in inference: Cin = 1 KPConv + per-cloud InstanceNorm + LeakyReLU as one library call
(spr_kpconv_stem, csrc/kpconv.hip) that never writes the raw [Nq, Cout] tensor.

    stem_route(...)   whether SimpleBlock.forward takes the fused call for these inputs
    kpconv_stem(...)  the call; refuses what stem_route refuses (no fallback inside)

Everything else -- training, use_batch_norm off, wider inputs, a Cout that is no multiple of 16, more than 16 kernel
points -- stays on ops.kpconv + ops.instnorm.
"""
from typing import Optional

import torch

from . import _lib, ops


def stem_shape_ok(cin: int, cout: int, n_kp: int) -> bool:
    """The shapes spr_kpconv_stem has kernels for (spr_kpconv_stem_supported restated, so that the predicate needs
    no library): one input channel, Cout a multiple of 16, at most 16 kernel points."""
    return cin == 1 and cout >= 16 and cout % 16 == 0 and 1 <= n_kp <= 16


def few_shape_ok(cin: int, cout: int, n_kp: int) -> bool:
    """The shapes spr_kpconv_fwd (impl 0 and 2) runs on the small-Cin kernel k_kpconv_few (spr_kpconv_few_supported
    restated): 2 to 8 input channels -- a first block fed per-point input features -- any Cout, at most 16 kernel
    points.  Such a block is KPConv + instnorm; the fused stem stays Cin = 1."""
    return 2 <= cin <= 8 and cout >= 1 and 1 <= n_kp <= 16


def stem_predicate(on_gpu: bool, wants_grad: bool, use_bn: bool, x_channels: int, weights_shape) -> bool:
    """The routing rule itself, on plain values: features on the GPU, nothing asks for a gradient, the block
    normalises (use_batch_norm), and the shape has a kernel."""
    if not on_gpu or wants_grad or not use_bn or len(weights_shape) != 3:
        return False
    n_kp, cin, cout = (int(v) for v in weights_shape)
    return int(x_channels) == cin and stem_shape_ok(cin, cout, n_kp)


def stem_route(x, weights, use_bn: bool) -> bool:
    """True when SimpleBlock.forward runs as spr_kpconv_stem for these tensors (stem_predicate of their state)."""
    if not (isinstance(x, torch.Tensor) and x.dim() == 2):
        return False
    return stem_predicate(x.is_cuda, ops._wants_grad(x, weights), bool(use_bn), x.shape[1], tuple(weights.shape))


def kpconv_stem(q_pts, s_pts, nbr, x, weights, kernel_points, kp_extent: float, cu, eps: float = 1e-5,
                slope: float = 0.1, rows_sorted: bool = False, max_len: Optional[int] = None,
                return_stats: bool = False):
    """lrelu(InstanceNorm_per_cloud(kpconv(q_pts, s_pts, nbr, x, weights, ...)), slope) for x [ns, 1]; the output
    carries its published range like ops.instnorm's.  return_stats: (out, mean [nb, cout], rstd [nb, cout])."""
    q_pts = ops._dev(q_pts, "q_pts", torch.float32)
    s_pts = ops._dev(s_pts, "s_pts", torch.float32)
    x = ops._dev(x, "x", torch.float32)
    weights = ops._dev(weights.detach(), "weights", torch.float32)
    kernel_points = ops._dev(kernel_points, "kernel_points", torch.float32)
    cu = ops._dev(cu, "cu", torch.int32)
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
    if not stem_shape_ok(int(cin), int(cout), int(n_kp)) or x.shape != (ns, 1):
        raise RuntimeError(f"kpconv_stem: no kernel for x {tuple(x.shape)}, weights {tuple(weights.shape)}")
    nb = cu.numel() - 1
    max_len = nq if max_len is None else max(1, min(int(max_len), nq))
    L = _lib.lib()
    ws = ops._workspace(L.spr_kpconv_stem_workspace_size(nq, ns, nb, max_len, cout), x.device)
    out = torch.empty((nq, cout), dtype=torch.float32, device=x.device)
    cnt = ops._STREAM_SLOTS
    rng = ops._zero_slots(cnt, x.device)
    st = torch.empty((2, nb, cout), dtype=torch.float32, device=x.device) if return_stats else None
    _lib.check(L.spr_kpconv_stem(ops._ptr(q_pts), nq, ops._ptr(s_pts), ns, ops._ptr(nbr), int(stride), kmax,
                                 int(bool(rows_sorted)), ops._ptr(x), ops._ptr(weights), cout,
                                 ops._ptr(kernel_points), n_kp, float(kp_extent), ops._ptr(cu), nb, max_len,
                                 float(eps), float(slope), ops._ptr(out), ops._ptr(rng), cnt,
                                 ops._ptr(None if st is None else st[0]), ops._ptr(None if st is None else st[1]),
                                 ops._ptr(ws), ws.numel(), ops._stream(x)), "spr_kpconv_stem")
    ops._set_range(out, rng, cnt)
    return (out, st[0], st[1]) if return_stats else out
