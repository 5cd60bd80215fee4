"""The projections of the KPConv decoder (KPFDecoder, kpconv.py): a UnaryBlock whose input is the concatenation of the
running features and a skip tensor, with or without a nearest upsample in front.

    upsample_unary(xc, xs, idx, weight)   [ xc[idx[:, 0]] | xs ] . weight^T      (NearestUpsampleBlock + cat + mlp)
    concat_unary(x, xs, weight)           [ x | xs ] . weight^T                  (cat + mlp)

Neither writes the concatenated tensor.  upsample_unary has two routes:

  fused      one spr_upsample_unary call (csrc/upsample_unary.hip): the GEMM gathers the coarse rows while it stages its
             tiles, so the gathered tensor is never written either.  Forward only; taken under torch.no_grad() where
             spr_upsample_unary_supported says the fused call is the default for the shape.
  operator   ops.gather_rows on column 0, then concat_unary: ops.linear on the skip columns of the weight, then
             ops.linear on the coarse columns with the first result as `residual`.  Every piece has a HIP backward, so
             this is the training route (autograd), and the inference route of shapes without a fused kernel.

route=None picks as described; 'fused' / 'operator' force one (tests, scripts/decoder_bench.py).
"""
import ctypes

import torch

from . import _lib, ops
from .ops import _dev, _ptr, _stream


def supported(kc: int, ks: int, n_out: int) -> bool:
    """Whether the fused call is the default for this shape (spr_upsample_unary_supported)."""
    return bool(_lib.lib().spr_upsample_unary_supported(int(kc), int(ks), int(n_out)))


def concat_unary(x, xs, weight) -> torch.Tensor:
    """[ x | xs ] . weight^T without the concatenated tensor: the skip columns first, the leading columns on top of
    them (residual).  Differentiable in all three (ops.linear)."""
    kx = x.shape[1]
    if weight.shape[1] != kx + xs.shape[1] or x.shape[0] != xs.shape[0]:
        raise ValueError(f"concat_unary: x {tuple(x.shape)}, xs {tuple(xs.shape)}, weight {tuple(weight.shape)}")
    y = ops.linear(xs, weight[:, kx:].contiguous())
    return ops.linear(x, weight[:, :kx].contiguous(), residual=y)


def _column0(idx) -> torch.Tensor:
    return (idx if idx.dim() == 1 else idx[:, 0]).contiguous().to(torch.int32)


def upsample_unary_fused(xc, xs, idx, weight) -> torch.Tensor:
    """One spr_upsample_unary call.  idx: int32 [n] or [n, w] with any positive row stride (the pyramid's upsamples
    matrix, or a column slice of it, goes in as it is: only column 0 is read); other index tensors are converted."""
    xc = _dev(xc, "xc", torch.float32)
    xs = _dev(xs, "xs", torch.float32)
    weight = _dev(weight.detach(), "weight", torch.float32)
    if not isinstance(idx, torch.Tensor) or not idx.is_cuda:
        raise RuntimeError("idx must be a tensor on the MI355X device")
    if idx.dtype != torch.int32 or idx.dim() not in (1, 2) or (idx.shape[0] > 1 and idx.stride(0) < 1):
        idx = _column0(idx)         # an expanded row (stride 0) as well: the kernel reads idx[i * stride]
    (nc, kc), (n, ks), n_out = xc.shape, xs.shape, weight.shape[0]
    if idx.shape[0] != n or weight.shape[1] != kc + ks:
        raise ValueError(f"upsample_unary: xc {tuple(xc.shape)}, xs {tuple(xs.shape)}, idx {tuple(idx.shape)}, "
                         f"weight {tuple(weight.shape)}")
    stride = int(idx.stride(0)) if idx.shape[0] > 1 else 1
    out = torch.empty((n, n_out), dtype=torch.float32, device=xs.device)
    if n == 0:
        return out
    L = _lib.lib()
    ws = ops._workspace(L.spr_upsample_unary_workspace_size(), xs.device)
    cr, cr_n = ops._get_range(xc)
    sr, sr_n = ops._get_range(xs)
    wr, wr_n = ops._static_range(weight)
    orng = torch.empty((ops._RANGE_CAP,), dtype=torch.float32, device=xs.device)
    on = ctypes.c_int(0)
    _lib.check(L.spr_upsample_unary(_ptr(xc), nc, kc, _ptr(xs), n, ks, _ptr(idx), stride, _ptr(weight), n_out,
                                    _ptr(out), _ptr(cr), int(cr_n), _ptr(sr), int(sr_n), _ptr(wr), int(wr_n),
                                    _ptr(orng), ops._RANGE_CAP, ctypes.byref(on), _ptr(ws), ws.numel(), _stream(xs)),
               "spr_upsample_unary")
    ops._set_range(out, orng, on.value)
    return out


def upsample_unary(xc, xs, idx, weight, route=None) -> torch.Tensor:
    """y = [ xc[idx[:, 0]] | xs ] . weight^T; an index outside [0, len(xc)) reads a zero row (closest_pool)."""
    if route not in (None, 'fused', 'operator'):
        raise ValueError(f"route must be None, 'fused' or 'operator', got {route!r}")
    if route is None:
        grad = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad
                                               for t in (xc, xs, weight))
        route = 'fused' if not grad and supported(xc.shape[1], xs.shape[1], weight.shape[0]) else 'operator'
    if route == 'fused':
        return upsample_unary_fused(xc, xs, idx, weight)
    if xs.shape[0] == 0:
        return torch.empty((0, weight.shape[0]), dtype=torch.float32, device=xs.device)
    return concat_unary(ops.gather_rows(xc, _column0(idx)), xs, weight)
