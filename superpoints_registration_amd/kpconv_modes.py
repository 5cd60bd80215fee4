"""KPConv in the reference's other modes (csrc/kpconv_modes.hip): KP_influence in {'constant', 'linear', 'gaussian'} x
aggregation_mode in {'sum', 'closest'}, rigid kernel points.

    kpconv(...)       forward, differentiable in x and weights (KPConvModesFn)
    kpconv_raw(...)   the plain launch (spr_kpconv_modes_fwd)

KPConv.forward (kpconv_blocks.py) calls ops.kpconv for linear / sum and this module for the other five combinations;
linear / sum is valid here too -- the cross-check of these kernels against the shipped ones.  Deformable and modulated
KPConv (linear / sum only, opt-in) is the `deformable` subpackage.
"""
import torch

from . import _lib, ops

INFLUENCES = {'constant': 0, 'linear': 1, 'gaussian': 2}     # SPR_KP_CONSTANT / _LINEAR / _GAUSSIAN
AGGREGATIONS = {'sum': 0, 'closest': 1}                      # SPR_KP_SUM / _CLOSEST


def mode_codes(KP_influence: str, aggregation_mode: str):
    """(influence, aggregation) as the C ABI's integers; ValueError for an unknown string, like the reference's
    KPConv.forward (kpconv_blocks.py:377, :385)."""
    if KP_influence not in INFLUENCES:
        raise ValueError('Unknown influence function type (config.KP_influence)')
    if aggregation_mode not in AGGREGATIONS:
        raise ValueError("Unknown convolution mode. Should be 'closest' or 'sum'")
    return INFLUENCES[KP_influence], AGGREGATIONS[aggregation_mode]


def is_default_mode(KP_influence: str, aggregation_mode: str) -> bool:
    """The mode of ops.kpconv, the stem and the ring kernels."""
    return KP_influence == 'linear' and aggregation_mode == 'sum'


def _index_rows(nbr):
    """int32 neighbour matrix with unit column stride, and its row stride."""
    if not nbr.is_cuda:
        raise RuntimeError("neighb_inds must be on the device")
    if nbr.dtype != torch.int32:
        nbr = nbr.to(torch.int32)
    if not (nbr.stride(1) == 1 and nbr.shape[1] > 0):
        nbr = nbr.contiguous()
        return nbr, nbr.shape[1]
    return nbr, nbr.stride(0)


def kpconv(q_pts, s_pts, nbr, x, weights, kernel_points, kp_extent: float, KP_influence: str = 'linear',
           aggregation_mode: str = 'sum', impl: int = 0) -> torch.Tensor:
    """KPConv.forward in the given mode.  nbr may be int32 or int64 [Nq, K] (possibly a column slice)."""
    infl, agg = mode_codes(KP_influence, aggregation_mode)
    if ops._wants_grad(x, weights):
        return KPConvModesFn.apply(ops._dev(q_pts, "q_pts", torch.float32), ops._dev(s_pts, "s_pts", torch.float32),
                                   nbr, ops._dev(x, "x", torch.float32), weights, kernel_points, float(kp_extent),
                                   infl, agg, int(impl))
    return kpconv_raw(q_pts, s_pts, nbr, x, weights, kernel_points, kp_extent, infl, agg, impl)


def kpconv_raw(q_pts, s_pts, nbr, x, weights, kernel_points, kp_extent: float, influence: int, aggregation: int,
               impl: int = 0) -> torch.Tensor:
    q_pts = ops._dev(q_pts, "q_pts", torch.float32)
    s_pts = ops._dev(s_pts, "s_pts", torch.float32)
    x = ops._dev(x, "x", torch.float32)
    weights = ops._dev(weights, "weights", torch.float32)
    kernel_points = ops._dev(kernel_points, "kernel_points", torch.float32)
    nbr, stride = _index_rows(nbr)
    nq, ns, kmax = q_pts.shape[0], s_pts.shape[0], nbr.shape[1]
    n_kp, cin, cout = weights.shape
    assert x.shape == (ns, cin), (x.shape, ns, cin)
    L = _lib.lib()
    ws = ops._workspace(L.spr_kpconv_modes_workspace_size(nq, ns, cin, cout), x.device)
    out = torch.empty((nq, cout), dtype=torch.float32, device=x.device)
    xr, xr_n = ops._get_range(x)
    wr, wr_n = ops._static_range(weights)
    wplanes = None
    if impl == 0 and n_kp == 15 and cin % 32 == 0 and cout % 32 == 0 and cout <= 256 and wr is not None:
        wplanes = ops._kpconv_wplanes(weights, wr, wr_n)      # the planes (and their cache) of ops.kpconv
    _lib.check(L.spr_kpconv_modes_fwd(ops._ptr(q_pts), nq, ops._ptr(s_pts), ns, ops._ptr(nbr), int(stride), kmax,
                                      ops._ptr(x), cin, ops._ptr(weights), cout, ops._ptr(kernel_points), n_kp,
                                      float(kp_extent), int(influence), int(aggregation), ops._ptr(out), int(impl),
                                      ops._ptr(xr), int(xr_n), ops._ptr(wr), int(wr_n), ops._ptr(wplanes),
                                      ops._ptr(ws), ws.numel(), ops._stream(x)), "spr_kpconv_modes_fwd")
    return out


def weighted_features(q_pts, s_pts, nbr, x, kernel_points, kp_extent: float, influence: int, aggregation: int):
    """wf [nq, n_kp * cin] (un-normalised) and cnt [nq] = max(1, neighbour count) as the forward forms them."""
    nbr, stride = _index_rows(nbr)
    nq, ns, kmax = q_pts.shape[0], s_pts.shape[0], nbr.shape[1]
    n_kp, cin = kernel_points.shape[0], x.shape[1]
    L = _lib.lib()
    wf = torch.empty((nq, n_kp * cin), dtype=torch.float32, device=x.device)
    cnt = torch.empty((nq,), dtype=torch.float32, device=x.device)
    ws = ops._workspace(L.spr_kpconv_modes_weighted_features_workspace_size(ns), x.device)
    _lib.check(L.spr_kpconv_modes_weighted_features(ops._ptr(q_pts), nq, ops._ptr(s_pts), ns, ops._ptr(nbr),
                                                    int(stride), kmax, ops._ptr(x), cin, ops._ptr(kernel_points),
                                                    n_kp, float(kp_extent), int(influence), int(aggregation),
                                                    ops._ptr(wf), ops._ptr(cnt), ops._ptr(ws), ws.numel(),
                                                    ops._stream(x)), "spr_kpconv_modes_weighted_features")
    return wf, cnt


def bwd_dx(q_pts, s_pts, nbr, cin: int, kernel_points, kp_extent: float, influence: int, aggregation: int, dwf):
    """dx [ns, cin] = scatter of influence x d wf (order-independent sums); dwf's published range is used if it has one."""
    nbr, stride = _index_rows(nbr)
    nq, ns, kmax = q_pts.shape[0], s_pts.shape[0], nbr.shape[1]
    n_kp = kernel_points.shape[0]
    L = _lib.lib()
    dx = torch.empty((ns, cin), dtype=torch.float32, device=dwf.device)
    ws = ops._workspace(L.spr_scatter_workspace_bytes(ns, cin), dwf.device)
    dr, dr_n = ops._get_range(dwf)
    _lib.check(L.spr_kpconv_modes_bwd_dx(ops._ptr(q_pts), nq, ops._ptr(s_pts), ns, ops._ptr(nbr), int(stride), kmax,
                                         cin, ops._ptr(kernel_points), n_kp, float(kp_extent), int(influence),
                                         int(aggregation), ops._ptr(dwf), ops._ptr(dr), int(dr_n), ops._ptr(dx),
                                         ops._ptr(ws), ws.numel(), ops._stream(dwf)), "spr_kpconv_modes_bwd_dx")
    return dx


class KPConvModesFn(torch.autograd.Function):
    """spr_kpconv_modes_fwd; backward with autograd.KPConvFn's factorisation (kpconv_blocks.py:388-412
    differentiated; the influences and the arg-min are constants: kernel points are not trained):
       g = dout / count;  d wf = g W_flat^T;  dW_flat = wf^T g;  dx = scatter(influence * d wf)."""

    @staticmethod
    def forward(ctx, q_pts, s_pts, nbr, x, weights, kernel_points, kp_extent, influence, aggregation, impl):
        with torch.no_grad():
            y = kpconv_raw(q_pts, s_pts, nbr, x, weights, kernel_points, kp_extent, influence, aggregation, impl)
        ctx.args = (float(kp_extent), int(influence), int(aggregation))
        ctx.save_for_backward(q_pts, s_pts, nbr, x, weights, kernel_points)
        return y

    @staticmethod
    def backward(ctx, dout):
        from .autograd import KP_WF_BOUND_MAX_ROW, _tn_product, bgemm
        q_pts, s_pts, nbr, x, w, kp = ctx.saved_tensors
        kp_extent, influence, aggregation = ctx.args
        dout = dout.contiguous()
        nq = q_pts.shape[0]
        n_kp, cin, cout = w.shape
        nbr32, _ = _index_rows(nbr)
        kmax = nbr32.shape[1]
        xd = x.detach().contiguous()
        kpd = kp.detach().contiguous()
        wf, cnt = weighted_features(q_pts, s_pts, nbr32, xd, kpd, kp_extent, influence, aggregation)
        g = (dout / cnt.unsqueeze(1)).contiguous()
        # |wf| <= kmax max|x| in every mode (every influence is <= 1): the bound KPConvFn hands to the products
        xr, xr_n = ops._get_range(x)
        if xr is not None and kmax <= KP_WF_BOUND_MAX_ROW:
            ops._set_range(wf, xr[:xr_n] * float(kmax), int(xr_n))
        wflat = w.detach().contiguous().view(n_kp * cin, cout)
        dx = dw = None
        if ctx.needs_input_grad[3]:
            if ops._modes["gemm"] == 1 and cout % 32 == 0:
                ops.ensure_range(g)
                dwf = ops.linear_raw(g, wflat)
            else:
                dwf = torch.empty((nq, n_kp * cin), dtype=torch.float32, device=x.device)
                bgemm(g, wflat, dwf, [(0, 0, 0, nq, n_kp * cin, cout)], (cout, 1), (1, cout), (n_kp * cin, 1))
            dx = bwd_dx(q_pts, s_pts, nbr32, cin, kpd, kp_extent, influence, aggregation, dwf)
        if ctx.needs_input_grad[4]:
            dw = _tn_product(wf, g, nq, n_kp * cin, cout, f64=(cin == 1)).view(n_kp, cin, cout)
        return None, None, None, dx, dw, None, None, None, None, None
