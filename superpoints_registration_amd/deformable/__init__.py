"""Deformable / modulated KPConv, linear influence and sum aggregation (csrc/kpconv_deform.hip): the reference's
KPConv.forward with deformable=True (kpconv_blocks.py:309-412).  Opt-in: block_decider builds the `*_deformable*` blocks
only under config.deformable_kpconv, and no shipped config sets it.

    kpconv_deform(...)       forward, differentiable in x, weights and offset_features (KPConvDeformFn)
    kpconv_deform_raw(...)   the plain launch (spr_kpconv_deform_fwd), optionally with min_d2
    KPConvDeformable         the module: a rigid offset convolution (its own kernel points) + bias -> kpconv_deform

A subpackage: the top-level modules import it lazily and never name its entry points.
"""
import math

import torch
import torch.nn as nn
from torch.nn.parameter import Parameter

from .. import _lib, ops
from ..kernel_points import load_kernels
from ..kpconv_modes import _index_rows


def offset_dim(n_kp: int, modulated: bool, p_dim: int = 3) -> int:
    return (p_dim + 1) * n_kp if modulated else p_dim * n_kp


def _offsets(offset_features, nq: int, n_kp: int, modulated: bool):
    """float32 offset features [nq, offset_dim] with unit column stride (possibly a column slice), and their row stride."""
    of = offset_features
    if of.dtype != torch.float32 or of.stride(1) != 1:
        of = of.float().contiguous()
    assert of.shape == (nq, offset_dim(n_kp, modulated)), (of.shape, nq, n_kp, modulated)
    return of, of.stride(0)


def kpconv_deform(q_pts, s_pts, nbr, x, weights, kernel_points, kp_extent: float, offset_features, modulated: bool,
                  impl: int = 0, want_min_d2: bool = False):
    """out [nq, cout]; with want_min_d2 (out, min_d2 [nq, K]).  nbr may be int32 or int64 [nq, kmax] (possibly a column
    slice); offset_features [nq, 3 K (+ K when modulated)] is the offset convolution's output plus bias."""
    if ops._wants_grad(x, weights, offset_features):
        out, min_d2 = KPConvDeformFn.apply(ops._dev(q_pts, "q_pts", torch.float32),
                                           ops._dev(s_pts, "s_pts", torch.float32), nbr,
                                           ops._dev(x, "x", torch.float32), weights, kernel_points, float(kp_extent),
                                           ops._dev(offset_features, "offset_features", torch.float32), bool(modulated),
                                           int(impl))
        return (out, min_d2) if want_min_d2 else out
    return kpconv_deform_raw(q_pts, s_pts, nbr, x, weights, kernel_points, kp_extent, offset_features, modulated, impl,
                             want_min_d2)


def kpconv_deform_raw(q_pts, s_pts, nbr, x, weights, kernel_points, kp_extent: float, offset_features,
                      modulated: bool, impl: int = 0, want_min_d2: bool = False):
    """The forward launch; with want_min_d2 returns (out, min_d2 [nq, K])."""
    q_pts = ops._dev(q_pts, "q_pts", torch.float32)
    s_pts = ops._dev(s_pts, "s_pts", torch.float32)
    x = ops._dev(x, "x", torch.float32)
    weights = ops._dev(weights, "weights", torch.float32)
    kernel_points = ops._dev(kernel_points, "kernel_points", torch.float32)
    nbr, stride = _index_rows(nbr)
    nq, ns, kmax = q_pts.shape[0], s_pts.shape[0], nbr.shape[1]
    n_kp, cin, cout = weights.shape
    assert x.shape == (ns, cin), (x.shape, ns, cin)
    of, of_stride = _offsets(offset_features, nq, n_kp, modulated)
    L = _lib.lib()
    ws = ops._workspace(L.spr_kpconv_deform_workspace_size(nq, ns, cin, cout), x.device)
    out = torch.empty((nq, cout), dtype=torch.float32, device=x.device)
    min_d2 = torch.empty((nq, n_kp), dtype=torch.float32, device=x.device) if want_min_d2 else None
    xr, xr_n = ops._get_range(x)
    wr, wr_n = ops._static_range(weights)
    wplanes = None
    if impl == 0 and n_kp == 15 and cin % 32 == 0 and cout % 32 == 0 and cout <= 256 and wr is not None:
        wplanes = ops._kpconv_wplanes(weights, wr, wr_n)      # the planes (and their cache) of ops.kpconv
    _lib.check(L.spr_kpconv_deform_fwd(ops._ptr(q_pts), nq, ops._ptr(s_pts), ns, ops._ptr(nbr), int(stride), kmax,
                                       ops._ptr(x), cin, ops._ptr(weights), cout, ops._ptr(kernel_points), n_kp,
                                       float(kp_extent), ops._ptr(of), int(of_stride), int(bool(modulated)),
                                       ops._ptr(out), ops._ptr(min_d2), int(impl), ops._ptr(xr), int(xr_n),
                                       ops._ptr(wr), int(wr_n), ops._ptr(wplanes), ops._ptr(ws), ws.numel(),
                                       ops._stream(x)), "spr_kpconv_deform_fwd")
    return (out, min_d2) if want_min_d2 else out


def weighted_features(q_pts, s_pts, nbr, x, kernel_points, kp_extent: float, offset_features):
    """wf [nq, n_kp * cin] (unmodulated, un-normalised) and cnt [nq] = max(1, in-range neighbour count)."""
    nbr, stride = _index_rows(nbr)
    nq, ns, kmax = q_pts.shape[0], s_pts.shape[0], nbr.shape[1]
    n_kp, cin = kernel_points.shape[0], x.shape[1]
    of, of_stride = _offsets(offset_features[:, :3 * n_kp], nq, n_kp, False)       # the modulation columns are not read
    L = _lib.lib()
    wf = torch.empty((nq, n_kp * cin), dtype=torch.float32, device=x.device)
    cnt = torch.empty((nq,), dtype=torch.float32, device=x.device)
    ws = ops._workspace(L.spr_kpconv_deform_weighted_features_workspace_size(ns), x.device)
    _lib.check(L.spr_kpconv_deform_weighted_features(ops._ptr(q_pts), nq, ops._ptr(s_pts), ns, ops._ptr(nbr),
                                                     int(stride), kmax, ops._ptr(x), cin, ops._ptr(kernel_points),
                                                     n_kp, float(kp_extent), ops._ptr(of), int(of_stride),
                                                     ops._ptr(wf), ops._ptr(cnt), ops._ptr(ws), ws.numel(),
                                                     ops._stream(x)), "spr_kpconv_deform_weighted_features")
    return wf, cnt


def bwd_dx(q_pts, s_pts, nbr, cin: int, kernel_points, kp_extent: float, offset_features, modulated: bool, dwfm):
    """dx [ns, cin] = scatter of influence x modulation x dwfm (order-independent sums); dwfm's published range is used
    if it has one."""
    nbr, stride = _index_rows(nbr)
    nq, ns, kmax = q_pts.shape[0], s_pts.shape[0], nbr.shape[1]
    n_kp = kernel_points.shape[0]
    of, of_stride = _offsets(offset_features, nq, n_kp, modulated)
    L = _lib.lib()
    dx = torch.empty((ns, cin), dtype=torch.float32, device=dwfm.device)
    ws = ops._workspace(L.spr_scatter_workspace_bytes(ns, cin), dwfm.device)
    dr, dr_n = ops._get_range(dwfm)
    _lib.check(L.spr_kpconv_deform_bwd_dx(ops._ptr(q_pts), nq, ops._ptr(s_pts), ns, ops._ptr(nbr), int(stride), kmax,
                                          cin, ops._ptr(kernel_points), n_kp, float(kp_extent), ops._ptr(of),
                                          int(of_stride), int(bool(modulated)), ops._ptr(dwfm), ops._ptr(dr), int(dr_n),
                                          ops._ptr(dx), ops._ptr(ws), ws.numel(), ops._stream(dwfm)),
               "spr_kpconv_deform_bwd_dx")
    return dx


def bwd_offsets(q_pts, s_pts, nbr, x, kernel_points, kp_extent: float, offset_features, modulated: bool, dwfm):
    """d offset_features [nq, 3 K (+ K)], every element written, sums in a fixed order."""
    nbr, stride = _index_rows(nbr)
    nq, ns, kmax = q_pts.shape[0], s_pts.shape[0], nbr.shape[1]
    n_kp, cin = kernel_points.shape[0], x.shape[1]
    of, of_stride = _offsets(offset_features, nq, n_kp, modulated)
    d_of = torch.empty((nq, offset_dim(n_kp, modulated)), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().spr_kpconv_deform_bwd_offsets(ops._ptr(q_pts), nq, ops._ptr(s_pts), ns, ops._ptr(nbr),
                                                        int(stride), kmax, ops._ptr(x), cin, ops._ptr(kernel_points),
                                                        n_kp, float(kp_extent), ops._ptr(of), int(of_stride),
                                                        int(bool(modulated)), ops._ptr(dwfm), ops._ptr(d_of),
                                                        ops._stream(x)), "spr_kpconv_deform_bwd_offsets")
    return d_of


class KPConvDeformFn(torch.autograd.Function):
    """spr_kpconv_deform_fwd -> (out, min_d2), min_d2 not differentiable (the reference has no loss on it); backward with KPConvModesFn's factorisation, the modulation and the offsets added:
       g = dout / count;  dWFm = g W_flat^T;  dW_flat = (m wf)^T g;  dx = scatter(h m dWFm);
       d offset_features from dWFm, x and the geometry (spr_kpconv_deform_bwd_offsets)."""

    @staticmethod
    def forward(ctx, q_pts, s_pts, nbr, x, weights, kernel_points, kp_extent, offset_features, modulated, impl):
        with torch.no_grad():
            y, min_d2 = kpconv_deform_raw(q_pts, s_pts, nbr, x, weights, kernel_points, kp_extent, offset_features,
                                          modulated, impl, want_min_d2=True)
        ctx.args = (float(kp_extent), bool(modulated))
        ctx.save_for_backward(q_pts, s_pts, nbr, x, weights, kernel_points, offset_features)
        ctx.mark_non_differentiable(min_d2)
        return y, min_d2

    @staticmethod
    def backward(ctx, dout, _d_min_d2):
        from ..autograd import KP_WF_BOUND_MAX_ROW, _tn_product, bgemm
        q_pts, s_pts, nbr, x, w, kp, of = ctx.saved_tensors
        kp_extent, modulated = ctx.args
        dout = dout.contiguous()
        nq = q_pts.shape[0]
        n_kp, cin, cout = w.shape
        nbr32, _ = _index_rows(nbr)
        kmax = nbr32.shape[1]
        xd = x.detach().contiguous()
        kpd = kp.detach().contiguous()
        ofd = of.detach()
        wf, cnt = weighted_features(q_pts, s_pts, nbr32, xd, kpd, kp_extent, ofd)
        g = (dout / cnt.unsqueeze(1)).contiguous()
        wflat = w.detach().contiguous().view(n_kp * cin, cout)
        dx = dw = d_of = None
        if ctx.needs_input_grad[3] or ctx.needs_input_grad[7]:
            if ops._modes["gemm"] == 1 and cout % 32 == 0:
                ops.ensure_range(g)
                dwfm = ops.linear_raw(g, wflat)
            else:
                dwfm = torch.empty((nq, n_kp * cin), dtype=torch.float32, device=x.device)
                bgemm(g, wflat, dwfm, [(0, 0, 0, nq, n_kp * cin, cout)], (cout, 1), (1, cout), (n_kp * cin, 1))
            if ctx.needs_input_grad[3]:
                dx = bwd_dx(q_pts, s_pts, nbr32, cin, kpd, kp_extent, ofd, modulated, dwfm)
            if ctx.needs_input_grad[7]:
                d_of = bwd_offsets(q_pts, s_pts, nbr32, xd, kpd, kp_extent, ofd, modulated, dwfm)
        if ctx.needs_input_grad[4]:
            bound = float(kmax)
            if modulated:   # wf <- m wf, m = 2 sigmoid < 2
                m = 2.0 * torch.sigmoid(ofd[:, 3 * n_kp:4 * n_kp])
                wf = (wf.view(nq, n_kp, cin) * m.unsqueeze(2)).view(nq, n_kp * cin)
                bound *= 2.0
            # |wf| <= (2) kmax max|x| (every influence is <= 1): the bound KPConvFn hands to the products
            xr, xr_n = ops._get_range(x)
            if xr is not None and kmax <= KP_WF_BOUND_MAX_ROW:
                ops._set_range(wf, xr[:xr_n] * bound, int(xr_n))
            dw = _tn_product(wf, g, nq, n_kp * cin, cout, f64=(cin == 1)).view(n_kp, cin, cout)
        return None, None, None, dx, dw, None, None, d_of, None, None


class KPConvDeformable(nn.Module):
    """The reference's KPConv class with deformable=True (kpconv_blocks.py:175-420): constructor signature, attributes
    and state-dict names (weights, kernel_points, offset_conv.weights, offset_conv.kernel_points, offset_bias).  After a
    forward the module holds offset_features, deformed_KP [nq, K, 3] and min_d2 [nq, K], as the reference's does.
    Only KP_influence 'linear' with aggregation_mode 'sum'.

    The offset convolution's width (3 K or 4 K: 45 or 60 columns) is no multiple of 32, so the rigid kernels would take
    their one-thread-per-output route: measured at 140 x the time of the same convolution on weights zero-padded to 64
    columns (profiles/deform_bench.txt).  So it runs padded, and the first offset_dim columns are kept: the padded
    copy is cached per weight version in inference and built on the tape in training (the slice is on the tape either
    way)."""

    def __init__(self, kernel_size, p_dim, in_channels, out_channels, KP_extent, radius, fixed_kernel_points='center',
                 KP_influence='linear', aggregation_mode='sum', deformable=True, modulated=False):
        super().__init__()
        from ..kpconv_blocks import KPConv
        from ..kpconv_modes import is_default_mode, mode_codes
        if not deformable:
            raise ValueError("KPConvDeformable is the deformable KPConv; kpconv_blocks.KPConv is the rigid one")
        mode_codes(KP_influence, aggregation_mode)                  # ValueError for an unknown string
        if not is_default_mode(KP_influence, aggregation_mode):
            raise NotImplementedError(f"deformable KPConv with KP_influence={KP_influence!r}, "
                                      f"aggregation_mode={aggregation_mode!r}: only 'linear' / 'sum' is built")
        if p_dim != 3:
            raise NotImplementedError(f"deformable KPConv in {p_dim} dimensions")
        self.K = kernel_size
        self.p_dim = p_dim
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.radius = radius
        self.KP_extent = KP_extent
        self.fixed_kernel_points = fixed_kernel_points
        self.KP_influence = KP_influence
        self.aggregation_mode = aggregation_mode
        self.deformable = True
        self.modulated = modulated
        self.rows_sorted = False
        self.impl = 0
        self.min_d2 = None
        self.deformed_KP = None
        self.offset_features = None
        # set (by the encoder, under cfg.deform_fitting_power > 0): forward() keeps references to its points and rows
        # for the regulariser (the deform_reg subpackage); off, the module holds nothing more than the three above
        self.keep_reg_inputs = False
        self.reg_inputs = None

        self.weights = Parameter(torch.zeros((self.K, in_channels, out_channels), dtype=torch.float32),
                                 requires_grad=True)
        self.offset_dim = offset_dim(self.K, modulated, p_dim)
        self.offset_conv = KPConv(self.K, p_dim, in_channels, self.offset_dim, KP_extent, radius,
                                  fixed_kernel_points=fixed_kernel_points, KP_influence=KP_influence,
                                  aggregation_mode=aggregation_mode)
        self.offset_bias = Parameter(torch.zeros(self.offset_dim, dtype=torch.float32), requires_grad=True)
        self.reset_parameters()
        self.kernel_points = self.init_KP()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weights, a=math.sqrt(5))
        nn.init.zeros_(self.offset_bias)

    def init_KP(self):
        K_points_numpy = load_kernels(self.radius, self.K, dimension=self.p_dim, fixed=self.fixed_kernel_points)
        return Parameter(torch.tensor(K_points_numpy, dtype=torch.float32), requires_grad=False)

    def _offset_conv(self, q_pts, s_pts, neighb_inds, x):
        conv = self.offset_conv
        conv.rows_sorted = self.rows_sorted
        w = conv.weights
        pad = -self.offset_dim % 32
        if pad == 0 or self.in_channels % 32 != 0 or not w.is_cuda:      # no tile shape to pad to
            return conv(q_pts, s_pts, neighb_inds, x)
        if ops._wants_grad(x, w):
            wp = nn.functional.pad(w, (0, pad))
        else:
            def build():
                padded = nn.functional.pad(w.detach(), (0, pad)).contiguous()
                return padded, padded
            wp = ops._derived(w, '_spr_deform_offset_pad', pad, build)
        out = ops.kpconv(q_pts, s_pts, neighb_inds, x, wp, conv.kernel_points.detach(), conv.KP_extent,
                         rows_sorted=conv.rows_sorted, impl=conv.impl)
        return out[:, :self.offset_dim]

    def forward(self, q_pts, s_pts, neighb_inds, x):
        self.offset_features = self._offset_conv(q_pts, s_pts, neighb_inds, x) + self.offset_bias
        self.reg_inputs = (q_pts, s_pts, neighb_inds) if self.keep_reg_inputs else None
        kp = self.kernel_points.detach()
        out, self.min_d2 = kpconv_deform(q_pts, s_pts, neighb_inds, x, self.weights, kp, self.KP_extent,
                                         self.offset_features, self.modulated, impl=self.impl, want_min_d2=True)
        with torch.no_grad():
            off = self.offset_features[:, :self.p_dim * self.K].view(-1, self.K, self.p_dim)
            self.deformed_KP = off * self.KP_extent + kp
        return out

    def __repr__(self):
        return 'KPConvDeformable(radius: {:.2f}, extent: {:.2f}, in_feat: {:d}, out_feat: {:d}, modulated: {:s})'.format(
            self.radius, self.KP_extent, self.in_channels, self.out_channels, str(self.modulated))
