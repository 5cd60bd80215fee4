"""The regulariser of deformable KPConv (csrc/deform_reg.hip): KPConv's fitting loss -- the squared distance from every
deformed kernel point to its nearest input point -- and repulsive loss -- a query's kernel points may not collapse onto
each other -- with their gradient at the offset features, in one launch.  Opt-in: cfg.deform_fitting_power > 0.

    deform_reg(...)                   (value, fit, rep) of one block: value = 2 fit + rep on the tape w.r.t. the offset
                                      features (DeformRegFn), fit and rep detached
    deform_reg_raw(...)               the plain launch: out [3] and, when asked for, d offset_features
    regularizer_terms(module, ...)    (power * sum value, sum fit, sum rep) over the KPConvDeformable blocks under a module
    p2p_fitting_regularizer(...)      the first of those: what joins the loss

The contract, and where it leaves KPConv's authors (a shadow entry never takes part in the minimum), is include/spr.h's.
A subpackage: the top-level modules import it lazily and never name its entry points.
"""
import torch

from .. import _lib, ops
from ..kpconv_modes import _index_rows


def _modulated(offset_features, n_kp: int) -> bool:
    cols = offset_features.shape[1]
    if cols not in (3 * n_kp, 4 * n_kp):
        raise ValueError(f"offset features of {cols} columns for {n_kp} kernel points (3 K, or 4 K when modulated)")
    return cols == 4 * n_kp


def deform_reg_raw(q_pts, s_pts, nbr, offset_features, kernel_points, kp_extent: float, repulse_extent: float = 1.2,
                   want_grad: bool = False):
    """(out [3] = (2 fit + rep, fit, rep), d offset_features [nq, 3 K (+ K)] or None).  Without want_grad the launch
    stores nothing but its partial sums."""
    q_pts = ops._dev(q_pts, "q_pts", torch.float32)
    s_pts = ops._dev(s_pts, "s_pts", torch.float32)
    kernel_points = ops._dev(kernel_points, "kernel_points", torch.float32)
    nbr, stride = _index_rows(nbr)
    nq, ns, kmax = q_pts.shape[0], s_pts.shape[0], nbr.shape[1]
    n_kp = kernel_points.shape[0]
    modulated = _modulated(offset_features, n_kp)
    of = offset_features.detach()
    if of.dtype != torch.float32 or of.stride(1) != 1:
        of = of.float().contiguous()
    assert of.shape[0] == nq, (of.shape, nq)
    L = _lib.lib()
    ws = ops._workspace(L.spr_deform_reg_workspace_size(nq), of.device)
    out = torch.empty((3,), dtype=torch.float32, device=of.device)
    d_of = torch.empty((nq, of.shape[1]), dtype=torch.float32, device=of.device) if want_grad else None
    _lib.check(L.spr_deform_reg(ops._ptr(q_pts), nq, ops._ptr(s_pts), ns, ops._ptr(nbr), int(stride), kmax,
                                ops._ptr(kernel_points), n_kp, float(kp_extent), ops._ptr(of), int(of.stride(0)),
                                int(modulated), float(repulse_extent), ops._ptr(out), ops._ptr(d_of), ops._ptr(ws),
                                ws.numel(), ops._stream(of)), "spr_deform_reg")
    return out, d_of


class DeformRegFn(torch.autograd.Function):
    """spr_deform_reg with the gradient: the forward's launch leaves d offset_features, the backward scales it.  fit and
    rep are for logging: not differentiable.  No gradient reaches the points or the kernel points."""

    @staticmethod
    def forward(ctx, q_pts, s_pts, nbr, offset_features, kernel_points, kp_extent, repulse_extent):
        out, d_of = deform_reg_raw(q_pts, s_pts, nbr, offset_features, kernel_points, kp_extent, repulse_extent,
                                   want_grad=True)
        ctx.save_for_backward(d_of)
        value, fit, rep = out.unbind(0)
        ctx.mark_non_differentiable(fit, rep)
        return value, fit, rep

    @staticmethod
    def backward(ctx, d_value, _d_fit, _d_rep):
        d_of, = ctx.saved_tensors
        return None, None, None, d_of * d_value, None, None, None


def deform_reg(q_pts, s_pts, nbr, offset_features, kernel_points, kp_extent: float, repulse_extent: float = 1.2):
    """(value, fit, rep), three 0-d float32 tensors: value = 2 fit + rep, on the tape with respect to offset_features
    [nq, 3 K (+ K when modulated)] when they want a gradient; fit and rep detached.  nbr may be int32 or int64
    [nq, kmax] (possibly a column slice)."""
    if ops._wants_grad(offset_features):
        return DeformRegFn.apply(q_pts, s_pts, nbr, offset_features, kernel_points.detach(), float(kp_extent),
                                 float(repulse_extent))
    out, _ = deform_reg_raw(q_pts, s_pts, nbr, offset_features, kernel_points.detach(), kp_extent, repulse_extent)
    return tuple(out.unbind(0))


def regularizer_terms(module, power: float, repulse_extent: float = 1.2):
    """(power * sum of value, sum of fit, sum of rep) over every KPConvDeformable under `module`, each from its last
    forward (the block keeps its points and rows when its keep_reg_inputs is set); None when no block has one."""
    from ..deformable import KPConvDeformable
    total = fit = rep = None
    for m in module.modules():
        if not isinstance(m, KPConvDeformable) or m.offset_features is None or m.reg_inputs is None:
            continue
        q_pts, s_pts, nbr = m.reg_inputs
        v, f, r = deform_reg(q_pts, s_pts, nbr, m.offset_features, m.kernel_points, m.KP_extent, repulse_extent)
        total, fit, rep = (v, f, r) if total is None else (total + v, fit + f, rep + r)
    if total is None:
        return None
    return power * total, fit, rep


def p2p_fitting_regularizer(module, power: float, repulse_extent: float = 1.2):
    """power * sum of deform_reg's value over the KPConvDeformable blocks under `module` (KPConv's
    p2p_fitting_regularizer with deform_fitting_power and repulse_extent); None when there is no block with a forward."""
    terms = regularizer_terms(module, power, repulse_extent)
    return None if terms is None else terms[0]
