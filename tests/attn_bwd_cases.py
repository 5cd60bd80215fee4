"""CPU only: inputs and float64 references for the attention backward (csrc/attention_bwd.hip), shared by
tests/test_attn_bwd_cases_host.py (which holds the references against each other) and tests/test_gpu_attn_bwd_routes.py.

  edge_case()        segment lengths around every multiple of 32 and 64, as query AND as key length
  recentring_case()  keys placed so that the forward's key loop moves its reference exponent (attention.hip, `redo`)
                     before it writes the log-sum-exp the backward is handed
  autograd_f64()     O, L and the three gradients by torch autograd in float64
  replica_f64()      the backward's documented formulas in float64 with O and L as INPUTS: the reference for a backward
                     that is handed another kernel's O and L
  recentre_counts()  a float64 model of how often the forward recentres per (query, head) row
  MinBwdLib          the library with the backward's workspace query answering the minimum (the route without planes)
"""
import math

import numpy as np
import torch

from superpoints_registration_amd import synthetic

NHEAD, HD = 8, 32
D = NHEAD * HD
LN2 = math.log(2.0)

# 1 to 4 tiles of 64 per side (both parities of mode 0's double buffer), every boundary of the 32 x 32 wave blocks
LENS = [1, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 193]
KV_SEGS = (list(range(len(LENS))), list(range(len(LENS)))[::-1])      # short queries meet long keys and the reverse

PATTERNS = ("spike_late", "two_steps", "huge_first")
RC_LENS, RC_KV_SEG, RC_SEED = [193, 129], [1, 0], 5


def edge_case(seed=9, seed_do=11):
    """(q, k, v, dO, LENS): float32, q / k / v column slices of one [T, 768] tensor (row stride 768)."""
    tot = sum(LENS)
    qkv = synthetic.rand((tot, 3 * D), seed, -1.5, 1.5)
    return qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], synthetic.rand((tot, D), seed_do), list(LENS)


def recentring_case(pattern, seed=RC_SEED):
    """(q, k, v, dO, lens, kv_seg).  Queries lean on a fixed unit vector u per head, ordinary keys are small, and a few
    hot keys lean on u too: a hot key's base-2 score stands ~14 (beta 5.66) or ~28 (beta 11.32) above the rest.  Hot keys
    come in pairs: one dominant key would make dS ~ 0 and the float32 gradients ill-conditioned."""
    assert pattern in PATTERNS, pattern
    g = torch.Generator().manual_seed(int(seed))
    tot = sum(RC_LENS)
    u = torch.randn((NHEAD, HD), generator=g)
    u = (u / u.norm(dim=1, keepdim=True)).reshape(1, D)
    q = torch.randn((tot, D), generator=g) + 9.7 * u
    k = 0.09 * torch.randn((tot, D), generator=g)
    v = torch.randn((tot, D), generator=g)
    go = torch.randn((tot, D), generator=g)
    beg = 0
    for n in RC_LENS:
        hot = {"spike_late": [(n - 20, 5.66), (n - 7, 5.66)],
               "two_steps": [(70, 5.66), (n - 2, 11.32), (n - 1, 11.32)],
               "huge_first": [(3, 5.66), (40, 5.66)]}[pattern]
        for row, beta in hot:
            k[beg + row] = beta * u[0] + 1.5 * torch.randn(D, generator=g)
        beg += n
    return q, k, v, go, list(RC_LENS), list(RC_KV_SEG)


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _heads(x):
    return x.view(-1, NHEAD, HD).transpose(0, 1)          # [head, rows, 32]


def _rows(x):
    return x.transpose(0, 1).reshape(-1, D)               # back to [rows, 256]


def _autograd(q0, k0, v0, go, lens, kv_seg, dtype):
    cq, ck, cv = (t.detach().to(dtype).clone().requires_grad_(True) for t in (q0, k0, v0))
    offs = _offsets(lens)
    outs, lses = [], []
    for s in range(len(lens)):
        ks = kv_seg[s]
        q, k, v = _heads(cq[offs[s]:offs[s + 1]]), _heads(ck[offs[ks]:offs[ks + 1]]), _heads(cv[offs[ks]:offs[ks + 1]])
        sc = q @ k.transpose(1, 2) / math.sqrt(HD)
        outs.append(_rows(torch.softmax(sc, -1) @ v))
        lses.append((torch.logsumexp(sc.detach(), -1) / LN2).transpose(0, 1))
    out = torch.cat(outs)
    out.backward(go.to(dtype))
    return out.detach(), torch.cat(lses), cq.grad, ck.grad, cv.grad


def autograd_f64(q, k, v, go, lens, kv_seg):
    """float64 (O [T, 256], L [T, 8], dq, dk, dv) by torch autograd; L = logsumexp(scores) / ln 2, the base-2
    log-sum-exp the forward hands to the backward."""
    return _autograd(q, k, v, go, lens, kv_seg, torch.float64)


def attention_grads_f64(q, k, v, go, lens, kv_seg):
    """The three float64 gradients alone."""
    return autograd_f64(q, k, v, go, lens, kv_seg)[2:]


def autograd_f32(q, k, v, go, lens, kv_seg):
    """The same graph in float32 on the CPU, returned as float64: what plain float32 arithmetic makes of the data."""
    return tuple(t.double() for t in _autograd(q, k, v, go, lens, kv_seg, torch.float32))


def replica_f64(q, k, v, out, lse, go, lens, kv_seg):
    """float64 (dq, dk, dv) by the formulas in the header of attention_bwd.hip, O and L given:
         D = rowsum(dO o O), P = exp2(c S - L), dV = P^T dO, dP = dO V^T, dS = P o (dP - D),
         dQ = scale dS K, dK = scale dS^T Q,                     c = log2(e) / sqrt(32), scale = 1 / sqrt(32)."""
    q, k, v, out, lse, go = (t.detach().double().cpu() for t in (q, k, v, out, lse, go))
    scale = 1.0 / math.sqrt(HD)
    c = scale / LN2
    offs = _offsets(lens)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(q)
    for s in range(len(lens)):
        ks = kv_seg[s]
        qs, kk = slice(offs[s], offs[s + 1]), slice(offs[ks], offs[ks + 1])
        qh, kh, vh, oh, gh = _heads(q[qs]), _heads(k[kk]), _heads(v[kk]), _heads(out[qs]), _heads(go[qs])
        dsum = (gh * oh).sum(-1, keepdim=True)                                     # [head, Lq, 1]
        p = torch.exp2(c * (qh @ kh.transpose(1, 2)) - lse[qs].transpose(0, 1).unsqueeze(-1))
        ds = p * (gh @ vh.transpose(1, 2) - dsum)
        dv[kk] = _rows(p.transpose(1, 2) @ gh)
        dq[qs] = _rows(scale * (ds @ kh))
        dk[kk] = _rows(scale * (ds.transpose(1, 2) @ qh))
    return dq, dk, dv


def recentre_counts(q, k, lens, kv_seg, tile=64, jump=11.0):
    """How often the forward's key loop recentres per (query, head) row, modelled in float64: the reference is the
    largest base-2 score over keys 0 .. tile - 1; a later tile whose largest score exceeds the running reference by
    >= jump (2^(4 + 11) = 2^15: a probability about to leave fp16's range) moves the reference to that maximum.
    Returns an int64 [T, 8] array."""
    q, k = q.double(), k.double()
    c = 1.0 / (math.sqrt(HD) * LN2)
    offs = _offsets(lens)
    counts = np.zeros((sum(lens), NHEAD), np.int64)
    for s in range(len(lens)):
        ks = kv_seg[s]
        sc = c * (_heads(q[offs[s]:offs[s + 1]]) @ _heads(k[offs[ks]:offs[ks + 1]]).transpose(1, 2))   # [head, Lq, Lk]
        ref = sc[:, :, :tile].max(-1).values
        n = torch.zeros_like(ref, dtype=torch.int64)
        for t0 in range(tile, sc.shape[2], tile):
            mx = sc[:, :, t0:t0 + tile].max(-1).values
            move = mx - ref >= jump
            ref = torch.where(move, mx, ref)
            n += move.to(torch.int64)
        counts[offs[s]:offs[s + 1]] = n.transpose(0, 1).numpy()
    return counts


def grad_errors(got, ref):
    """Per gradient (error, scale): the largest absolute error and the float64 gradient's largest entry."""
    out = []
    for a, r in zip(got, ref):
        a, r = a.detach().double().cpu(), r.detach().double().cpu()
        out.append((float((a - r).abs().max()), float(r.abs().max())))
    return out


def check_grads(got, ref, rel, what, floor=None):
    """The project's attention-gradient criterion: every gradient within rel of the float64 gradient's largest entry;
    where the float64 gradient is exactly zero (dq, dk with one key per query) within rel of the largest entry of the
    three gradients together.  floor: per-gradient absolute allowances that may raise the bound (4 x the float32 CPU
    error on ill-scaled data).  Prints every figure before it asserts; returns the relative errors."""
    errs = grad_errors(got, ref)
    joint = max(s for _, s in errs)
    rows = []
    for i, ((err, scale), nm) in enumerate(zip(errs, "qkv")):
        base = scale if scale > 0.0 else joint
        bound = rel * base if floor is None else max(rel * base, floor[i])
        rows.append((nm, err, base, bound))
        print(f"{what} d{nm}: max err {err:.3e}, scale {base:.3e}, rel {err / base:.3e} (bound {bound / base:.3e})")
    for nm, err, base, bound in rows:
        assert math.isfinite(err) and err <= bound, f"{what} d{nm}: {err:.3e} > {bound:.3e} (scale {base:.3e})"
    return [err / base for _, err, base, _ in rows]


class MinBwdLib:
    """The library with spr_attn_bwd_workspace_bytes answering the minimum: the route without operand planes.  The
    entry point takes that route only when the workspace it is GIVEN has no room for the planes, so the caller must
    also hand over exactly the bytes asked for (exact_workspace), not the grow-only buffer of ops._workspace."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name == "spr_attn_bwd_workspace_bytes":
            return lambda t, nseg, nhead: self._lib.spr_attn_bwd_min_workspace_bytes(t, nhead)
        return getattr(self._lib, name)


def exact_workspace(nbytes, device):
    """A stand-in for ops._workspace that hands out exactly the bytes asked for."""
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
