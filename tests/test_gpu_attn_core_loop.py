"""GPU: the key loop of the attention core k_attn_s (csrc/attention.hip) -- tile fetch with scalar addressing, the
full-tile loop unrolled by two with a static buffer index, the peeled clamped fetch of the tail tile, and waves
without a query -- against float64, on the smallest segment lengths that reach every branch:

  key loop    0 .. 5 full tiles (both parities of the pair loop), with and without a tail tile, a clamped fetch right
              after the first tile (65, 129, 193, 257), a one-key segment;
  query loop  last workgroups with 1, 2 and 3 empty waves (129 and 257; 161, 33 and 65; 97 and 193), and none (128, 320).

kv_seg = identity (self) and the reversed list (cross): every query length meets short and long key lengths."""
import math

import numpy as np
import pytest
import torch

from superpoints_registration_amd import ops, synthetic
from superpoints_registration_amd.transformers import (TransformerCrossEncoder, TransformerCrossEncoderLayer,
                                                       make_segments)

pytestmark = pytest.mark.gpu

LENS = [1, 33, 64, 65, 97, 128, 129, 161, 192, 193, 257, 320]
KV_SEGS = (list(range(len(LENS))), list(range(len(LENS)))[::-1])
# relative to the output scale, per attention mode (tests/test_gpu_ops.py, tests/test_gpu_range.py)
BOUND = {0: 3e-6, 1: 3e-6, 4: 3e-5, 3: 3e-4, 2: 2e-3}


def _close(got, ref, rel, what=""):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref).max()
    scale = max(np.abs(ref).max(), 1e-30)
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}, rel {err / scale:.3e} (bound {rel})")
    assert err <= rel * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.3e} > {rel})"


@pytest.fixture(scope="module")
def case():
    """Inputs and the float64 references (output and base-2 log-sum-exp of the scaled scores), computed once."""
    tot = sum(LENS)
    qkv = synthetic.rand((tot, 768), 9, -2, 2)
    offs = np.concatenate([[0], np.cumsum(LENS)])
    refs = []
    for kv_seg in KV_SEGS:
        out = torch.zeros((tot, 256), dtype=torch.float64)
        lse = torch.zeros((tot, 8), dtype=torch.float64)
        for s, ks in enumerate(kv_seg):
            q = qkv[offs[s]:offs[s + 1], :256].double().view(-1, 8, 32).transpose(0, 1)
            k = qkv[offs[ks]:offs[ks + 1], 256:512].double().view(-1, 8, 32).transpose(0, 1)
            v = qkv[offs[ks]:offs[ks + 1], 512:].double().view(-1, 8, 32).transpose(0, 1)
            sc = q @ k.transpose(1, 2) / math.sqrt(32)
            out[offs[s]:offs[s + 1]] = (torch.softmax(sc, -1) @ v).transpose(0, 1).reshape(-1, 256)
            lse[offs[s]:offs[s + 1]] = (torch.logsumexp(sc, -1) / math.log(2.0)).transpose(0, 1)
        refs.append((out.numpy(), lse.numpy()))
    return qkv, refs


@pytest.mark.parametrize("mode", [4, 1, 2, 3, 0])
def test_core_vs_fp64(device, case, mode):
    qkv, refs = case
    d = qkv.to(device)
    cu = ops.lengths_to_cu(LENS, device)
    ops.set_attn_mode(mode)
    try:
        for kv_seg, (ref, _) in zip(KV_SEGS, refs):
            seg = torch.tensor(kv_seg, dtype=torch.int32, device=device)
            o = ops.attention(d[:, :256], d[:, 256:512], d[:, 512:], cu, seg, max(LENS), 8)
            _close(o.cpu().numpy(), ref, BOUND[mode], f"attention mode={mode} kv_seg[0]={kv_seg[0]}")
    finally:
        ops.set_attn_mode(ops.DEFAULT_ATTN_MODE)


def test_lse_vs_fp64(device, case):
    """The log-sum-exp handed to the backward, mode 1.  Bound: 2e-5 of the scale, what the backward tests
    (tests/test_gpu_backward.py) ask of the gradients formed from it."""
    qkv, refs = case
    d = qkv.to(device)
    cu = ops.lengths_to_cu(LENS, device)
    ops.set_attn_mode(1)
    try:
        for kv_seg, (ref, ref_lse) in zip(KV_SEGS, refs):
            seg = torch.tensor(kv_seg, dtype=torch.int32, device=device)
            o, lse = ops.attention_raw(d[:, :256], d[:, 256:512], d[:, 512:], cu, seg, max(LENS), 8, want_lse=True)
            assert lse is not None, "mode 1 writes the log-sum-exp"
            _close(lse.cpu().numpy(), ref_lse, 2e-5, f"lse kv_seg[0]={kv_seg[0]}")
            _close(o.cpu().numpy(), ref, BOUND[1], f"output beside lse kv_seg[0]={kv_seg[0]}")
    finally:
        ops.set_attn_mode(ops.DEFAULT_ATTN_MODE)


def test_tiled_output_with_empty_waves_through_the_fused_stack(device):
    """The fused cross-encoder takes the core's TILED output, where a wave without a query writes zeros into its 32
    padding rows: clouds whose last 128-row tile has 1, 2 and 3 such waves, and a one-token cloud."""
    layer = TransformerCrossEncoderLayer(256, 8, 64, 0.0, 'relu', True, True, True, 'dot_prod')
    enc = TransformerCrossEncoder(layer, 2, torch.nn.LayerNorm(256))
    synthetic.fill_parameters(enc, seed=21)
    enc = enc.to(device)
    s_l, t_l = [129, 33, 257], [97, 161, 1]
    g = torch.Generator().manual_seed(5)
    T = sum(s_l) + sum(t_l)
    x = (torch.randn(T, 256, generator=g) * 1.7).to(device)
    pos = torch.rand(T, 256, generator=g).mul(2).sub(1).to(device)
    cu, s_self, s_cross, mx = make_segments(s_l, t_l, device)
    with torch.no_grad():
        fused = enc.forward_packed(x, cu, s_self, s_cross, mx, pos=pos, pos_bound=1.0)
        assert getattr(enc, '_spr_xenc', None) is not None, "the fused route was not taken"
        plain = enc.forward_packed(x, cu, s_self, s_cross, mx, pos=pos)     # no bound given: operator by operator
        again = enc.forward_packed(x, cu, s_self, s_cross, mx, pos=pos, pos_bound=1.0)
    assert torch.isfinite(fused).all()
    assert torch.equal(fused, again), "fused stack is not deterministic"
    _close(fused.cpu().numpy(), plain.cpu().numpy(), 5e-6, "fused vs operator route")
