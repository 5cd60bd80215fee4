"""CPU: the attention-map fixture against a float64 restatement, the recording layout and the
host-side argument checks of spr_attn_probs (no GPU needed)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from oracle import torch_oracle
from superpoints_registration_amd import _lib, synthetic
from superpoints_registration_amd.transformers import (AttnLayout, TransformerCrossEncoder,
                                                       TransformerCrossEncoderLayer)

D, NHEAD = 256, 8


def make_encoder(nlayers, d_ff, seed, pre_norm=True):
    layer = TransformerCrossEncoderLayer(D, NHEAD, d_ff, 0.0, normalize_before=pre_norm, sa_val_has_pos_emb=True,
                                         ca_val_has_pos_emb=True)
    enc = TransformerCrossEncoder(layer, nlayers, torch.nn.LayerNorm(D) if pre_norm else None)
    synthetic.fill_parameters(enc, seed=seed)
    return enc


def probs64(sd, p, prefix, q_in, k_in):
    """Head-averaged softmax weights of nn.MultiheadAttention (float64)."""
    w, b = sd[p + prefix + '.in_proj_weight'], sd[p + prefix + '.in_proj_bias']
    q = (q_in @ w[:D].t() + b[:D]).view(-1, NHEAD, D // NHEAD).transpose(0, 1)
    k = (k_in @ w[D:2 * D].t() + b[D:2 * D]).view(-1, NHEAD, D // NHEAD).transpose(0, 1)
    return torch.softmax(q @ k.transpose(1, 2) / math.sqrt(D // NHEAD), dim=-1).mean(0)


def maps_pre(sd, p, src, tgt, spe, tpe):
    """The four maps of TransformerCrossEncoderLayer.forward_pre (transformers.py:184-245), one pair."""
    def ln(x, n):
        return F.layer_norm(x, (D,), sd[p + n + '.weight'], sd[p + n + '.bias'], 1e-5)

    def att(prefix, q, k, v):
        return torch_oracle.mha(q, k, v, sd[p + prefix + '.in_proj_weight'], sd[p + prefix + '.in_proj_bias'],
                                sd[p + prefix + '.out_proj.weight'], sd[p + prefix + '.out_proj.bias'], NHEAD)

    s2p, t2p = ln(src, 'norm1') + spe, ln(tgt, 'norm1') + tpe
    ss, ts = probs64(sd, p, 'self_attn', s2p, s2p), probs64(sd, p, 'self_attn', t2p, t2p)
    src, tgt = src + att('self_attn', s2p, s2p, s2p), tgt + att('self_attn', t2p, t2p, t2p)
    s2p, t2p = ln(src, 'norm2') + spe, ln(tgt, 'norm2') + tpe
    return ss, ts, probs64(sd, p, 'multihead_attn', s2p, t2p), probs64(sd, p, 'multihead_attn', t2p, s2p)


def maps_post(sd, p, src, tgt, spe, tpe):
    """The four maps of TransformerCrossEncoderLayer.forward_post (transformers.py:122-182), one pair."""
    def ln(x, n):
        return F.layer_norm(x, (D,), sd[p + n + '.weight'], sd[p + n + '.bias'], 1e-5)

    def att(prefix, q, k, v):
        return torch_oracle.mha(q, k, v, sd[p + prefix + '.in_proj_weight'], sd[p + prefix + '.in_proj_bias'],
                                sd[p + prefix + '.out_proj.weight'], sd[p + prefix + '.out_proj.bias'], NHEAD)

    sp, tp = src + spe, tgt + tpe
    ss, ts = probs64(sd, p, 'self_attn', sp, sp), probs64(sd, p, 'self_attn', tp, tp)
    src, tgt = ln(src + att('self_attn', sp, sp, sp), 'norm1'), ln(tgt + att('self_attn', tp, tp, tp), 'norm1')
    sp, tp = src + spe, tgt + tpe
    return ss, ts, probs64(sd, p, 'multihead_attn', sp, tp), probs64(sd, p, 'multihead_attn', tp, sp)


def fixture_restatement(g):
    """Per pair and layer the four float64 maps of the fixture's configuration (unpadded)."""
    nl, d_ff = int(g["nlayers"]), int(g["d_ff"])
    sd = {k: v.double() for k, v in make_encoder(nl, d_ff, int(g["seed"])).state_dict().items()}
    out = []
    for b in range(g["src"].shape[1]):
        ns, nt = int((~g["src_mask"][b]).sum()), int((~g["tgt_mask"][b]).sum())
        src = torch.from_numpy(g["src"][:ns, b]).double()
        tgt = torch.from_numpy(g["tgt"][:nt, b]).double()
        spe = torch.from_numpy(g["src_pos"][:ns, b]).double()
        tpe = torch.from_numpy(g["tgt_pos"][:nt, b]).double()
        per_layer = []
        for l in range(nl):
            per_layer.append(maps_pre(sd, f'layers.{l}.', src, tgt, spe, tpe))
            src, tgt = torch_oracle.layer_pre(sd, f'layers.{l}.', src, tgt, spe, tpe, NHEAD)
        out.append((ns, nt, per_layer))
    return out


def test_fixture_matches_float64_restatement():
    g = load_golden("attn_maps_b2.npz")
    for b, (ns, nt, per_layer) in enumerate(fixture_restatement(g)):
        for l, (ss, ts, sx, tx) in enumerate(per_layer):
            for name, ref, rows, cols in (("src_satt", ss, ns, ns), ("tgt_satt", ts, nt, nt),
                                          ("src_xatt", sx, ns, nt), ("tgt_xatt", tx, nt, ns)):
                fx = g[name][l, b]
                assert np.abs(fx[:rows, :cols] - ref.numpy()).max() < 1e-6, (name, l, b)
                assert not fx[:rows, cols:].any()          # masked keys carry no weight


def test_get_attentions_raises_before_a_recorded_forward():
    enc = make_encoder(2, 64, seed=1)
    with pytest.raises(RuntimeError, match="no attention maps recorded"):
        enc.get_attentions()
    enc.record_attn = True
    assert all(l.record_attn for l in enc.layers)
    with pytest.raises(RuntimeError, match="no attention maps recorded"):
        enc.get_attentions()


def test_recording_layout_tiles_the_buffers():
    lay = AttnLayout([5, 3, 7, 2, 4, 6], None, torch.device("cpu"))
    assert (lay.B, lay.Ls, lay.Lt) == (3, 7, 6)
    for place, n in ((lay.place_self, lay.n_self), (lay.place_cross, lay.n_cross)):
        cover = np.zeros(n, np.int64)
        for off, ld, _, rows, cols in place.numpy():
            assert cols == ld
            cover[off:off + rows * ld] += 1
        assert (cover == 1).all()
    a, b = lay.split_cross(torch.arange(lay.n_cross, dtype=torch.float32))
    assert a.shape == (3, 7, 6) and b.shape == (3, 6, 7)
    assert int(b[1, 0, 0]) == int(lay.place_cross[4, 0])


def test_attn_probs_rejects_bad_arguments_on_the_host():
    L = _lib.lib()
    rc = L.spr_attn_probs(None, 256, None, 256, None, None, 20, 2, 10, 8, 64, 0.1, 0, None, None, 10, 10, None, 0,
                          None)
    assert rc != 0 and b"head_dim" in L.spr_last_error()
    rc = L.spr_attn_probs(None, 256, None, 256, None, None, 20, 2, 10, 8, 32, 0.1, 0, None, None, 10, 10, None, 0,
                          None)
    assert rc != 0 and b"null" in L.spr_last_error()
    assert L.spr_attn_probs_workspace_bytes(100, 8, 64) == 0
    assert L.spr_attn_probs_workspace_bytes(100, 8, 32) > 4 * 100 * 256 * 2


def test_attention_probs_refuses_cpu_tensors():
    from superpoints_registration_amd import ops
    x = torch.zeros(4, 256)
    with pytest.raises(RuntimeError, match="no\\s+CPU fallback"):
        ops.attention_probs(x, x, torch.tensor([0, 4], dtype=torch.int32), torch.tensor([0], dtype=torch.int32),
                            4, 8)
