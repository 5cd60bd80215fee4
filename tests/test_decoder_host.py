"""CPU: the KPConv decoder's construction (kpconv.KPFDecoder, kpconv_blocks.NearestUpsampleBlock, KPFEncoder's skip
bookkeeping with a decoder behind it) against the values the reference's constructors gave
(tests/golden/decoder_3dmatch.npz, scripts/gen_decoder_golden.py), and the plain-torch restatement of the decoder
(tests/decoder_cases.py) against the reference's outputs."""
import numpy as np
import pytest
import torch

import decoder_cases as dc
from conftest import load_golden
from superpoints_registration_amd import get_config, synthetic
from superpoints_registration_amd.kpconv import KPFDecoder, KPFEncoder, plan_pyramid
from superpoints_registration_amd.kpconv_blocks import NearestUpsampleBlock, UnaryBlock, block_decider

TAGS = ("3dmatch", "kitti", "modelnet")


@pytest.fixture(scope="module")
def gold():
    return load_golden("decoder_3dmatch.npz")


def _full_decoder(tag):
    cfg = get_config(tag)
    levels = sum("strided" in b for b in cfg.architecture)
    cfg["architecture"] = list(cfg.architecture) + ["nearest_upsample", "unary"] * levels
    return cfg


@pytest.mark.parametrize("reduce", [True, False])
@pytest.mark.parametrize("tag", TAGS)
def test_constructor_bookkeeping_is_the_references(gold, tag, reduce):
    cfg = _full_decoder(tag)
    enc = KPFEncoder(cfg, cfg.d_embed)
    dec = KPFDecoder(cfg, enc.encoder_skip_dims[-1], enc.encoder_skip_dims, reduce_channel_when_upsample=reduce)
    k = f"book|{tag}|{int(reduce)}|"
    assert enc.encoder_skips == gold[k + "skips"].tolist()
    assert enc.encoder_skip_dims == gold[k + "skip_dims"].tolist()
    assert dec.decoder_concats == gold[k + "concats"].tolist()
    assert [repr(b) for b in dec.decoder_blocks] == gold[k + "reprs"].tolist()
    assert list(dec.state_dict().keys()) == gold[k + "keys"].tolist()
    dims = [[b.in_dim, b.out_dim] for b in dec.decoder_blocks if isinstance(b, UnaryBlock)]
    assert dims == gold[k + "dims"].tolist()
    # forward() appends one skip per strided block: the listed upsample index is never reached
    assert len(enc.encoder_blocks) == enc.encoder_skips[-1]
    # the widths of every projection are multiples of 32: the fused call has a kernel for each of them
    for (kin, nout), j in zip(dims, dec.decoder_concats):
        ks = enc.encoder_skip_dims[dec.decoder_blocks[j - 1].layer_ind - 1]
        assert (kin - ks) % 32 == 0 and ks % 32 == 0 and nout % 32 == 0


def test_3dmatch_decoder_is_the_one_the_issue_names(gold):
    cfg = dc.with_decoder(get_config("3dmatch"))
    enc = KPFEncoder(cfg, cfg.d_embed)
    dec = KPFDecoder(cfg, 512, enc.encoder_skip_dims)
    assert enc.encoder_skips == [2, 5, 8] and enc.encoder_skip_dims == [128, 256, 512]
    assert dec.decoder_concats == [1, 3]
    assert [(b.in_dim, b.out_dim) for b in dec.decoder_blocks if isinstance(b, UnaryBlock)] == [(768, 256), (384, 128)]
    assert repr(dec.decoder_blocks[0]) == "NearestUpsampleBlock(layer: 2 -> 1)"
    assert list(dec.state_dict().keys()) == gold["state_dict_keys"].tolist() == \
        ["decoder_blocks.1.mlp.weight", "decoder_blocks.3.mlp.weight"]
    cfg_b = dc.with_decoder(get_config("3dmatch"), use_batch_norm=False)
    dec_b = KPFDecoder(cfg_b, 512, KPFEncoder(cfg_b, cfg_b.d_embed).encoder_skip_dims)
    assert list(dec_b.state_dict().keys()) == gold["bias|state_dict_keys"].tolist()
    assert "decoder_blocks.1.batch_norm.bias" in dec_b.state_dict()
    dec_b.load_state_dict({k: torch.zeros_like(v) for k, v in dec_b.state_dict().items()}, strict=True)


@pytest.mark.parametrize("tag", TAGS)
def test_without_a_decoder_nothing_changes(tag):
    cfg = get_config(tag)
    enc = KPFEncoder(cfg, cfg.d_embed)
    strided = [i for i, b in enumerate(cfg.architecture) if "strided" in b]
    assert enc.encoder_skips == strided + [len(cfg.architecture) - 1]
    assert len(enc.encoder_blocks) == len(cfg.architecture)
    if tag == "3dmatch":
        assert enc.encoder_skips == [2, 5, 7] and enc.encoder_skip_dims == [128, 256, 512]
    # the pyramid plan stops at the first upsample block: same blocks, same levels
    assert plan_pyramid(_full_decoder(tag)) == plan_pyramid(cfg)


@pytest.mark.parametrize("name", ["unary2", "global_average", "max_pool", "max_pool_wide", "simple_deformable",
                                  "resnetb_deformable_strided", "simple_equivariant", "resnetb_invariant",
                                  "nearest_upsample_2", "upsample"])
def test_unsupported_block_names_still_raise(name):
    with pytest.raises((ValueError, NotImplementedError)):
        block_decider(name, 0.1, 128, 128, 1, get_config("3dmatch"))


def test_block_decider_builds_the_upsample_block():
    b = block_decider("nearest_upsample", 0.1, 128, 128, 2, get_config("3dmatch"))
    assert isinstance(b, NearestUpsampleBlock) and b.layer_ind == 2 and not list(b.parameters())


def _small(gold, bias=False):
    cfg = dc.with_decoder(get_config("3dmatch"), use_batch_norm=not bias)
    enc = KPFEncoder(cfg, cfg.d_embed)
    dec = KPFDecoder(cfg, enc.encoder_skip_dims[-1], enc.encoder_skip_dims)
    synthetic.fill_parameters(dc.Backbone(enc, dec), seed=int(gold["seed"]))
    return dec


def test_seeded_decoder_weights_are_the_goldens(gold):
    dec = _small(gold)
    for name, p in dec.state_dict().items():
        assert abs(float(p.double().norm()) - float(gold[f"weight|{name}|norm"])) <= 1e-12 * float(gold[f"weight|{name}|norm"])
        assert abs(float(p.double().sum()) - float(gold[f"weight|{name}|sum"])) <= 1e-9


@pytest.mark.parametrize("bias", [False, True])
def test_the_restated_decoder_is_the_references(gold, bias):
    """tests/decoder_cases.restated_decoder in float64 on the reference's own inputs: within 1e-5 of the tensor's scale
    of the reference's float32 x_all, or within 4 x the float32 restatement's own distance from float64."""
    dec = _small(gold, bias)
    T = torch.from_numpy
    w = [dec.decoder_blocks[1].mlp.weight.detach(), dec.decoder_blocks[3].mlp.weight.detach()]
    b = [dec.decoder_blocks[j].batch_norm.bias.detach() for j in (1, 3)] if bias else None
    up0 = [T(gold[f"small|upsamples{l}"][:, 0].astype(np.int64)) for l in (0, 1)]
    lens = [gold[f"small|lens{l}"] for l in (0, 1, 2)]
    out = {}
    for dt in (torch.float64, torch.float32):
        out[dt] = dc.restated_decoder(T(gold["small|enc_out"]).to(dt), [T(gold[f"small|skip{l}"]).to(dt) for l in (0, 1)],
                                      up0, lens, [t.to(dt) for t in w], None if b is None else [t.to(dt) for t in b])
    for j in (0, 1):
        ref = T(gold[f"small|bias|x_all{j}" if bias else f"small|x_all{j}"]).double()
        err = float((out[torch.float64][j] - ref).abs().max())
        err32 = float((out[torch.float32][j].double() - out[torch.float64][j]).abs().max())
        assert err <= max(1e-5 * float(ref.abs().max()), 4 * err32), (j, err, err32)
