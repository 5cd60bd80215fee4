"""Shared by scripts/gen_decoder_golden.py, tests/test_decoder_host.py and tests/test_gpu_decoder.py: the decoder cases of
tests/golden/decoder_3dmatch.npz, the row-sampling rule of that file, and the decoder restated in plain torch (any
dtype: the float64 reference of the gradient test and the float32 evaluation behind the 4 * err32 rule).

The fixture holds two reference runs (Preprocessor -> KPFEncoder -> KPFDecoder, 3DMatch architecture + DECODER):

  big    clouds of BIG_SIZES points in a 0.6 box.  Inputs are regenerated from seeds (clouds: cloud(); weights:
         synthetic.fill_parameters(Backbone, seed)); of the outputs only every ROW_STEP-th row of each x_all tensor is
         kept (sample_rows) -- the whole tensors, with the encoder output and skips they come from, are 4.8 MB of float32
         and a committed file holds 1 MiB at most.  Serves the end-to-end test.
  small  clouds of SMALL_SIZES points: everything whole -- encoder output, skips, upsamples, x_all, the gradients of
         sum(y * g) with respect to the three inputs, and the sampled gradients of the two weights.  Serves the tests
         that feed the decoder the reference's own tensors.  The same inputs through the reference decoder with
         use_batch_norm: False (seeded bias) pin the bias variant.
"""
import numpy as np
import torch

DECODER = ['nearest_upsample', 'unary', 'nearest_upsample', 'unary']
BIG_SIZES = (900, 500, 40)
SMALL_SIZES = (40, 25)
BOX = 0.6
ROW_STEP = 16
SEED = 0
G_SEED = 900          # upstream gradient of x_all[l]: synthetic.rand(shape, G_SEED + l)
W_SAMPLES = 4096      # pinned entries of a weight gradient (oracle.gen_golden.grad_sample_indices(name, numel, k))


def cloud(n, seed):
    """n points on three faces of a BOX-sized box with 2 mm of noise, float32 (synthetic.box_faces)."""
    from superpoints_registration_amd import synthetic
    rng = np.random.default_rng(seed)
    return (synthetic.box_faces(n, rng, BOX) + rng.normal(0.0, 0.002, (n, 3))).astype(np.float32)


def clouds(case, cloud_seed):
    sizes = BIG_SIZES if case == 'big' else SMALL_SIZES
    return [cloud(n, 1000 * cloud_seed + 10 * i + (0 if case == 'big' else 5)) for i, n in enumerate(sizes)]


def sample_rows(n):
    return np.arange(0, n, ROW_STEP)


def with_decoder(cfg, use_batch_norm=True):
    """A copy of the config with DECODER appended to its architecture."""
    import copy
    cfg = copy.deepcopy(cfg)
    cfg['architecture'] = list(cfg['architecture']) + DECODER
    cfg['use_batch_norm'] = use_batch_norm
    return cfg


class Backbone(torch.nn.Module):
    """encoder + decoder under fixed names, so that synthetic.fill_parameters draws the same weights for the
    reference's modules and for this package's."""

    def __init__(self, encoder, decoder):
        super().__init__()
        self.encoder, self.decoder = encoder, decoder


def restated_decoder(x, skips, up0, lens, weights, biases=None, slope=0.1, eps=1e-5):
    """KPFDecoder.forward for DECODER in plain torch, in the dtype of x: per pair closest_pool (shadow index -> zero
    row), cat, mlp (no bias), per-cloud InstanceNorm1d (biased variance, eps) or `+ bias`, LeakyReLU(slope).
    skips = [level 0, level 1] (popped from the end); up0[l] = column 0 of the upsamples matrix of level l (int64);
    lens[l] = per-cloud row counts of level l; weights = [first unary, second unary].  Returns x_all."""
    x_all = []
    skips = list(skips)
    for j, w in enumerate(weights):
        level = len(weights) - 1 - j
        ext = torch.cat([x, torch.zeros_like(x[:1])], 0)
        idx = up0[level].clamp(min=-1)
        idx = torch.where((idx < 0) | (idx >= x.shape[0]), torch.full_like(idx, x.shape[0]), idx)
        y = torch.cat([ext[idx], skips.pop()], 1) @ w.t()
        if biases is None:
            out, o = [], 0
            for n in lens[level]:
                seg = y[o:o + int(n)]
                mean = seg.mean(0, keepdim=True)
                var = ((seg - mean) ** 2).mean(0, keepdim=True)
                out.append((seg - mean) / torch.sqrt(var + eps))
                o += int(n)
            y = torch.cat(out, 0)
        else:
            y = y + biases[j]
        x = torch.nn.functional.leaky_relu(y, slope)
        x_all.append(x)
    return x_all
