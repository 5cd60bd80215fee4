"""GPU: the one cache rule of ops.py (ops._derived) at the three sites that had no test of their own -- the
transposed weight of the linear backward, the weight-side inputs of the fused in-projection and the tile table of
the fused block tail -- each reached through its public operator at the smallest shape that takes the cached
route.  A derived value must be reused while its source is untouched, rebuilt after an in-place edit or
ops.invalidate_ranges(), never shared between tensors, and ordered against a consumer on another stream.
Every comparison of outputs is bitwise: both sides run the same kernels on the same values."""
import pytest
import torch

from superpoints_registration_amd import ops

pytestmark = pytest.mark.gpu

TAIL_SHAPE = (32, 0, 128)       # smallest (ka, kb, n_out) with a fused tail kernel (csrc/block_tail.hip tail_shape)


def _wt_case(device, seed):
    """LinearFn backward, x [64, 32], w [32, 32]: n % 32 == 0 and k >= 16, dX runs on ops.weight_transposed(w)."""
    g = torch.Generator().manual_seed(seed)
    x, dy = torch.randn(64, 32, generator=g).to(device), torch.randn(64, 32, generator=g).to(device)
    w = (torch.randn(32, 32, generator=g) * 0.1).to(device).requires_grad_(True)

    def run(w):
        xg = x.clone().requires_grad_(True)
        ops.linear(xg, w).backward(dy.clone())     # a gradient of its own: the backward attaches an unguarded range to it
        return xg.grad

    def edit(w):
        with torch.no_grad():
            w.mul_(3.0)
    return w, run, lambda w: getattr(w, "_spr_wt", None), edit


def _inproj_case(device, seed):
    """attention_inproj, T = 256 tokens (the threshold of the fused route) in two segments, d = 256, 8 heads."""
    g = torch.Generator().manual_seed(seed)
    d, lens = 256, [156, 100]
    x = torch.randn(sum(lens), d, generator=g).to(device)
    w = (torch.randn(3 * d, d, generator=g) * 0.05).to(device)
    b = (torch.randn(3 * d, generator=g) * 0.1).to(device)
    cu = ops.lengths_to_cu(lens, device)
    kv = torch.arange(len(lens), dtype=torch.int32, device=device)

    def run(w):
        return ops.attention_inproj(x, x, w, b, cu, kv, max(lens), 8, w_prep=ops.inproj_prepare(w))
    return w, run, lambda w: getattr(w, "_spr_inproj", None), lambda w: w.mul_(3.0)


def _tail_case(device, seed):
    """block_tail over three clouds of 70, 1 and 130 rows: a partial tile, a one-row cloud and three tiles."""
    g = torch.Generator().manual_seed(seed)
    ka, kb, n_out = TAIL_SHAPE
    tr = ops.block_tail_tile_rows(ka, kb, n_out)
    assert tr > 0
    xa = torch.randn(201, ka, generator=g).to(device)
    wa = (torch.randn(n_out, ka, generator=g) * 0.2).to(device)
    add = torch.randn(201, n_out, generator=g).to(device)
    cu = ops.lengths_to_cu([70, 1, 130], device)

    def edit(cu):
        cu[1:3] = torch.tensor([60, 61], dtype=torch.int32, device=device)     # clouds of 60, 1 and 140 rows
    run = lambda cu: ops.block_tail(xa, wa, cu, add=add)
    return cu, run, lambda cu: getattr(cu, f"_spr_tail_tiles_{tr}", None), edit


CASES = {"weight_transposed": _wt_case, "inproj_prepare": _inproj_case, "tail_tiles": _tail_case}


def _fresh(src):
    """A new tensor with equal data that has never been cached on."""
    return src.detach().clone().requires_grad_(src.requires_grad)


@pytest.fixture(autouse=True)
def _default_arithmetic(device):
    ops.set_gemm_mode(1)                    # the cached routes exist in the split-fp16 modes only
    ops.set_attn_mode(ops.DEFAULT_ATTN_MODE)


@pytest.mark.parametrize("case", CASES)
def test_derived_value_is_reused_and_rebuilt_with_its_source(device, case):
    src, run, entry, edit = CASES[case](device, 1)
    assert entry(src) is None
    y0 = run(src)
    first = entry(src)[1]
    assert torch.equal(run(src), y0) and entry(src)[1] is first, "hit: the cached object is reused"
    other = _fresh(src)                                               # equal data, another tensor: no aliasing
    assert entry(other) is None
    assert torch.equal(run(other), y0) and entry(other)[1] is not first and entry(src)[1] is first
    edit(src)                                                         # in-place edit: the version counter moves
    y1 = run(src)
    second = entry(src)[1]
    assert second is not first
    assert not torch.equal(y1, y0)
    assert torch.equal(y1, run(_fresh(src))), "after an in-place edit the output is that of a never-cached source"
    ops.invalidate_ranges()                                           # epoch: everything derived is dropped
    assert torch.equal(run(src), y1) and entry(src)[1] is not second


@pytest.mark.parametrize("case", CASES)
def test_derived_value_built_on_one_stream_is_ordered_for_another(device, case):
    """The guard's job: the value is built on the current stream BEHIND queued work, so a consumer on a second
    stream that did not wait for the build would read the buffer before it is written.  No synchronisation between
    the build and the second-stream call."""
    src, run, entry, _ = CASES[case](device, 2)
    want = run(_fresh(src))                                           # the operator entirely on one stream
    side = torch.cuda.Stream(device)
    busy = torch.zeros(1 << 26, device=device)
    torch.cuda.synchronize()                                          # inputs are ready for both streams
    assert entry(src) is None
    for _ in range(16):
        busy.add_(1.0)                                                # a few ms ahead of the build on this stream
    run(src)                                                          # builds the value on the current stream
    built = entry(src)[1]
    with torch.cuda.stream(side):
        got = run(src)
    assert entry(src)[1] is built and side.cuda_stream in entry(src)[2].seen
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_share_range_hands_the_range_to_a_detached_alias(device):
    x = torch.randn(64, 32, generator=torch.Generator().manual_seed(3)).to(device)
    ops.ensure_range(x)
    parts, n = ops._get_range(x)
    assert parts is not None and n > 0
    alias = x.detach().contiguous()
    assert alias is not x and ops._get_range(alias) == (None, 0)
    ops.share_range(x, alias)
    got = ops._get_range(alias)
    assert got[0] is parts and got[1] == n
    x.mul_(2.0)                                                       # the alias shares the version counter
    assert ops._get_range(alias) == (None, 0) and ops._get_range(x) == (None, 0)
