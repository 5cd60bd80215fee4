"""CPU: which inputs SimpleBlock.forward sends to the fused stem call (stem.stem_predicate / stem_route), that the
library's own shape rule agrees with it, and what the two entry points refuse on the host before any launch."""
import torch

from superpoints_registration_amd import _lib, stem

W = (15, 1, 64)


def test_routing_predicate():
    ok = dict(on_gpu=True, wants_grad=False, use_bn=True, x_channels=1, weights_shape=W)
    assert stem.stem_predicate(**ok)
    assert not stem.stem_predicate(**{**ok, "on_gpu": False})             # CPU tensors: the operator route refuses them
    assert not stem.stem_predicate(**{**ok, "wants_grad": True})          # training keeps kpconv + instnorm
    assert not stem.stem_predicate(**{**ok, "use_bn": False})             # bias instead of the norm
    assert not stem.stem_predicate(**{**ok, "x_channels": 4})
    assert not stem.stem_predicate(**{**ok, "weights_shape": (15, 4, 64)})     # Cin = 4 (KITTI-style inputs)
    assert not stem.stem_predicate(**{**ok, "weights_shape": (15, 1, 40)})     # Cout no multiple of 16
    assert not stem.stem_predicate(**{**ok, "weights_shape": (17, 1, 64)})     # more than 16 kernel points
    assert not stem.stem_predicate(**{**ok, "weights_shape": (15, 1, 8)})
    assert stem.stem_predicate(**{**ok, "weights_shape": (16, 1, 16)})
    assert stem.stem_predicate(**{**ok, "weights_shape": (1, 1, 128)})


def test_route_reads_the_tensors_state():
    x = torch.ones(5, 1)
    w = torch.nn.Parameter(torch.zeros(W))
    with torch.no_grad():
        assert stem.stem_route(x, w, True) is False                        # not on the GPU
        assert stem.stem_route(None, w, True) is False
    assert stem.stem_route(x, w, True) is False


def test_library_rule_is_the_predicates():
    L = _lib.lib()
    for cin in (1, 2, 32):
        for cout in (0, 8, 16, 24, 40, 48, 64, 128, 256):
            for n_kp in (0, 1, 15, 16, 17):
                assert bool(L.spr_kpconv_stem_supported(cin, cout, n_kp)) == stem.stem_shape_ok(cin, cout, n_kp)


def test_size_query_and_host_side_refusals():
    L = _lib.lib()
    small, big = L.spr_kpconv_stem_workspace_size(1000, 1100, 3, 600, 64), L.spr_kpconv_stem_workspace_size(2000, 1100, 3, 600, 64)
    assert 0 < small < big
    assert small >= 1000 * 16 * 4 + 1100 * 16                              # the influence sums and the support records
    assert L.spr_kpconv_stem_workspace_size(1000, 1100, 3, 1100, 64) > small   # one more statistics slice per cloud
    args = lambda cout, n_kp: (None, 100, None, 120, None, 20, 20, 1, None, None, cout, None, n_kp, 0.1, None, 2, 60,
                               1e-5, 0.1, None, None, 0, None, None, None, 0, None)
    assert L.spr_kpconv_stem(*args(40, 15)) != 0 and b"no kernel" in L.spr_last_error()
    assert L.spr_kpconv_stem(*args(64, 17)) != 0 and b"no kernel" in L.spr_last_error()
    assert L.spr_kpconv_stem(*args(64, 15)) != 0 and b"workspace too small" in L.spr_last_error()
    # the sine embedding keeps d_model / 6 frequencies in a table of 1024
    assert L.spr_posemb_sine(None, 4, 6150, 1.0, 10000.0, None, None) != 0 and b"frequency table" in L.spr_last_error()
