"""CPU: the references of tests/attn_bwd_cases.py against each other, and the data of the recentring patterns.

  * replica_f64 (the backward's documented formulas, O and L as inputs) fed the exact float64 O and L reproduces torch
    autograd: the two references of tests/test_gpu_attn_bwd_routes.py agree before either meets the GPU.
  * the recentring patterns do what they are named for: the share of (query, head) rows on which the forward's key
    loop moves its reference exponent, in a float64 model of that loop.
  * the patterns are well conditioned: plain float32 arithmetic on the CPU stays far inside the GPU tests' 2e-5, so
    that bound is about the kernels and not about the data."""
import numpy as np
import pytest

import attn_bwd_cases as ac


def _case(name):
    if name == "edge":
        q, k, v, go, lens = ac.edge_case()
        return [(q, k, v, go, lens, kv) for kv in ac.KV_SEGS]
    return [ac.recentring_case(name)]


@pytest.fixture(scope="module")
def refs():
    """autograd_f64 of every case, computed once."""
    return {name: [(c, ac.autograd_f64(*c)) for c in _case(name)] for name in ("edge",) + ac.PATTERNS}


def test_edge_case_shape():
    q, k, v, go, lens = ac.edge_case()
    assert lens == [1, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 193] and sum(lens) == 932
    assert q.shape == k.shape == v.shape == go.shape == (932, 256)
    assert q.stride(0) == 768 and k.stride(0) == 768 and v.stride(0) == 768       # slices of one projection
    for kv in ac.KV_SEGS:
        assert sorted(kv) == list(range(len(lens)))
    # under the reversed map every short query length meets a long key length and the reverse
    pairs = {(lens[s], lens[ks]) for s, ks in enumerate(ac.KV_SEGS[1])}
    assert {(1, 193), (193, 1), (31, 129), (128, 32), (33, 97), (96, 63), (64, 65), (65, 64)} <= pairs


@pytest.mark.parametrize("name", ("edge",) + ac.PATTERNS)
def test_replica_reproduces_autograd(refs, name):
    for (q, k, v, go, lens, kv), (out, lse, *grads) in refs[name]:
        rep = ac.replica_f64(q, k, v, out, lse, go, lens, kv)
        ac.check_grads(rep, grads, 1e-12, f"replica {name} kv_seg[0]={kv[0]}")


@pytest.mark.parametrize("pattern", ac.PATTERNS)
def test_recentring_share(pattern):
    q, k, v, go, lens, kv = ac.recentring_case(pattern)
    n = ac.recentre_counts(q, k, lens, kv)
    once, twice = float((n >= 1).mean()), float((n >= 2).mean())
    print(f"{pattern}: rows that recentre at least once {once:.3f}, twice {twice:.3f}")
    if pattern == "spike_late":
        assert once >= 0.50
    elif pattern == "two_steps":
        assert twice >= 0.10 and once >= 0.90
    else:
        assert not n.any()


@pytest.mark.parametrize("pattern", ac.PATTERNS)
def test_recentring_patterns_are_well_conditioned(refs, pattern):
    (case, (out, lse, *grads)), = refs[pattern]
    g32 = ac.autograd_f32(*case)[2:]
    for (err, scale), nm in zip(ac.grad_errors(g32, grads), "qkv"):
        print(f"{pattern} d{nm}: float32 CPU autograd {err / scale:.3e} of the float64 gradient's largest entry")
        assert err <= 5e-6 * scale, f"{pattern} d{nm}: {err / scale:.3e}"
    lmax = float(lse.abs().max())
    print(f"{pattern}: max |L| {lmax:.2f}")
    assert lmax <= 64.0
    assert np.isfinite(out.numpy()).all()
