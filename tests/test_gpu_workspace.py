"""GPU: every operator inside exactly the workspace its size query reports, poisoned (tests/workspace_arena.py).

ops._workspace keeps one grow-only buffer of at least 1 MiB per stream and every caller passes the whole buffer as
ws_bytes, so the rest of the suite cannot see an operator that (1) writes past what its query reported, (2) reads
scratch it never wrote, or (3) expects bytes to survive until a later call.  Here every case runs three times --
production, under Arena(poison=0xFF) (NaN in every float format, -1 in every integer width) and under
Arena(poison=0x00) -- and must give the same BITS each time, finite wherever production is finite, with every guard
band intact.  Bit equality is the bar: the atomics of csrc/ are integer atomics and every operator promises
reproducible results.  A case whose shape no existing test holds against float64 also compares production with a
float64 evaluation on the CPU under that operator's existing criterion (imported from its test module, or restated
with the test named where it is written inline there); a case that reuses an existing test's inputs names that test.

The two poisoned runs also sit in the tensor arena (tests/tensor_arena.py): every tensor the host layer allocates with
torch.empty and its kin -- the outputs, the scratch handed over by pointer, plans and planes -- lies between guard
bands and starts out as poison, 0xFF with the 0xFF workspace and zeros with the zero one.  The same three runs then
also show a store outside a tensor, a returned element that was never written (the caching allocator would hand
production last call's correct value there) and scratch read before it is written.  Regions of a returned tensor
that include/spr.h declares not written are cut away inside the case (_owned).

The last test of the module checks that the cases above reached every `_workspace(` / `_loss_ws(` call site of every
module of the package: a new operator fails it until it has a case here.  Run the module as a whole."""
import math
import os
import re

import numpy as np
import pytest
import torch

import forward_cases as fc
from attn_bwd_cases import MinBwdLib as _MinBwdLib, attention_grads_f64 as _attention_f64
from conftest import load_golden
from oracle import torch_oracle as O
from oracle.gen_golden import loss_inputs, ops_inputs, pairs_for
from superpoints_registration_amd import _lib, autograd, get_config, ops, synthetic
from superpoints_registration_amd.regtr import RegTR
from superpoints_registration_amd.transformers import make_segments
from test_gpu_attn_maps import _ref_maps
from test_gpu_backward import _rel
from test_gpu_block_tail import LENS as TAIL_LENS, SHAPES as TAIL_SHAPES, _inputs as tail_inputs
from test_gpu_circle_loss import REGIMES as CIRCLE_REGIMES, make_case as circle_case, run as circle_run
from test_gpu_forward_range import _bounded
from test_gpu_match_range import U, _check_dual_softmax, _check_sinkhorn, _ds_ref, _infonce64, _coef
from test_gpu_ops import _close
from test_gpu_posemb_learned import BWD_SEEDS, _ours as posemb_grads, bwd_case as posemb_case
from test_gpu_refine import pack as refine_pack, synth_pair
from test_gpu_xenc import _encoder, _oracle64
from tensor_arena import TensorArena
from workspace_arena import GUARD, Arena

pytestmark = pytest.mark.gpu
T = torch.from_numpy
SEEN = set()             # (file, line) of every _workspace / _loss_ws call site the cases reached


def _flat(obj, out=None):
    """Every tensor inside a result (tensors, lists, tuples, dicts; None and host values are skipped), in a fixed order."""
    out = [] if out is None else out
    if isinstance(obj, torch.Tensor):
        out.append(obj.detach())
    elif isinstance(obj, dict):
        for k in sorted(obj, key=str):
            _flat(obj[k], out)
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            _flat(o, out)
    return out


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8) if t.numel() else t.reshape(-1)


def run_three(monkeypatch, f, what, guard=GUARD, verify_every=0, placed=False):
    """production / poison 0xFF / poison 0x00; asserts in the order: guards, finiteness, bit equality.  Returns the
    production result.  The two poisoned runs also sit in the tensor arena (tests/tensor_arena.py), flavour 1 with 0xFF
    and flavour 2 with 0x00: every tensor the case allocates through Python -- outputs, host-side scratch, plans and
    planes -- lies between bands that are checked after the workspace guards, and its unwritten elements hold the
    poison, so the finiteness and bit-equality checks below speak for them as well.
    placed: f takes one argument, put, and passes its inputs through it: the identity in production, the arena's put()
    in the poisoned runs, where every input then ends flush against a band (tests/test_gpu_tensor_bounds.py, whose
    cases include operators without a workspace: only there may a case ask for none)."""
    production = f(lambda t: t) if placed else f()
    runs, arenas, tensor_arenas = [_flat(production)], [], []
    for flavour, poison in ((1, 0xFF), (2, 0x00)):
        arena = Arena(poison, guard, verify_every)
        tensors = TensorArena(flavour, guard, verify_every)
        with monkeypatch.context() as m:
            m.setattr(ops, "_workspace", arena)
            tensors.install(m)
            runs.append(_flat(f(tensors.put) if placed else f()))
        arenas.append(arena)
        tensor_arenas.append(tensors)
        SEEN.update(arena.callers)
    for arena in arenas:
        arena.verify()
        if not placed:
            assert arena.calls > 0, f"{what}: the case never asked for a workspace"
    for tensors in tensor_arenas:
        tensors.verify()
        assert tensors.calls > 0, f"{what}: the case never allocated a tensor"
    prod = runs[0]
    assert len(prod) > 0 and all(len(r) == len(prod) for r in runs), what
    for name, run in (("0xFF", runs[1]), ("0x00", runs[2])):
        for i, (p, r) in enumerate(zip(prod, run)):
            assert p.shape == r.shape and p.dtype == r.dtype, f"{what}: output {i} under poison {name}"
            if p.is_floating_point():
                ok = torch.isfinite(p)
                assert bool(torch.isfinite(r)[ok].all()), f"{what}: output {i} is not finite under poison {name}"
    for name, run in (("0xFF", runs[1]), ("0x00", runs[2])):
        for i, (p, r) in enumerate(zip(prod, run)):
            assert torch.equal(_bits(p), _bits(r)), \
                f"{what}: output {i} under poison {name} differs from production in " \
                f"{int((_bits(p) != _bits(r)).sum())} bytes"
    return production


# ---- token operators ---------------------------------------------------------------------------------------------------
# ragged with a one-token cloud and a partly empty last tile / the smallest batch / whole 64-row tiles
SEGS = {"ragged": ([70, 129, 33], [200, 1, 64]), "one": ([1], [1]), "tiles": ([64, 64], [64, 64])}


def _tokens(name, device, seed):
    s_l, t_l = SEGS[name]
    lens = list(s_l) + list(t_l)
    cu, s_self, s_cross, mx = make_segments(s_l, t_l, device)
    B = len(s_l)
    kv_cross = list(range(B, 2 * B)) + list(range(B))
    qkv = synthetic.rand((sum(lens), 768), seed, -1.5, 1.5)
    return lens, cu, s_self, s_cross, kv_cross, mx, qkv


def _attn_ref64(qkv, lens, kv_seg):
    offs = np.concatenate([[0], np.cumsum(lens)])
    ref = torch.zeros((sum(lens), 256), dtype=torch.float64)
    for s in range(len(lens)):
        ks = kv_seg[s]
        q = qkv[offs[s]:offs[s + 1], :256].double().view(-1, 8, 32).transpose(0, 1)
        k = qkv[offs[ks]:offs[ks + 1], 256:512].double().view(-1, 8, 32).transpose(0, 1)
        v = qkv[offs[ks]:offs[ks + 1], 512:].double().view(-1, 8, 32).transpose(0, 1)
        a = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(32), -1)
        ref[offs[s]:offs[s + 1]] = (a @ v).transpose(0, 1).reshape(-1, 256)
    return ref


@pytest.mark.parametrize("segs", list(SEGS))
def test_attention_core(device, monkeypatch, segs):
    lens, cu, s_self, s_cross, kv_cross, mx, qkv = _tokens(segs, device, 9)
    d = qkv.to(device)

    def f():
        return [ops.attention_raw(d[:, :256], d[:, 256:512], d[:, 512:], cu, seg, mx, 8, want_lse=True)
                for seg in (s_self, s_cross)]
    (o_self, _), (o_cross, _) = run_three(monkeypatch, f, f"attention {segs}")
    # test_gpu_ops.py::test_attention_core_vs_fp64, default mode
    _close(o_self.cpu().numpy(), _attn_ref64(qkv, lens, list(range(len(lens)))).numpy(), 3e-5, "attention self")
    _close(o_cross.cpu().numpy(), _attn_ref64(qkv, lens, kv_cross).numpy(), 3e-5, "attention cross")


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("segs", list(SEGS))
def test_attention_with_in_projection(device, monkeypatch, segs, shared):
    """ragged: 497 tokens, the fused route (>= 256); tiles: exactly 256; one: the plain projection into the workspace."""
    lens, cu, s_self, s_cross, kv_cross, mx, _ = _tokens(segs, device, 9)
    tot = sum(lens)
    x_qk = synthetic.rand((tot, 256), 31, -1.5, 1.5)
    x_v = x_qk if shared else synthetic.rand((tot, 256), 32, -1.5, 1.5)
    w, b = synthetic.rand((768, 256), 33, -0.1, 0.1), synthetic.rand((768,), 34, -0.2, 0.2)
    d_qk = x_qk.to(device)
    d_v = d_qk if shared else x_v.to(device)
    dw, db = w.to(device), b.to(device)

    def f():
        return ops.attention_inproj(d_qk, d_v, dw, db, cu, s_cross, mx, 8, w_prep=ops.inproj_prepare(dw))
    o = run_three(monkeypatch, f, f"in-projection {segs} shared={shared}")
    qkv = torch.cat([x_qk.double() @ w[:512].double().t() + b[:512].double(),
                     x_v.double() @ w[512:].double().t() + b[512:].double()], 1)
    # test_gpu_ops.py::test_attention_with_fused_in_projection_vs_fp64, default mode
    _close(o.cpu().numpy(), _attn_ref64(qkv, lens, kv_cross).numpy(), 3e-5, "in-projection attention")


@pytest.mark.parametrize("average", [True, False])
@pytest.mark.parametrize("segs", list(SEGS))
def test_attention_probs(device, monkeypatch, segs, average):
    lens, cu, s_self, s_cross, kv_cross, mx, qkv = _tokens(segs, device, 12)
    d = qkv.to(device)
    p = run_three(monkeypatch, lambda: ops.attention_probs(d[:, :256], d[:, 256:512], cu, s_cross, mx, 8, average=average),
                  f"attention_probs {segs}")
    # test_gpu_attn_maps.py::test_operator_matches_float64: 1e-5 absolute on the maps, exact zeros in the padding
    maps = p.cpu().double()
    for s, ref in enumerate(_ref_maps(d[:, :256], d[:, 256:512], lens, kv_cross, average)):
        lq, lk = lens[s], lens[kv_cross[s]]
        got = maps[s]
        assert (got[..., :lq, :lk] - ref).abs().max().item() <= 1e-5, (segs, s)
        assert not got[..., lq:, :].any() and not got[..., :, lk:].any()


@pytest.mark.parametrize("route", ["planes", "min"])
@pytest.mark.parametrize("segs", list(SEGS))
def test_attention_backward(device, monkeypatch, segs, route):
    lens, cu, s_self, s_cross, kv_cross, mx, qkv = _tokens(segs, device, 41)
    d = qkv.to(device)
    q, k, v = d[:, :256].contiguous(), d[:, 256:512].contiguous(), d[:, 512:].contiguous()
    go = synthetic.rand((sum(lens), 256), 44)
    dgo = go.to(device)
    if route == "min":
        real = _lib.lib()
        monkeypatch.setattr(_lib, "lib", lambda: _MinBwdLib(real))

    def f():
        out, lse = ops.attention_raw(q, k, v, cu, s_cross, mx, 8, want_lse=True)
        return ops.attention_bwd(q, k, v, out, dgo, cu, kv_cross, mx, 8, lse=lse)
    grads = run_three(monkeypatch, f, f"attention backward {segs} {route}")
    # test_gpu_backward.py: 2e-5 of each gradient's largest entry.  With one key per query (`one`) the probabilities are
    # exactly 1 and the float64 dq and dk are exactly 0: that criterion has no scale there, so those two are held to
    # 2e-5 of the largest entry of the three gradients together (they share dO and operands of one magnitude).
    ref = _attention_f64(qkv[:, :256], qkv[:, 256:512], qkv[:, 512:], go, lens, kv_cross)
    joint = max(float(r.abs().max()) for r in ref)
    for got, r, nm in zip(grads, ref, "qkv"):
        if float(r.abs().max()) == 0.0:
            assert segs == "one" and nm in "qk"
            assert float(got.abs().max()) <= 2e-5 * joint, f"attention d{nm} {segs} {route}: {float(got.abs().max()):.2e}"
        else:
            assert _rel(got, r) <= 2e-5, f"attention d{nm} {segs} {route}: {_rel(got, r):.2e}"


@pytest.mark.parametrize("n_layers,final", [(1, True), (2, False)])
@pytest.mark.parametrize("segs", list(SEGS))
def test_cross_encoder_stack(device, monkeypatch, segs, n_layers, final):
    s_l, t_l = SEGS[segs]
    enc = _encoder(device, n_layers, 1024, final)
    g = torch.Generator().manual_seed(5)
    tot = sum(s_l) + sum(t_l)
    x = (torch.randn(tot, 256, generator=g) * 1.7).to(device)
    pos = torch.rand(tot, 256, generator=g).mul(2).sub(1).to(device)
    cu, s_self, s_cross, mx = make_segments(s_l, t_l, device)

    def f():
        with torch.no_grad():
            return enc.forward_packed(x, cu, s_self, s_cross, mx, pos=pos, pos_bound=1.0)
    fused = run_three(monkeypatch, f, f"xenc {segs} {n_layers} layers")
    assert getattr(enc, '_spr_xenc', None) is not None, "the fused route was not taken"
    # test_gpu_xenc.py::test_stack_against_float64_and_the_operator_route: 2e-5 of the output scale
    _close(fused.cpu().numpy(), _oracle64(enc, x, pos, s_l, t_l), 2e-5, f"xenc {segs} vs float64")


# ---- products and reductions -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,k,n", [(1, 256, 256), (257, 64, 32)])
def test_linear_forward_and_backward(device, monkeypatch, m, k, n):
    """spr_linear (constant workspace), dW through spr_tn_product_split, db through spr_colsum."""
    x, w = synthetic.rand((m, k), 1, -3.0, 3.0), synthetic.rand((n, k), 2, -0.2, 0.2)
    b, r, go = synthetic.rand((n,), 3), synthetic.rand((m, n), 4), synthetic.rand((m, n), 5).to(device)

    def f():
        lx, lw, lb, lr = (t.clone().to(device).requires_grad_(True) for t in (x, w, b, r))
        y = ops.linear(lx, lw, lb, lr, ops.ACT_RELU)
        y.backward(go)
        return y, lx.grad, lw.grad, lb.grad, lr.grad
    y, dx, dw, db, _ = run_three(monkeypatch, f, f"linear {m}x{k}x{n}")
    cx, cw, cb, cr = (t.double().requires_grad_(True) for t in (x, w, b, r))
    ref = torch.relu(cx @ cw.t() + cb + cr)
    ref.backward(go.cpu().double())
    _close(y.detach().cpu().numpy(), ref.detach().numpy(), 2e-6 * max(1, k // 256), "linear")       # test_gpu_ops.py
    for got, c, nm in ((dx, cx, "dx"), (dw, cw, "dw"), (db, cb, "db")):
        assert _rel(got, c.grad) <= 2e-5, f"linear {nm}: {_rel(got, c.grad):.2e}"          # test_gpu_backward.py


@pytest.mark.parametrize("rows", [1, 257])
def test_tn_product_f64(device, monkeypatch, rows):
    L = synthetic.rand((rows, 15), 6).to(device)
    R = synthetic.rand((rows, 64), 7).to(device)
    out = run_three(monkeypatch, lambda: autograd._tn_product(L, R, rows, 15, 64, f64=True), f"tn_product_f64 {rows}")
    ref = L.cpu().double().t() @ R.cpu().double()
    assert _rel(out, ref) <= 2e-5


@pytest.mark.parametrize("m", [1, 257])
def test_layernorm_backward(device, monkeypatch, m):
    x, g, b, p = synthetic.rand((m, 256), 5, -3, 5), synthetic.rand((256,), 6, 0.5, 1.5), synthetic.rand((256,), 7), \
        synthetic.rand((m, 256), 8)
    g1, g2 = synthetic.rand((m, 256), 9).to(device), synthetic.rand((m, 256), 10).to(device)

    def f():
        lx, lg, lb = (t.clone().to(device).requires_grad_(True) for t in (x, g, b))
        n, npos = ops.layernorm(lx, lg, lb, 1e-5, pos=p.to(device))
        (n * g1).sum().add((npos * g2).sum()).backward()
        return lx.grad, lg.grad, lb.grad
    got = run_three(monkeypatch, f, f"layernorm backward {m}")
    cx, cg, cb = (t.double().requires_grad_(True) for t in (x, g, b))
    y = torch.nn.functional.layer_norm(cx, (256,), cg, cb, 1e-5)
    ((y * g1.cpu().double()).sum() + ((y + p.double()) * g2.cpu().double()).sum()).backward()
    for a, c, nm in zip(got, (cx, cg, cb), ("dx", "dgamma", "dbeta")):
        assert _rel(a, c.grad) <= 2e-5, f"layernorm {nm}: {_rel(a, c.grad):.2e}"         # test_gpu_backward.py


@pytest.mark.parametrize("tokens", [1, 63, 64, 65])
def test_posemb_mlp_backward(device, monkeypatch, tokens):
    """The inputs of test_gpu_posemb_learned.py::test_backward_against_float64_autograd, which holds exactly these
    shapes and values against float64."""
    xyz, params, dpe, _ = posemb_case(load_golden("posemb_learned_ops.npz"), tokens, BWD_SEEDS[tokens])
    run_three(monkeypatch, lambda: posemb_grads(device, xyz, params, dpe), f"posemb_mlp backward T={tokens}")


# ---- point operators ---------------------------------------------------------------------------------------------------
POINT_COUNTS = [(255, 1, 257), (256, 257, 1)]


def _clouds(counts, device, seed):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0, 1, (sum(counts), 3)).astype(np.float32)
    return pts, T(pts).to(device), ops.lengths_to_cu(list(counts), device)


@pytest.mark.parametrize("counts", POINT_COUNTS)
def test_subsampling_and_ordering(device, monkeypatch, counts):
    _, pts, cu = _clouds(counts, device, 1)

    def f():
        sub, lens = ops.grid_subsample(pts, cu, 0.1)
        return sub, lens, ops.voxel_downsample(pts, 0.1), ops.cell_order(pts, cu, 0.1)
    sub, lens, vox, order = run_three(monkeypatch, f, f"subsampling {counts}")
    assert int(lens.sum()) == sub.shape[0] and 1 <= vox.shape[0] <= pts.shape[0]
    off = 0
    for c in counts:                       # a permutation of every cloud's own points
        assert sorted(order[off:off + c].tolist()) == list(range(off, off + c))
        off += c


@pytest.mark.parametrize("counts", POINT_COUNTS)
def test_radius_searches(device, monkeypatch, counts):
    """Both algorithms of spr_radius_neighbors, the table's build and its three query forms: the same rows."""
    host, pts, cu = _clouds(counts, device, 2)

    def f():
        a0, m0 = ops.radius_neighbors(pts, pts, cu, cu, 0.2, 40, algo=0)
        a1, m1 = ops.radius_neighbors(pts, pts, cu, cu, 0.2, 40, algo=1)
        out = [a0, a1, torch.tensor([m0, m1])]
        for dense in (None, True, False):
            table = ops.RadiusTable(pts, cu, 0.2)
            q, m = table.query(pts, cu, 40, dense=dense)
            out += [q, torch.tensor([m])]
        return out
    out = run_three(monkeypatch, f, f"radius {counts}")
    for q in (out[1], out[3], out[5], out[7]):
        assert torch.equal(out[0], q)
    # brute force, independent of the library: every support of the query's own cloud with d2 below r^2 is in the row,
    # nothing beyond r^2 is, rows ascend in d2 (float64 d2; a band of 1e-5 r^2 around the radius is left to rounding)
    rows, n = out[0].cpu().numpy(), host.shape[0]
    assert int(out[2][0]) <= 40, "a row was cut at the limit: the brute-force comparison needs whole rows"
    cloud = np.repeat(np.arange(len(counts)), counts)
    d2 = ((host[:, None, :].astype(np.float64) - host[None, :, :].astype(np.float64)) ** 2).sum(-1)
    d2[cloud[:, None] != cloud[None, :]] = np.inf
    r2 = 0.2 ** 2
    for i in range(n):
        got = rows[i][rows[i] != n]
        assert len(set(got.tolist())) == len(got) and i in got
        assert set(np.nonzero(d2[i] < r2 * (1 - 1e-5))[0].tolist()) <= set(got.tolist()), i
        assert bool((d2[i][got] <= r2 * (1 + 1e-5)).all()), i
        assert bool((np.diff(d2[i][got]) >= -1e-7).all()), i


def _overlap_inputs(counts, device):
    """Target cloud b = source cloud b, shuffled, with 2 mm of noise: every point has its partner inside the radius."""
    host, src, scu = _clouds(counts, device, 3)
    rng = np.random.default_rng(4)
    tgt, off = [], 0
    for c in counts:
        tgt.append(host[off:off + c][rng.permutation(c)] + rng.normal(0, 0.002, (c, 3)).astype(np.float32))
        off += c
    pose = torch.eye(4)[None, :3].repeat(len(counts), 1, 1).contiguous().to(device)
    return src, scu, T(np.concatenate(tgt).astype(np.float32)).to(device), scu.clone(), pose


def _owned(corr, off, counts):
    """The columns of a [2, W] correspondence tensor that its pairs own, [off[b], off[b] + counts[b]): the rest of the
    tensor is never written (include/spr.h) and holds whatever torch.empty found."""
    return torch.cat([corr[:, o:o + c] for o, c in zip(off, counts)], 1)


@pytest.mark.parametrize("counts", POINT_COUNTS)
def test_gt_overlap_and_augment(device, monkeypatch, counts):
    src, scu, tgt, tcu, pose = _overlap_inputs(counts, device)
    keys = [11, 12, 13]
    off = scu[:-1].cpu().tolist()

    def f():
        s_corr, t_corr, s_mask, t_mask, corr, cnt = ops.gt_overlap(src, scu, tgt, tcu, pose, 0.05)
        psrc, swap, perturb = ops.augment_draw(7, keys, 'small')
        aug = ops.augment_pairs(src, scu, tgt, tcu, pose, psrc, swap, perturb, 'small', 0.005, seed=7, pair_keys=keys,
                                src_mask=s_mask, tgt_mask=t_mask, corr=corr, corr_off=off, corr_count=cnt)
        # the output rows the call owns: the sum of that side's output lengths, and the owned correspondence columns
        n_s, n_t = int(aug['src_cu'][-1]), int(aug['tgt_cu'][-1])
        for k in ('src_xyz', 'src_perm', 'src_mask'):
            aug[k] = aug[k][:n_s]
        for k in ('tgt_xyz', 'tgt_perm', 'tgt_mask'):
            aug[k] = aug[k][:n_t]
        aug['corr'] = _owned(aug['corr'], off, aug['corr_count'].tolist())
        return s_corr, t_corr, s_mask, t_mask, _owned(corr, off, cnt), torch.tensor(cnt), aug
    out = run_three(monkeypatch, f, f"gt_overlap + augment {counts}")
    assert int(out[5].sum()) > 0, "no correspondence at all: the case is vacuous"
    assert not bool(out[6]['status'].any()) and int(out[6]['corr_count'].sum()) > 0


@pytest.mark.parametrize("counts", POINT_COUNTS)
def test_instance_norm(device, monkeypatch, counts):
    n = sum(counts)
    cu = ops.lengths_to_cu(list(counts), device)
    x, add, go = synthetic.rand((n, 64), 201, -5.0, 7.0), synthetic.rand((n, 64), 77), synthetic.rand((n, 64), 78).to(device)

    def f():
        lx, la = x.clone().to(device).requires_grad_(True), add.clone().to(device).requires_grad_(True)
        y = ops.instnorm(lx, cu, add=la, slope=0.1, max_len=max(counts))
        y.backward(go)
        mean, rstd = ops.instnorm_stats(lx.detach(), cu, max_len=max(counts))
        return y, lx.grad, la.grad, mean, rstd, ops.instnorm_raw(lx.detach(), cu)        # max_len defaulted to n
    y, dx, dadd, mean, rstd, plain = run_three(monkeypatch, f, f"instnorm {counts}")
    L = list(counts)
    # forward: test_gpu_forward_range.py::test_instnorm_ragged_every_regime (2e-6 of scale, or 4 x float32's own error)
    _bounded(y, fc.instnorm_f64(x, L, add=add, slope=0.1), fc.instnorm_f32(x, L, add=add, slope=0.1), 2e-6,
             "instnorm+add")
    _bounded(plain, fc.instnorm_f64(x, L), fc.instnorm_f32(x, L), 2e-6, "instnorm")
    # statistics: test_gpu_forward_range.py::test_instnorm_variants_bitwise
    m64, r64 = fc.instnorm_stats_f64(x, L)
    assert float((mean.cpu().double() - m64).abs().max()) <= 2.0 ** -23 * float(m64.abs().max())
    assert float(((rstd.cpu().double() - r64) / r64).abs().max()) <= 2e-6
    # backward: test_gpu_backward.py::test_instnorm_lrelu_add_backward
    cx, ca = x.double().requires_grad_(True), add.double().requires_grad_(True)
    torch.nn.functional.leaky_relu(O.instance_norm(cx, np.asarray(L)) + ca, 0.1).backward(go.cpu().double())
    assert _rel(dx, cx.grad) <= 2e-5 and _rel(dadd, ca.grad) <= 1e-6, (_rel(dx, cx.grad), _rel(dadd, ca.grad))


@pytest.mark.parametrize("form", ["shortcut", "none"])
def test_block_tail(device, monkeypatch, form):
    """The inputs of test_gpu_block_tail.py::test_block_tail_vs_float64_and_separate_operators[SHAPES[0]] and
    ::test_block_tail_without_shortcut_tensor, which hold them against float64."""
    ka, kb, n_out = TAIL_SHAPES[0]
    if form == "shortcut":
        xa, wa, xb, wb, ad, cu = tail_inputs(ka, kb, n_out, TAIL_LENS, device)
    else:
        xa, wa, xb, wb, ad, cu = tail_inputs(32, 0, 128, TAIL_LENS, device, add=False)
    run_three(monkeypatch, lambda: ops.block_tail(xa, wa, cu, xb=xb, wb=wb, add=ad), f"block_tail {form}")


# ---- KPConv ------------------------------------------------------------------------------------------------------------
def _kp_inputs(tag, device):
    gold, inp = load_golden("ops.npz"), ops_inputs()
    pts = T(inp["kp.pts"]).to(device)
    nb = T(gold["kp.nb"].astype(np.int32)).to(device)
    return pts, nb, inp[f"kp.{tag}.x"].to(device), inp[f"kp.{tag}.w"].to(device), T(gold[f"kp.{tag}.kpts"]).to(device), \
        inp["kp.extent"], gold[f"kp.{tag}.y"]


@pytest.mark.parametrize("cached", [False, True])
@pytest.mark.parametrize("impl", [0, 1])
@pytest.mark.parametrize("tag", ["c32", "c64", "c128"])
def test_kpconv_forward(device, monkeypatch, tag, impl, cached):
    """cached: the tile plan and the weight planes ride on the index / weight tensors from the production run on;
    otherwise every run gets fresh tensors and builds both.  The inputs of test_gpu_ops.py::test_kpconv_vs_reference,
    which holds these shapes; the same bound is asserted here."""
    pts, nb, x, w, kp, ext, gold_y = _kp_inputs(tag, device)

    def f():
        nbr, wt = (nb, w) if cached else (nb.clone(), w.clone())
        return ops.kpconv_raw(pts, pts, nbr, x, wt, kp, ext, rows_sorted=True, impl=impl)
    y = run_three(monkeypatch, f, f"kpconv {tag} impl {impl} cached {cached}")
    _close(y.cpu().numpy(), gold_y, 1e-5, f"kpconv {tag} impl {impl}")


@pytest.mark.parametrize("tag", ["c1", "c32", "c64", "c128"])
def test_kpconv_backward(device, monkeypatch, tag):
    """Weighted features, the dx scatter, dW (c1: the float64 product)."""
    pts, nb, x, w, kp, ext, y = _kp_inputs(tag, device)
    go = synthetic.rand((600, w.shape[2]), 90).to(device)

    def f():
        lx, lw = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        out = ops.kpconv(pts, pts, nb, lx, lw, kp, ext, rows_sorted=True)
        out.backward(go)
        return out, lx.grad, lw.grad
    _, dx, dw = run_three(monkeypatch, f, f"kpconv backward {tag}")
    # test_gpu_backward.py::test_kpconv_backward (same inputs for c32, c64, c128; c1 is new): 2e-5 per gradient
    cx, cw = x.cpu().double().requires_grad_(True), w.cpu().double().requires_grad_(True)
    O.kpconv(pts.cpu().double(), pts.cpu().double(), nb.cpu().long(), cx, cw, kp.cpu().double(),
             float(ext)).backward(go.cpu().double())
    assert _rel(dx, cx.grad) <= 2e-5, f"kpconv {tag} dx {_rel(dx, cx.grad):.2e}"
    assert _rel(dw, cw.grad) <= 2e-5, f"kpconv {tag} dW {_rel(dw, cw.grad):.2e}"


def test_maxpool_and_gather_backward(device, monkeypatch):
    """The inputs of test_gpu_backward.py::test_maxpool_and_gather_backward, which holds them against float64."""
    gold, inp = load_golden("ops.npz"), ops_inputs()
    idx = T(gold["mp.idx"].astype(np.int32)).to(device)
    x, go = inp["in.x"], synthetic.rand((idx.shape[0], 64), 80).to(device)
    sel = torch.tensor([5, 0, 5, 599, 17], dtype=torch.int32, device=device)

    def f():
        a, b = x.clone().to(device).requires_grad_(True), x.clone().to(device).requires_grad_(True)
        ops.maxpool(a, idx).backward(go)
        ops.gather_rows(b, sel).backward(go[:5])
        return a.grad, b.grad
    run_three(monkeypatch, f, "maxpool / gather_rows backward")


# ---- matching head, Sinkhorn, refinement ---------------------------------------------------------------------------------
MATCH_PAIRS = [(1, 1), (63, 65), (129, 200)]


def _match_inputs(device):
    lens = [n for n, _ in MATCH_PAIRS] + [m for _, m in MATCH_PAIRS]
    cu_host = [0] + [int(c) for c in np.cumsum(lens)]
    feat = synthetic.rand((cu_host[-1], 256), 260, -0.9, 0.9)
    xyz = synthetic.rand((cu_host[-1], 3), 262, -1.0, 1.0)
    return feat, xyz, torch.tensor(cu_host, dtype=torch.int32, device=device), cu_host


def _per_pair(t, cu_host):
    """(source rows, target rows) of every pair of a packed [T, .] tensor."""
    B = len(MATCH_PAIRS)
    return [t[cu_host[k]:cu_host[k + 1]] for k in range(B)], [t[cu_host[B + k]:cu_host[B + k + 1]] for k in range(B)]


@pytest.mark.parametrize("n_iters", [0, 3])
def test_matching_head(device, monkeypatch, n_iters):
    feat, xyz_h, cu, cu_host = _match_inputs(device)
    B = len(MATCH_PAIRS)
    dfeat, xyz = feat.to(device), xyz_h.to(device)

    def f():
        val, ind = ops.match_dualsoftmax_raw(dfeat, cu, cu_host, B)
        top2 = ops.match_dualsoftmax_top2(dfeat, cu, cu_host, B)
        w, that = ops.sinkhorn_correspondences_raw(dfeat, xyz, cu, cu_host, B, 0.9, 1.1, n_iters)
        both = ops.match_and_sinkhorn(dfeat, xyz, cu, cu_host, B, 0.9, 1.1, n_iters, top2=True)
        return val, ind, top2, w, that, both
    val, ind, top2, w, that, both = run_three(monkeypatch, f, f"matching head n_iters={n_iters}")
    assert torch.equal(val, both[0]) and torch.equal(ind, both[2]) and torch.equal(w, both[3]) and torch.equal(that, both[4])
    assert torch.equal(top2[0], val) and torch.equal(top2[1], both[1])
    # float64, with the per-element bounds of test_gpu_match_range.py (test_dual_softmax_every_path,
    # test_sinkhorn_parameter_grid)
    (fs, ft), (_, xt) = _per_pair(feat, cu_host), _per_pair(xyz_h, cu_host)
    _check_dual_softmax("workspace", fs, ft, [_ds_ref(a, b) for a, b in zip(fs, ft)], top2[0], top2[1], top2[2],
                        f"dual softmax n_iters={n_iters}")
    _check_sinkhorn(fs, ft, xt, w, that, 0.9, 1.1, n_iters, f"sinkhorn n_iters={n_iters}")


@pytest.mark.parametrize("n_iters", [0, 3])
def test_sinkhorn_backward(device, monkeypatch, n_iters):
    feat, xyz_h, cu, cu_host = _match_inputs(device)
    xyz = xyz_h.to(device)
    B, tsrc = len(MATCH_PAIRS), cu_host[len(MATCH_PAIRS)]
    gw, gt = synthetic.rand((tsrc,), 13).to(device), synthetic.rand((tsrc, 3), 14).to(device)

    def f():
        lf = feat.clone().to(device).requires_grad_(True)
        al = torch.tensor(0.9, device=device, requires_grad=True)
        be = torch.tensor(1.1, device=device, requires_grad=True)
        w, that = ops.sinkhorn_correspondences(lf, xyz, cu, cu_host, B, al, be, n_iters)
        ((w * gw).sum() + (that * gt).sum()).backward()
        return w, that, lf.grad, al.grad, be.grad
    _, _, dfeat, dal, dbe = run_three(monkeypatch, f, f"sinkhorn backward n_iters={n_iters}")
    # float64 autograd of the potential form; the bounds of
    # test_gpu_match_range.py::test_sinkhorn_backward_double_potentials
    cf = feat.double().requires_grad_(True)
    ca = torch.tensor(0.9, dtype=torch.float64, requires_grad=True)
    cb = torch.tensor(1.1, dtype=torch.float64, requires_grad=True)
    (_, xt), loss, affs = _per_pair(xyz_h, cu_host), 0.0, []
    for k in range(B):
        a_, b_ = cf[cu_host[k]:cu_host[k + 1]], cf[cu_host[B + k]:cu_host[B + k + 1]]
        aff = -(torch.clamp(a_ @ b_.t() / 16.0, min=0.0) - torch.nn.functional.softplus(ca)) / (cb.exp() + 0.02)
        aff.retain_grad()
        affs.append(aff)
        u_ = torch.zeros(aff.shape[0], dtype=torch.float64)
        v_ = torch.zeros(aff.shape[1], dtype=torch.float64)
        for _ in range(n_iters):
            u_ = torch.log1p(torch.exp(aff - v_[None, :]).sum(1))
            v_ = torch.log1p(torch.exp(aff - u_[:, None]).sum(0))
        P = torch.exp(aff - u_[:, None] - v_[None, :])
        wr = P.sum(1)
        tr = P @ xt[k].double() / (wr[:, None] + 1e-6)
        sl = slice(cu_host[k], cu_host[k + 1])
        loss = loss + (wr * gw.cpu()[sl].double()).sum() + (tr * gt.cpu()[sl].double()).sum()
    loss.backward()
    assert _rel(dfeat, cf.grad) <= 5e-5, f"sinkhorn dfeat {_rel(dfeat, cf.grad):.2e}"
    den, sig = math.exp(1.1) + 0.02, 1.0 / (1.0 + math.exp(-0.9))
    mag_a = sum(float(a.grad.abs().sum()) for a in affs) * sig / den
    mag_b = sum(float((a.grad * a.detach()).abs().sum()) for a in affs) * math.exp(1.1) / den
    for got, ref, mag, nm in ((dal, ca.grad, mag_a, "alpha"), (dbe, cb.grad, mag_b, "beta")):
        err = abs(float(got) - float(ref))
        assert err <= max(5e-5 * abs(float(ref)), 16 * U * mag), f"sinkhorn d{nm}: {float(got):.9e} vs {float(ref):.9e}"


@pytest.mark.parametrize("n", [4097, 100])
def test_refine_pairs(device, monkeypatch, n):
    """4 097 entries: the first size that asks for a workspace; 100: none is asked for (and none is handed out)."""
    rng = np.random.default_rng(17)
    P = refine_pack([synth_pair(rng, n, n + 11)], device)
    need = _lib.lib().spr_refine_pairs_workspace_bytes(1, n)
    assert (need > 0) == (n > 4096)

    def f():
        return ops.refine_pairs(P['val'], P['val2'], P['ind'], P['ov'], P['xyz'], P['cu'], P['cu_host'], 1, None, ratio=True,
                                median=True, overlap_prune=True, lgr_steps=2, lowe_thres=0.9, acceptance_radius=0.3)
    if need:
        out = run_three(monkeypatch, f, f"refine_pairs n={n}")
    else:       # ops.refine_pairs asks for nothing when the query answers 0: the arena must not be called at all
        arena = Arena(0xFF)
        with monkeypatch.context() as m:
            m.setattr(ops, "_workspace", arena)
            out = f()
        assert arena.calls == 0
    assert not bool(out['status'].any()) and bool(torch.isfinite(out['pose']).all())


# ---- losses ------------------------------------------------------------------------------------------------------------
def test_loss_kernels(device, monkeypatch):
    """The four _loss_ws users: BCE, InfoNCE forward and backward, the transform L1."""
    inp = ops_inputs()
    fs, ft, xs, xt = inp["sk.fs"], inp["sk.ft"], (inp["sk.xs"] * 0.3).to(device), (inp["sk.xt"] * 0.3).to(device)
    W = synthetic.rand((256, 256), 16, -0.05, 0.05)
    pose = torch.tensor([[1.0, 0, 0, 0.02], [0, 1, 0, -0.01], [0, 0, 1, 0.0]]).to(device)
    x, y = synthetic.rand((500,), 17, 0.01, 0.99), (synthetic.rand((500,), 18) > 0).float().to(device)
    pp = (pose.cpu() + 0.05 * synthetic.rand((3, 4), 19))

    def f():
        la, lp, lw = (t.clone().to(device).requires_grad_(True) for t in (fs, ft, W))
        nce = ops.infonce_pair(la, lp, xs, pose, xt, lw, 0.2, 0.4)
        nce.backward()
        lx = x.clone().to(device).requires_grad_(True)
        bce = ops.bce_logits_mean(lx, y)
        bce.backward()
        lpp = pp.clone().to(device).requires_grad_(True)
        l1 = ops.transform_l1_pair(pose, lpp, xs)
        l1.backward()
        return nce, la.grad, lp.grad, lw.grad, bce, lx.grad, l1, lpp.grad
    nce, _, _, _, bce, _, l1, _ = run_three(monkeypatch, f, "loss kernels")
    # the gradients: exactly the inputs of test_gpu_backward.py::test_loss_kernels_backward, held against float64 there.
    # The three values, with the bounds of test_gpu_match_range.py (_infonce_check, test_bce_logits_mean_edges,
    # test_transform_l1_far_coordinates):
    xs64, xt64, p64 = xs.cpu().double(), xt.cpu().double(), pose.cpu().double()
    ref = float(_infonce64(fs.double(), ft.double(), O.se3_transform(p64, xs64), xt64, W.double(), 0.2, 0.4))
    Ws = torch.triu(W.double()) + torch.triu(W.double()).t()
    mag = float((fs.double().abs() @ Ws.abs() @ ft.double().abs().t()).max())
    allow = 2 * (2 * _coef(256) * mag) + 8 * U * (abs(ref) + 1) + (60 / 16 + 40) * U
    assert abs(float(nce) - ref) <= allow, f"infonce {float(nce):.9e} vs {ref:.9e} (allow {allow:.2e})"
    ref = float(torch.nn.functional.binary_cross_entropy_with_logits(x.double(), y.cpu().double()))
    assert abs(float(bce) - ref) <= 4 * U * float((x.abs().double() + 1).mean()) + 1e-12 + 2 * U * abs(ref)
    ref = float((O.se3_transform(p64, xs64) - O.se3_transform(pp.double(), xs64)).abs().mean())
    mag = float((xs64.abs() @ p64[:, :3].abs().t() + p64[:, 3].abs()).mean())
    assert abs(float(l1) - ref) <= 2 * 5 * U * mag + 2 * U * ref, f"transform_l1 {float(l1):.9e} vs {ref:.9e}"


def test_circle_loss(device, monkeypatch):
    """The `ragged` case of test_gpu_circle_loss.py (same seed), held against float64 there:
    test_forward_matches_float64 and test_input_gradients_match_float64."""
    fs, ft, xs, xt = circle_case(seed=sorted(CIRCLE_REGIMES).index("ragged") + 1, **CIRCLE_REGIMES["ragged"])
    run_three(monkeypatch, lambda: circle_run(device, fs, ft, xs, xt, grad=True), "circle loss forward + backward")


# ---- whole model: bytes expected to survive between calls, nested use of the buffer ----------------------------------------
def _train_step(device, pos_emb_type):
    B = 2
    cfg = get_config("3dmatch") if pos_emb_type == "sine" else get_config("3dmatch", pos_emb_type=pos_emb_type)
    pairs, sizes = pairs_for("3dmatch", B)
    pose, src_ov, tgt_ov = loss_inputs("3dmatch", B)
    model = RegTR(cfg)
    synthetic.fill_parameters(model, seed=0)
    model = model.to(device).train()
    batch = {"src_xyz": [T(p[0][:n]).to(device) for p, (n, m) in zip(pairs, sizes)],
             "tgt_xyz": [T(p[1][:m]).to(device) for p, (n, m) in zip(pairs, sizes)],
             "pose": T(pose).to(device),
             "src_overlap": [T(o).to(device) for o in src_ov], "tgt_overlap": [T(o).to(device) for o in tgt_ov]}
    out = model(batch)
    losses = model.compute_loss(out, batch)
    model.zero_grad(set_to_none=True)
    losses["total"].backward()
    keep = {k: out[k] for k in ("pose", "src_feat", "tgt_feat", "src_overlap", "tgt_overlap") if k in out}
    assert "pose" in keep and "src_feat" in keep and "src_overlap" in keep
    grads = [p.grad for _, p in model.named_parameters() if p.grad is not None]
    assert len(grads) > 100
    return keep, {k: v for k, v in losses.items()}, grads


@pytest.mark.parametrize("pos_emb_type", ["sine", "learned"])
def test_whole_training_step(device, monkeypatch, pos_emb_type):
    run_three(monkeypatch, lambda: _train_step(device, pos_emb_type), f"training step ({pos_emb_type})", guard=1 << 16,
              verify_every=256)


def test_whole_inference_forward(device, monkeypatch):
    """eval(): the fused cross-encoder stack, the fused block tails and the one-call matching head."""
    pairs, sizes = pairs_for("3dmatch", 2)
    model = RegTR(get_config("3dmatch"))
    synthetic.fill_parameters(model, seed=0)
    model = model.to(device).eval()
    batch = {"src_xyz": [T(p[0][:n]).to(device) for p, (n, m) in zip(pairs, sizes)],
             "tgt_xyz": [T(p[1][:m]).to(device) for p, (n, m) in zip(pairs, sizes)]}

    def f():
        with torch.no_grad():
            out = model(dict(batch))
        return {k: out[k] for k in ("pose", "src_feat", "tgt_feat", "src_overlap", "tgt_overlap") if k in out}
    run_three(monkeypatch, f, "inference forward", guard=1 << 16, verify_every=256)


# ---- operators of the other host modules: decoder.py, stem.py, kpconv_modes.py, modelnet.py, tie_order.py --------------
# Each builder returns (f, check): f(put) builds its inputs anew, passes every device operand through put and runs the
# operator; check(production) applies the criterion of the test it names.  tests/test_gpu_tensor_bounds.py runs the
# same builders with placed inputs.  (The test modules that import this one are imported inside the builders.)
def decoder_case(device):
    """decoder.upsample_unary, fused route: the widest-tail shape of
    test_gpu_decoder.py::test_fused_call_inside_its_tensors_and_workspace (two whole tiles + 3 rows, shadow and negative
    indices), under the float64 bound of ::test_upsample_unary_against_float64."""
    import test_gpu_decoder as D
    from superpoints_registration_amd import decoder
    kc, ks, n_out, n, nc = 64, 32, 64, 2 * D.TILE + 3, 5
    xc, xs = synthetic.rand((nc, kc), 71, -3.0, 3.0), synthetic.rand((n, ks), 72, -3.0, 3.0)
    w = synthetic.rand((n_out, kc + ks), 73, -0.2, 0.2)
    idx = D._indices("shadow", n, nc)

    def f(put):
        ins = [put(t) for t in (xc.to(device), xs.to(device), D._matrix(idx, 1, device), w.to(device))]
        return decoder.upsample_unary(*ins, route="fused")

    def check(y):
        D._check(y, D._ref64(xc, xs, idx, w), 2e-6 * max(1, (kc + ks) // 256), "upsample_unary")
    return f, check


def stem_case(device):
    """stem.kpconv_stem on the ragged batch of test_gpu_stem.py (cout 64, random features), statistics included: the
    bits of that module's production call (::test_stem_inside_exactly_its_workspace's criterion); the float64 check
    of these shapes is tests/test_gpu_stem_range.py."""
    import test_gpu_stem as S
    from superpoints_registration_amd import stem
    d = S._stem_case(device, 64, "random")

    def f(put):
        q, s, nb, x, w, kp, cu = (put(d[k].clone()) for k in ("q", "s", "nb", "x", "w", "kp", "cu"))
        return stem.kpconv_stem(q, s, nb, x, w, kp, S.EXT, cu, slope=0.1, rows_sorted=True, max_len=d["ml"],
                                return_stats=True)

    def check(out):
        for got, want in zip(out, (d["out"], d["smean"], d["srstd"])):
            assert torch.equal(_bits(got), _bits(want))
    return f, check


def kpconv_modes_case(device, name, mode):
    """kpconv_modes forward, weighted features and d x (KPConvModesFn) on a case of tests/test_gpu_kpconv_modes.py,
    under ::test_backward_matches_float64_autograd's bounds."""
    import test_gpu_kpconv_modes as M
    case = M.case_of(name)
    go, ref, dx_ref, dw_ref = M.ref_of(name, mode)

    def f(put):
        d = M.on_device(case, device, put)
        x, w = d["x"].requires_grad_(True), d["w"].requires_grad_(True)
        out = M.run_forward(dict(d, x=x, w=w), mode)
        out.backward(put(go.clone().to(device)))
        return out.detach(), x.grad, w.grad

    def check(res):
        out, dx, dw = res
        assert M.scale_err(out, ref) <= 1e-5 and _rel(dx, dx_ref) <= 2e-5 and _rel(dw, dw_ref) <= 2e-5
    return f, check


MODES_CASES = [("tile strided nq37 ns130 k33 32-64", ('gaussian', 'closest')), ("tile nq37 k5 64-64", ('constant', 'sum')),
               ("simple 48-40", ('linear', 'closest'))]


def modelnet_case(device):
    """modelnet.modelnet_draw (device form) and modelnet.modelnet_pairs with inline and with explicit draws, the batch
    of test_gpu_modelnet_pairs.py::test_every_tensor_and_the_workspace_between_poisoned_guard_bands; the two forms
    agree in every bit (::test_inline_draws_equal_explicit_buffers_and_the_numpy_philox)."""
    import test_gpu_modelnet_pairs as MP
    from superpoints_registration_amd import modelnet
    seed, keys, lens, k = 77, [5, 6, 7], [700, 2048, 333], 717
    xyz = T(np.concatenate([MP.shape_cloud(n, 20 + b) for b, n in enumerate(lens)])).to(device)

    def owned(r):
        cnt = r["corr_count"].tolist()                 # columns past a pair's count are not written (include/spr.h)
        cols = torch.cat([torch.arange(i * k, i * k + c) for i, c in enumerate(cnt)]).to(r["corr"].device)
        return dict(r, corr=r["corr"][:, cols])

    def f(put):
        pts, cu = put(xyz.clone()), put(ops.lengths_to_cu(lens, device))
        dirs, tf, rk, ex, nz, sk = modelnet.modelnet_draw(seed, keys, 45.0, 0.5, cu, sum(lens), k)
        tf_d, dirs_d = put(T(tf).to(device)), put(T(dirs).to(device))
        inline = modelnet.modelnet_pairs(pts, cu, max(lens), MP.P07, k, tf_d, dirs_d, seed=seed, pair_keys=keys)
        explicit = modelnet.modelnet_pairs(pts, cu, max(lens), MP.P07, k, tf_d, dirs_d, rkeys=rk, extra=ex, noise=nz, skeys=sk)
        return owned(inline), owned(explicit), rk, ex, nz, sk

    def check(res):
        inline, explicit = res[0], res[1]
        assert not bool(inline["status"].any()) and int(inline["corr_count"].sum()) > 0
        for key in inline:
            assert torch.equal(_bits(inline[key]), _bits(explicit[key])), f"inline and explicit draws differ in {key}"
    return f, check


def tie_order_case(device, name, limit):
    """ops.radius_neighbors(tie_order='reference'): the kd-tree replay and spr_tie_order on a case of
    test_gpu_tie_order.py::test_radius_neighbors_gives_the_reference_rows, held against the reference's rows."""
    import tie_order_cases as tc
    c, gold = tc.cases()[name], tc.load_golden()
    sup, qry = T(np.array(c.sup)).to(device), T(np.array(c.qry)).to(device)

    def f(put):
        s, scu = put(sup.clone()), put(ops.lengths_to_cu(list(c.s_lens), device))
        q, qcu = (s, scu) if c.qry is c.sup else (put(qry.clone()), put(ops.lengths_to_cu(list(c.q_lens), device)))
        rows, mc = ops.radius_neighbors(q, s, qcu, scu, c.radius, limit, tie_order='reference')
        return rows, torch.tensor([mc])

    def check(res):
        assert np.array_equal(res[0].cpu().numpy(), tc.reference_rows(gold, name, limit))
    return f, check


def _unplaced(f):
    return lambda: f(lambda t: t)


def test_decoder_upsample_unary(device, monkeypatch):
    f, check = decoder_case(device)
    check(run_three(monkeypatch, _unplaced(f), "upsample_unary"))


def test_kpconv_stem(device, monkeypatch):
    f, check = stem_case(device)
    check(run_three(monkeypatch, _unplaced(f), "kpconv_stem"))


@pytest.mark.parametrize("name,mode", MODES_CASES, ids=lambda v: v if isinstance(v, str) else "-".join(v))
def test_kpconv_modes(device, monkeypatch, name, mode):
    f, check = kpconv_modes_case(device, name, mode)
    check(run_three(monkeypatch, _unplaced(f), f"kpconv_modes {name} {mode}"))


def test_modelnet_pairs(device, monkeypatch):
    f, check = modelnet_case(device)
    check(run_three(monkeypatch, _unplaced(f), "modelnet_pairs"))


@pytest.mark.parametrize("name,limit", [("batch3", 17), ("n1", 5)])
def test_tie_order(device, monkeypatch, name, limit):
    f, check = tie_order_case(device, name, limit)
    check(run_three(monkeypatch, _unplaced(f), f"tie order {name}"))


# ---- one byte short is refused -------------------------------------------------------------------------------------------
class _OneByteShort(Arena):
    """Hands out [GUARD, GUARD + nbytes - 1): the guards still stand around the nbytes the caller asked for."""

    def __call__(self, nbytes, device):
        view = super().__call__(nbytes, device)
        return view[:-1] if nbytes > 0 else view


# Operators that by contract do not refuse a workspace below their full size query (a fixed list).
# spr_attn_varlen_bwd: below spr_attn_bwd_workspace_bytes it runs without the operand planes, down to
# spr_attn_bwd_min_workspace_bytes: the result must be production's, bit for bit.
FALLS_BACK = ("attention backward",)


def _one_byte_short(monkeypatch, what, prepare, run):
    """prepare() builds fresh inputs with production's workspace (a forward whose backward is the case, say); run(state)
    is the one operator call under test.  Refused: RuntimeError naming the workspace, nothing written to the buffer
    (the refusal comes before the first launch or memset), guards intact, and production unchanged afterwards."""
    production = _flat(run(prepare()))
    state = prepare()
    arena = _OneByteShort(0xFF)
    with monkeypatch.context() as m:
        m.setattr(ops, "_workspace", arena)
        if what in FALLS_BACK:
            got = _flat(run(state))
        else:
            with pytest.raises(RuntimeError, match="workspace"):
                run(state)
            got = None
    assert arena.calls >= 1 and all(n > 0 for _, n, _ in arena.records), f"{what}: no workspace was asked for"
    torch.cuda.synchronize()
    if got is None:
        for _, n, buf in arena.records:
            assert bool((buf[arena.guard:arena.guard + n] == 0xFF).all()), f"{what}: the refused call wrote to its workspace"
    arena.verify()
    for label, other in (("with a workspace one byte short", got), ("after the refusal", _flat(run(prepare())))):
        if other is not None:
            assert len(other) == len(production) > 0, what
            for i, (p, r) in enumerate(zip(production, other)):
                assert torch.equal(_bits(p), _bits(r)), f"{what}: output {i} {label} differs from production"


def test_one_byte_short_is_refused(device, monkeypatch):
    """One smallest-shape case per layout style, each handed its size query minus one byte."""
    cases = []

    def case(what, run, prepare=lambda: None):
        cases.append((what, prepare, run))

    # token operators, SEGS["one"]
    lens, cu, s_self, s_cross, kv_cross, mx, qkv = _tokens("one", device, 9)
    d = qkv.to(device)
    q, k, v = d[:, :256].contiguous(), d[:, 256:512].contiguous(), d[:, 512:].contiguous()
    w_in, b_in = synthetic.rand((768, 256), 33, -0.1, 0.1).to(device), synthetic.rand((768,), 34, -0.2, 0.2).to(device)
    dgo = synthetic.rand((sum(lens), 256), 44).to(device)
    case("attention", lambda _: ops.attention_raw(q, k, v, cu, s_cross, mx, 8, want_lse=True))
    case("attention with in-projection", lambda _: ops.attention_inproj(q, q, w_in, b_in, cu, s_cross, mx, 8))
    case("attention_probs", lambda _: ops.attention_probs(q, k, cu, s_cross, mx, 8))
    case("attention backward", lambda fwd: ops.attention_bwd(q, k, v, fwd[0], dgo, cu, kv_cross, mx, 8, lse=fwd[1]),
         lambda: ops.attention_raw(q, k, v, cu, s_cross, mx, 8, want_lse=True))
    enc = _encoder(device, 1, 1024, True)
    pos = synthetic.rand((sum(lens), 256), 45).to(device)
    with torch.no_grad():
        enc.forward_packed(q, cu, s_self, s_cross, mx, pos=pos, pos_bound=1.0)
    plan = enc._spr_xenc
    case("xenc_forward", lambda _: ops.xenc_forward(plan, q, pos, cu, s_self, s_cross, mx))

    # products
    x, w = synthetic.rand((1, 256), 1, -3.0, 3.0).to(device), synthetic.rand((256, 256), 2, -0.2, 0.2).to(device)
    case("linear", lambda _: ops.linear_raw(x, w))

    # point operators, POINT_COUNTS[0]
    counts = POINT_COUNTS[0]
    _, pts, pcu = _clouds(counts, device, 2)
    case("grid_subsample", lambda _: ops.grid_subsample(pts, pcu, 0.1))
    for algo in (0, 1):            # 1: the path ops.radius_neighbors falls back to when the cell table overflows
        case(f"radius_neighbors algo {algo}", lambda _, algo=algo: ops.radius_neighbors(pts, pts, pcu, pcu, 0.2, 40, algo=algo))
    src, scu, tgt, tcu, pose = _overlap_inputs(counts, device)
    keys, off = [11, 12, 13], scu[:-1].cpu().tolist()

    def overlap(_):
        out = ops.gt_overlap(src, scu, tgt, tcu, pose, 0.05)
        return out[:4], _owned(out[4], off, out[5]), torch.tensor(out[5])
    case("gt_overlap", overlap)
    _, _, s_mask, t_mask, corr, cnt = ops.gt_overlap(src, scu, tgt, tcu, pose, 0.05)
    psrc, swap, perturb = ops.augment_draw(7, keys, 'small')

    def augment(_):
        aug = ops.augment_pairs(src, scu, tgt, tcu, pose, psrc, swap, perturb, 'small', 0.005, seed=7, pair_keys=keys,
                                src_mask=s_mask, tgt_mask=t_mask, corr=corr, corr_off=off, corr_count=cnt)
        return aug['src_cu'], aug['tgt_cu'], aug['pose'], aug['status'], aug['corr_count']
    case("augment_pairs", augment)
    n = sum(counts)
    xin = synthetic.rand((n, 64), 201, -5.0, 7.0).to(device)
    case("instnorm", lambda _: ops.instnorm_raw(xin, pcu, max_len=max(counts)))
    ka, kb, n_out = TAIL_SHAPES[0]
    xa, wa, xb, wb, ad, tcu_ = tail_inputs(ka, kb, n_out, TAIL_LENS, device)
    case("block_tail", lambda _: ops.block_tail(xa, wa, tcu_, xb=xb, wb=wb, add=ad))
    kpts, nb_, kx, kw, kp, ext, _ = _kp_inputs("c32", device)
    case("kpconv", lambda _: ops.kpconv_raw(kpts, kpts, nb_.clone(), kx, kw.clone(), kp, ext, rows_sorted=True, impl=0))

    # matching head, Sinkhorn backward, refinement
    feat, xyz_h, mcu, cu_host = _match_inputs(device)
    B, tsrc = len(MATCH_PAIRS), cu_host[len(MATCH_PAIRS)]
    dfeat, xyz = feat.to(device), xyz_h.to(device)
    case("match_and_sinkhorn", lambda _: ops.match_and_sinkhorn(dfeat, xyz, mcu, cu_host, B, 0.9, 1.1, 3, top2=True))
    gw, gt = synthetic.rand((tsrc,), 13).to(device), synthetic.rand((tsrc, 3), 14).to(device)

    def sinkhorn_forward():
        lf = feat.clone().to(device).requires_grad_(True)
        al = torch.tensor(0.9, device=device, requires_grad=True)
        be = torch.tensor(1.1, device=device, requires_grad=True)
        w_, that = ops.sinkhorn_correspondences(lf, xyz, mcu, cu_host, B, al, be, 3)
        return (w_ * gw).sum() + (that * gt).sum(), (lf, al, be)

    def backward(state):
        loss, leaves = state
        loss.backward()
        return [t.grad for t in leaves]
    case("sinkhorn backward", backward, sinkhorn_forward)
    rng = np.random.default_rng(17)
    P = refine_pack([synth_pair(rng, 4097, 4108)], device)
    case("refine_pairs", lambda _: ops.refine_pairs(P['val'], P['val2'], P['ind'], P['ov'], P['xyz'], P['cu'], P['cu_host'], 1,
                                                    None, ratio=True, median=True, overlap_prune=True, lgr_steps=2,
                                                    lowe_thres=0.9, acceptance_radius=0.3))

    # losses
    inp = ops_inputs()
    fs, ft, xs, xt = inp["sk.fs"], inp["sk.ft"], (inp["sk.xs"] * 0.3).to(device), (inp["sk.xt"] * 0.3).to(device)
    W = synthetic.rand((256, 256), 16, -0.05, 0.05)
    lpose = torch.tensor([[1.0, 0, 0, 0.02], [0, 1, 0, -0.01], [0, 0, 1, 0.0]]).to(device)

    def infonce_forward():
        leaves = tuple(t.clone().to(device).requires_grad_(True) for t in (fs, ft, W))
        return ops.infonce_pair(leaves[0], leaves[1], xs, lpose, xt, leaves[2], 0.2, 0.4), leaves
    case("infonce_pair", lambda _: infonce_forward()[0].detach())
    case("infonce_pair backward", backward, infonce_forward)
    cfs, cft, cxs, cxt = circle_case(seed=sorted(CIRCLE_REGIMES).index("ragged") + 1, **CIRCLE_REGIMES["ragged"])
    case("circle_loss", lambda _: circle_run(device, cfs, cft, cxs, cxt)[0])

    # the other host modules: one case per workspace layout (the builders above, inputs as they come)
    for what, builder in (("upsample_unary", decoder_case), ("kpconv_stem", stem_case), ("modelnet_pairs", modelnet_case)):
        case(what, lambda _, f=builder(device)[0]: f(lambda t: t))
    import test_gpu_kpconv_modes as M
    md = M.on_device(M.case_of("simple 48-40"), device)
    case("kpconv_modes forward", lambda _: M.run_forward(md, ('gaussian', 'closest')))
    # the two backward sites of kpconv_modes.py, as test_gpu_kpconv_modes.py::test_one_byte_short_is_refused calls them
    from superpoints_registration_amd import kpconv_modes, tie_order
    infl, agg = kpconv_modes.mode_codes('gaussian', 'closest')
    dwf = synthetic.rand((md["q"].shape[0], md["kp"].shape[0] * md["x"].shape[1]), 5).to(device)
    case("kpconv_modes weighted features", lambda _: kpconv_modes.weighted_features(md["q"], md["s"], md["idx"], md["x"], md["kp"],
                                                                                     md["extent"], infl, agg))
    case("kpconv_modes bwd_dx", lambda _: kpconv_modes.bwd_dx(md["q"], md["s"], md["idx"], md["x"].shape[1], md["kp"],
                                                              md["extent"], infl, agg, dwf))
    # the tie-order fix-up alone (ops.radius_neighbors would ask for the search's workspace first): the nearest-rule
    # rows of tie_order_cases' "batch3", built anew per run since the fix-up rewrites them in place
    import tie_order_cases as tc
    c = tc.cases()["batch3"]
    sup, scu = T(np.array(c.sup)).to(device), ops.lengths_to_cu(list(c.s_lens), device)
    tree = tie_order.ReplayTree(sup, scu)

    def tie_rows():
        rows, mc = ops.radius_neighbors(sup, sup, scu, scu, c.radius, 17)
        return rows, mc

    def tie_fix(state):
        rows, mc = state
        tree.apply(rows, sup, scu, c.radius, mc)
        return rows
    case("tie_order", tie_fix, tie_rows)

    assert set(FALLS_BACK) <= {c[0] for c in cases}
    for what, prepare, run in cases:
        _one_byte_short(monkeypatch, what, prepare, run)


# ---- coverage: keep this test last ---------------------------------------------------------------------------------------
# call sites that no case can reach at small size, with the reason (none so far)
EXCLUDED = {}


def test_every_workspace_call_site_was_reached(device):
    """Every module of the package is scanned (all but _lib.py, the binding itself): a `_workspace(` / `_loss_ws(` call
    site in any of them fails this test until a case above reaches it."""
    pkg = os.path.dirname(ops.__file__)
    sites = []
    names = sorted(n for n in os.listdir(pkg) if n.endswith(".py") and n != "_lib.py")
    assert {"ops.py", "autograd.py", "decoder.py", "stem.py", "kpconv_modes.py", "modelnet.py", "tie_order.py"} <= set(names)
    for name in names:
        for no, line in enumerate(open(os.path.join(pkg, name)).read().splitlines(), 1):
            if re.search(r"_workspace\(|_loss_ws\(", line) and not re.match(r"\s*def (_workspace|_loss_ws)\(", line):
                sites.append((name, no))
    assert len(sites) >= 45, len(sites)
    missing = [s for s in sites if s not in SEEN and s not in EXCLUDED]
    assert not missing, f"no case of this module reached {missing}"
