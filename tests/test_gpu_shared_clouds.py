"""GPU: training over shared clouds (shared_clouds.py) -- the two operators (spr_pair_gather_bwd, spr_overlap_pool_pairs)
bit for bit against their CPU restatements and between poisoned guard bands; RegTR.forward / compute_loss on a batch of
clouds and pairs against the forward on the expanded pair lists and against the reference's gradients; the Trainer."""
import copy
import math

import numpy as np
import pytest
import torch

import test_gpu_backward as tgb
import test_gpu_encode_once as teo
from conftest import load_golden
from oracle.gen_golden import grad_sample_indices, loss_inputs, pairs_for
from superpoints_registration_amd import get_config, ops, overlap, shared_clouds, synthetic
from superpoints_registration_amd.regtr import RegTR
from superpoints_registration_amd.training import Trainer
from tensor_arena import TensorArena
from test_shared_clouds_host import GATHER_PAIRS, LENS
from workspace_arena import GUARD

pytestmark = pytest.mark.gpu
T = torch.from_numpy
U = 2.0 ** -24
F64 = torch.float64
PAIRS = teo.PAIRS


def test_the_restated_case_lists_are_the_encode_once_ones():
    assert LENS == teo.LENS and GATHER_PAIRS == teo.GATHER_PAIRS


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. spr_pair_gather_bwd -------------------------------------------------------------------------------------------
def _bwd_case(c, npairs, device):
    """gy on the CPU, the layout, and the float32 sum taken on the CPU in ascending segment order (the first use as it
    is, then pure additions); rows of unused clouds zero."""
    pairs = GATHER_PAIRS[npairs]
    lay = shared_clouds.PairLayout([i for i, _ in pairs], [j for _, j in pairs], [LENS], device)
    g = torch.Generator().manual_seed(1000 * c + npairs)
    gy = torch.randn(lay.rows[0], c, generator=g)
    cu, cu_out, order = np.concatenate([[0], np.cumsum(LENS)]), lay.host["cu_out"][0], lay.host["seg_cloud"]
    ref = torch.zeros(sum(LENS), c)
    for k in range(len(LENS)):
        acc = None
        for s in range(2 * npairs):                       # ascending segment index
            if order[s] == k:
                rows = gy[cu_out[s]:cu_out[s + 1]]
                acc = rows.clone() if acc is None else acc + rows
        if acc is not None:
            ref[cu[k]:cu[k + 1]] = acc
    return gy, lay, ops.lengths_to_cu(LENS, device), ref


def _gather_bwd(gy, lay, cu, **kw):
    return shared_clouds.pair_gather_bwd(gy, cu, lay.use_ptr, lay.use_seg, lay.cu_out[0], rows=sum(LENS), **kw)


@pytest.mark.parametrize("npairs", [1, 7])
@pytest.mark.parametrize("c", [256, 3])
def test_pair_gather_bwd_is_the_ordered_sum(device, c, npairs):
    gy, lay, cu, ref = _bwd_case(c, npairs, device)
    got = _gather_bwd(gy.to(device), lay, cu)
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert torch.equal(_bits(got.cpu()), _bits(ref))
    # every row is written: a NaN-filled buffer comes back with the unused cloud's rows exactly zero
    buf = torch.full((sum(LENS) + 2, c), float("nan"), device=device)
    out = _gather_bwd(gy.to(device), lay, cu, out=buf[:sum(LENS)])
    assert out.data_ptr() == buf.data_ptr() and torch.equal(_bits(out.cpu()), _bits(ref))
    assert torch.isnan(buf[sum(LENS):]).all()
    start = np.concatenate([[0], np.cumsum(LENS)])
    used = {int(k) for k in lay.host["seg_cloud"]}
    assert 2 not in used or npairs == 1
    for k in set(range(len(LENS))) - used:
        assert not _bits(out[start[k]:start[k + 1]]).any()            # +0.0, bit for bit
    if c % 4 == 0:
        # an output that starts 4 bytes behind a 16-byte boundary takes the 4-byte path: same bits
        flat = torch.full((ref.numel() + 1,), float("nan"), device=device)
        out = _gather_bwd(gy.to(device), lay, cu, out=flat[1:].view(ref.shape))
        assert torch.equal(_bits(out.cpu()), _bits(ref)) and torch.isnan(flat[0])


def test_pair_gather_bwd_on_a_side_stream(device):
    gy, lay, cu, ref = _bwd_case(256, 7, device)
    gy = gy.to(device)
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        got = _gather_bwd(gy, lay, cu)
    side.synchronize()
    assert torch.equal(_bits(got.cpu()), _bits(ref))


@pytest.mark.parametrize("npairs", [1, 7])
@pytest.mark.parametrize("c", [256, 3])
def test_autograd_through_the_gather(device, c, npairs):
    gy, lay, cu, ref = _bwd_case(c, npairs, device)
    x = torch.randn(sum(LENS), c, generator=torch.Generator().manual_seed(5)).to(device).requires_grad_(True)
    ops.ensure_range(x)
    y = shared_clouds.pair_gather(x, cu, lay)
    assert y.requires_grad and torch.equal(y.detach(), ops.pair_gather(x.detach(), cu, lay.seg_cloud[:npairs],
                                                                      lay.seg_cloud[npairs:], lay.cu_out[0], rows=lay.rows[0]))
    assert ops._get_range(y)[0] is ops._get_range(x)[0] is not None   # the operand range rides along
    (gx,) = torch.autograd.grad(y, x, gy.to(device))
    assert torch.equal(_bits(gx.cpu()), _bits(ref))
    with torch.no_grad():
        assert not shared_clouds.pair_gather(x, cu, lay).requires_grad


# ---- 2. spr_overlap_pool_pairs ----------------------------------------------------------------------------------------
W = 7
LENS0 = [4 * n + 1 for n in LENS]                          # the finer level of the toy pyramid


def _pool_case(npairs, device):
    """A two-level pyramid in cloud layout (pool width 7, shadow entries = the level's total, one row of shadow entries
    only), labels in pair layout, and the pair-layout pool matrix materialised on the CPU: the rows of every segment's
    cloud, indices rebased to the segment, shadow -> the new total."""
    pairs = GATHER_PAIRS[npairs]
    lay = shared_clouds.PairLayout([i for i, _ in pairs], [j for _, j in pairs], [LENS0, LENS], device)
    g = torch.Generator().manual_seed(900 + npairs)
    cu0, cu1 = np.concatenate([[0], np.cumsum(LENS0)]), np.concatenate([[0], np.cumsum(LENS)])
    n0 = int(cu0[-1])
    pool = torch.empty(sum(LENS), W, dtype=torch.int64)
    for k in range(len(LENS)):
        r = torch.randint(0, LENS0[k] + 2, (LENS[k], W), generator=g)
        pool[cu1[k]:cu1[k + 1]] = torch.where(r >= LENS0[k], torch.tensor(n0), r + int(cu0[k]))
    pool[cu1[4] + 5] = n0                                  # cloud 4 (in both pair lists): a row of shadow entries only
    pool[cu1[4] + 6, 1:] = n0                              # ... and a row with one valid entry
    ov = torch.rand(lay.rows[0], generator=g)
    ov[::17] = 1.0
    co0, order = lay.host["cu_out"][0], lay.host["seg_cloud"]
    total = lay.rows[0]
    rows = []
    for s, k in enumerate(order):
        blk = pool[cu1[k]:cu1[k + 1]]
        rows.append(torch.where(blk >= n0, torch.tensor(total), blk - int(cu0[k]) + int(co0[s])))
    return lay, pool.to(torch.int32), ov, torch.cat(rows).to(torch.int32)


def _pool_pairs(lay, pool, ov, cu0, cu1):
    return shared_clouds.overlap_pool_pairs(ov, pool, cu0, cu1, lay.seg_cloud, lay.cu_out[0], lay.cu_out[1], lay.rows[1])


@pytest.mark.parametrize("npairs", [1, 7])
def test_overlap_pool_pairs_is_overlap_pool_on_the_pair_layout(device, npairs):
    lay, pool, ov, pool_pairs = _pool_case(npairs, device)
    cu0, cu1 = ops.lengths_to_cu(LENS0, device), ops.lengths_to_cu(LENS, device)
    got = _pool_pairs(lay, pool.to(device), ov.to(device), cu0, cu1).cpu()
    ref = ops.overlap_pool(ov.to(device), pool_pairs.to(device), lay.rows[0]).cpu()
    assert got.shape == ref.shape == (lay.rows[1],)
    nan = torch.isnan(ref)
    assert int(nan.sum()) == int((lay.host["seg_cloud"] == 4).sum()) >= 1       # the all-shadow row, once per use
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(_bits(got), _bits(ref))
    # a pool matrix whose rows are wider than its columns (a column slice: stride 8, 16-byte index loads)
    wide = torch.full((pool.shape[0], W + 1), -5, dtype=torch.int32)
    wide[:, :W] = pool
    sliced = wide.to(device)[:, :W]
    assert sliced.stride(0) == W + 1
    nq = lay.rows[1]
    out = torch.empty(nq, device=device)
    from superpoints_registration_amd import _lib
    _lib.check(_lib.lib().spr_overlap_pool_pairs(ops._ptr(ov.to(device)), ov.numel(), ops._ptr(sliced), W + 1, W,
                                                 pool.shape[0], ops._ptr(cu0), ops._ptr(cu1), len(LENS),
                                                 ops._ptr(lay.seg_cloud), npairs, ops._ptr(lay.cu_out[0]),
                                                 ops._ptr(lay.cu_out[1]), nq, ops._ptr(out), ops._stream(out)),
               "spr_overlap_pool_pairs")
    assert torch.equal(_bits(out.cpu()), _bits(ref))
    # against float64, within the bound of tests/test_gpu_match_range.py::test_overlap_pool_edges
    idx = pool_pairs.long()
    ext = torch.cat([ov.double(), torch.zeros(1, dtype=F64)])
    valid = (idx < lay.rows[0]).double()
    ref64 = (ext[idx] * valid).sum(1) / valid.sum(1)
    assert torch.equal(torch.isnan(ref64), nan)
    err = (got.double()[~nan] - ref64[~nan].clamp(0, 1)).abs()
    assert bool((err <= (W + 2) * U * ref64[~nan].abs() + 1e-30).all()), f"err {float(err.max()):.3e}"


# ---- 3. both operators between poisoned guard bands ----------------------------------------------------------------------
def _bounded(monkeypatch, f, what, min_calls):
    """f(put) in production and under both flavours of the tensor arena; the results must agree bit for bit."""
    production = f(lambda t: t)
    for flavour in (1, 2):
        tensors = TensorArena(flavour, GUARD)
        with monkeypatch.context() as m:
            tensors.install(m)
            guarded = f(tensors.put)
        tensors.verify()                                   # nothing outside the outputs (and the placed inputs) written
        assert tensors.calls >= min_calls, (what, tensors.calls)
        for a, b in zip(production, guarded):
            assert torch.equal(_bits(a), _bits(b)), (what, flavour)
    return production


@pytest.mark.parametrize("npairs", [1, 7])
@pytest.mark.parametrize("c", [256, 3])
def test_pair_gather_bwd_inside_its_tensors(device, monkeypatch, c, npairs):
    gy, lay, cu, ref = _bwd_case(c, npairs, device)

    def f(put):
        ins = [put(t) for t in (gy.to(device), cu, lay.use_ptr.clone(), lay.use_seg.clone(), lay.cu_out[0].clone())]
        keep = [t.clone() for t in ins]
        out = shared_clouds.pair_gather_bwd(*ins, rows=sum(LENS))
        assert all(torch.equal(a, b) for a, b in zip(ins, keep)), "an input was written"
        return [out]
    (got,) = _bounded(monkeypatch, f, "pair_gather_bwd", 6)
    assert torch.equal(_bits(got.cpu()), _bits(ref))


@pytest.mark.parametrize("npairs", [1, 7])
def test_overlap_pool_pairs_inside_its_tensors(device, monkeypatch, npairs):
    lay, pool, ov, pool_pairs = _pool_case(npairs, device)
    ref = ops.overlap_pool(ov.to(device), pool_pairs.to(device), lay.rows[0])

    def f(put):
        ins = [put(t) for t in (ov.to(device), pool.to(device), ops.lengths_to_cu(LENS0, device),
                                ops.lengths_to_cu(LENS, device), lay.seg_cloud.clone(), lay.cu_out[0].clone(),
                                lay.cu_out[1].clone())]
        keep = [t.clone() for t in ins]
        out = shared_clouds.overlap_pool_pairs(*ins, rows=lay.rows[1])
        assert all(torch.equal(a, b) for a, b in zip(ins, keep)), "an input was written"
        return [out]
    (got,) = _bounded(monkeypatch, f, "overlap_pool_pairs", 8)
    assert torch.equal(_bits(got), _bits(ref))


# ---- 4. the model: no reuse is the old forward; against the reference -----------------------------------------------------
_STEPS = {}


def _grads(model):
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}


def _golden_step(tag, device, shared):
    """tests/test_gpu_backward.py::_train_step(tag, device, "total"), through either batch form; computed once."""
    key = (tag, shared)
    if key not in _STEPS:
        g = load_golden(f"grad_{tag}_b2.npz")
        B = int(g["B"])
        assert B == 2
        pairs, sizes = pairs_for(tag, B)
        pose, src_ov, tgt_ov = loss_inputs(tag, B)
        model = RegTR(get_config(tag))
        synthetic.fill_parameters(model, seed=int(g["seed"]))
        model = model.to(device).train()
        src = [T(p[0][:n]).to(device) for p, (n, m) in zip(pairs, sizes)]
        tgt = [T(p[1][:m]).to(device) for p, (n, m) in zip(pairs, sizes)]
        batch = {"pose": T(pose).to(device),
                 "src_overlap": [T(o).to(device) for o in src_ov], "tgt_overlap": [T(o).to(device) for o in tgt_ov]}
        if shared:
            batch.update(clouds=src + tgt, pairs=[(0, 2), (1, 3)])
        else:
            batch.update(src_xyz=src, tgt_xyz=tgt)
        out = model(batch)
        losses = model.compute_loss(out, batch)
        model.zero_grad(set_to_none=True)
        losses["total"].backward()
        _STEPS[key] = dict(g=g, model=model, out=out, losses={k: v.detach() for k, v in losses.items()}, batch=batch)
    return _STEPS[key]


def test_no_reuse_is_the_old_forward_bit_for_bit(device):
    """clouds = src + tgt, pairs = [(0, 2), (1, 3)]: the tail receives the same rows in the same order and every sum of
    the backward has a fixed order, so outputs, losses and every parameter gradient carry the same bits."""
    a, b = _golden_step("3dmatch", device, False), _golden_step("3dmatch", device, True)
    assert b["batch"]["src_xyz"][1] is b["batch"]["clouds"][1] and b["batch"]["tgt_xyz"][0] is b["batch"]["clouds"][2]
    assert torch.equal(_bits(a["out"]["pose"]), _bits(b["out"]["pose"]))
    for key in teo.LIST_KEYS:
        assert len(a["out"][key]) == len(b["out"][key]) == 2
        for x, y in zip(a["out"][key], b["out"][key]):
            assert x.dtype == y.dtype and torch.equal(x, y), key
    for k in ("feature", "T", "overlap", "total"):
        assert torch.equal(_bits(a["losses"][k]), _bits(b["losses"][k])), k
    for lvl, x in a["batch"]["overlap_pyr"].items():
        assert torch.equal(_bits(x), _bits(b["batch"]["overlap_pyr"][lvl])), lvl
    n = 0
    for (k1, p1), (k2, p2) in zip(a["model"].named_parameters(), b["model"].named_parameters()):
        assert k1 == k2 and (p1.grad is None) == (p2.grad is None), k1
        if p1.grad is not None:
            assert torch.equal(_bits(p1.grad), _bits(p2.grad)), k1
            n += 1
    assert n > 100


def _check_against(tag, which, model, losses, g, f64_scalars):
    """The criteria of tests/test_gpu_backward.py::test_parameter_gradients_match_the_reference and its loss check, with
    `g` in the reference's role (its docstring gives the reasons for every window).  f64_scalars(name) -> d loss / d
    alpha, beta by the float64 oracle."""
    for k in ("feature", "T", "overlap", "total"):
        assert abs(float(losses[k]) - float(g[f"loss_{k}"])) <= 5e-5 * max(1.0, abs(float(g[f"loss_{k}"]))), k
    n_checked, n_enc, enc_loose, report = 0, 0, 0, []
    for name, p in model.items():
        if f"{which}|{name}|none" in g:
            assert p is None or float(p.abs().max()) == 0.0, f"{name}: the reference has no gradient here"
            continue
        if f"{which}|{name}|norm" not in g:
            continue
        assert p is not None, f"{name}: no gradient"
        gr = p.double().reshape(-1).cpu().numpy()
        ref_norm = float(g[f"{which}|{name}|norm"])
        if f"{which}|{name}|full" in g:
            ref_e, got_e = np.asarray(g[f"{which}|{name}|full"]).astype(np.float64).reshape(-1), gr
        else:
            ref_e = g[f"{which}|{name}|samples"].astype(np.float64)
            got_e = gr[grad_sample_indices(name, gr.size)]
        scale = max(np.abs(ref_e).max(), ref_norm / math.sqrt(gr.size), 1e-30)
        err = np.abs(got_e - ref_e).max() / scale
        rms = np.sqrt(np.mean((got_e - ref_e) ** 2)) / max(np.sqrt(np.mean(ref_e ** 2)), 1e-30)
        nerr = abs(np.linalg.norm(gr) - ref_norm) / max(ref_norm, 1e-30)
        n_checked += 1
        if name in ("alpha", "beta"):
            assert nerr <= 1e-3, f"{tag} {name}: deviates by {nerr:.2e}"
            ours, ref_v = float(gr[0]), float(ref_e.reshape(-1)[0])
            # e_ours <= max(1e-4, 2 e_ref) against the float64 oracle holds whenever ours is within 5e-5 of the
            # reference (e_ours <= e_ref + 5e-5 <= max(1e-4, 2 e_ref)); only otherwise is the oracle needed
            if abs(ours - ref_v) > 5e-5 * abs(ref_v) * (1 - 1e-3):
                f64 = f64_scalars(name)
                e_ours, e_ref = abs(ours - f64) / abs(f64), abs(ref_v - f64) / abs(f64)
                assert e_ours <= max(1e-4, 2.0 * e_ref), f"{tag} d{name}: {e_ours:.2e} from float64 (reference: {e_ref:.2e})"
        elif name.startswith("kpf_encoder."):
            n_enc += 1
            enc_loose += err > 1e-4
            assert nerr <= 5e-4, f"{tag} {name}: norm deviates by {nerr:.2e}"
            assert rms <= 2e-2, f"{tag} {name}: RMS deviation {rms:.2e}"
        else:
            assert nerr <= 1e-4, f"{tag} {name}: norm deviates by {nerr:.2e}"
            assert err <= 1e-4, f"{tag} {name}: entries deviate by {err:.2e}"
        report.append((err, name))
    report.sort(reverse=True)
    print(f"{tag}: {n_checked} tensors; encoder tensors above 1e-4 entrywise: {enc_loose}/{n_enc}; worst: " +
          ", ".join(f"{n} {e:.1e}" for e, n in report[:3]))
    assert n_checked >= 100
    return enc_loose, n_enc


@pytest.mark.parametrize("tag", ["3dmatch", "kitti", "modelnet"])
def test_the_shared_route_matches_the_reference(device, tag):
    """The cloud / pair batch on the reference's golden training step (two-, three- and four-level overlap pyramids)."""
    s = _golden_step(tag, device, True)
    assert len(s["batch"]["kpconv_meta"]["points"]) == {"modelnet": 2, "3dmatch": 3, "kitti": 4}[tag]
    enc_loose, n_enc = _check_against(tag, "total", _grads(s["model"]), s["losses"], s["g"],
                                      lambda name: tgb._f64_sinkhorn_scalar_grads(tag, "total")[name])
    if tag != "3dmatch":                                   # test_parameter_gradients_match_the_reference says why
        assert enc_loose <= 0.5 * n_enc, f"{enc_loose} of {n_enc} encoder tensors deviate entrywise"


# ---- 5. reuse: four views of one surface, five pairs ---------------------------------------------------------------------
def _views():
    """Four partial views (~3 000 points each) of one synthetic surface, each under its own rigid motion and in its own
    point order, and the true pose of every pair of PAIRS (src -> tgt)."""
    rng = np.random.default_rng(2024)
    base = synthetic.box_faces(4200, rng, 2.0) + rng.normal(0.0, 0.005, (4200, 3))
    dirs = np.array([[1.0, 0.2, 0.1], [-0.3, 1.0, 0.2], [0.2, -0.1, 1.0], [-1.0, -0.6, 0.3]])
    clouds, motion = [], []
    for v in range(4):
        keep = base[np.argsort(base @ dirs[v])[-3024:]]
        R, t = synthetic.rotation_z(0.12 * v - 0.1), np.array([0.05 * v, -0.03 * v, 0.02 * (v - 1)])
        pts = keep @ R.T + t + rng.normal(0.0, 0.002, keep.shape)
        clouds.append(pts[rng.permutation(len(pts))].astype(np.float32))
        motion.append((R, t))
    poses = []
    for i, j in PAIRS:
        (Ri, ti), (Rj, tj) = motion[i], motion[j]
        R = Rj @ Ri.T
        poses.append(np.concatenate([R, (tj - R @ ti)[:, None]], 1))
    return clouds, np.stack(poses).astype(np.float32)


@pytest.fixture(scope="module")
def reuse(device):
    """One model; the training step on the expanded pair lists, then twice on the cloud / pair batch, with the same
    labels.  Computed once and only read by the tests below."""
    clouds, pose = _views()
    clouds, pose = [T(c).to(device) for c in clouds], T(pose).to(device)
    cfg = get_config("3dmatch")
    model = RegTR(cfg)
    synthetic.fill_parameters(model, seed=0)
    model = model.to(device).train()
    expanded = {"src_xyz": [clouds[i] for i, _ in PAIRS], "tgt_xyz": [clouds[j] for _, j in PAIRS], "pose": pose}
    overlap.label_batch(expanded, cfg.overlap_radius)
    runs = []
    for form in ("expanded", "shared", "shared"):
        batch = dict(expanded) if form == "expanded" else {
            "clouds": clouds, "pairs": PAIRS, "pose": pose,
            "src_overlap": expanded["src_overlap"], "tgt_overlap": expanded["tgt_overlap"]}
        out = model(batch)
        losses = model.compute_loss(out, batch)
        model.zero_grad(set_to_none=True)
        losses["total"].backward()
        runs.append(dict(out=out, losses={k: v.detach() for k, v in losses.items()}, batch=batch, grads=_grads(model)))
    torch.cuda.synchronize()
    return dict(model=model, cfg=cfg, clouds=clouds, pose=pose, expanded=runs[0], shared=runs[1], again=runs[2])


def test_reuse_labels_are_mixed(reuse):
    for side in ("src_overlap", "tgt_overlap"):
        for b, m in enumerate(reuse["expanded"]["batch"][side]):
            assert m.dtype == torch.bool and bool(m.any()) and not bool(m.all()), (side, b)


def test_reuse_forward_and_losses_equal_the_expanded_forward(reuse):
    a, b = reuse["shared"], reuse["expanded"]
    lens = reuse["shared"]["batch"]["_pair_layout"].seg_lens[-1]
    n_gt_m = [lens[p] > lens[len(PAIRS) + p] for p in range(len(PAIRS))]
    assert any(n_gt_m) and not all(n_gt_m)                 # both matching branches ran (N > M and N <= M)
    assert a["out"]["pose"].shape == b["out"]["pose"].shape == (len(PAIRS), 3, 4)
    for p, pair in enumerate(PAIRS):
        teo._assert_rounding_level(a["out"], p, b["out"], p, f"pair {p} = {pair}")
    for k in ("feature", "T", "overlap", "total"):
        x, y = float(a["losses"][k]), float(b["losses"][k])
        assert abs(x - y) <= 5e-5 * max(1.0, abs(y)), (k, x, y)


def test_reuse_overlap_pyramid_is_the_expanded_one(reuse):
    """Level by level and bit for bit, pair by pair: segment s of the shared route is cloud k's rows, the expanded route
    holds them at position s of its own cloud layout."""
    a, b = reuse["shared"]["batch"], reuse["expanded"]["batch"]
    lay = a["_pair_layout"]
    assert set(a["overlap_pyr"]) == set(b["overlap_pyr"]) == {f"pyr_{l}" for l in range(lay.levels)}
    for l in range(lay.levels):
        x, y = a["overlap_pyr"][f"pyr_{l}"], b["overlap_pyr"][f"pyr_{l}"]
        assert b["kpconv_meta"]["_lens_host"][l] == lay.seg_lens[l]
        assert torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(_bits(x), _bits(y)), l


def test_reuse_parameter_gradients_equal_the_expanded_forward(reuse):
    """test_parameter_gradients_match_the_reference's criteria with the expanded forward in the reference's role (every
    tensor compared whole).  The encoder keeps its decision-flip window: a cloud's rows are scaled by the ranges of
    another batch composition, and an activation within rounding of zero takes the other LeakyReLU branch."""
    ref = reuse["expanded"]
    g = {f"loss_{k}": float(v) for k, v in ref["losses"].items()}
    for name, t in ref["grads"].items():
        if t is None or float(t.abs().max()) == 0.0:
            g[f"total|{name}|none"] = True
        else:
            g[f"total|{name}|norm"] = float(t.double().norm())
            g[f"total|{name}|full"] = t.double().cpu().numpy()

    def f64_scalars(name):
        if "f64" not in reuse:
            from oracle import torch_oracle as O
            cfg, b = reuse["cfg"], ref["batch"]
            sd = {k: (v.detach().cpu().clone().double() if v.is_floating_point() else v.cpu().clone())
                  for k, v in reuse["model"].state_dict().items()}
            for k in ("alpha", "beta"):
                sd[k].requires_grad_(True)
            fwd = O.regtr_forward(cfg, sd, [c.cpu().numpy() for c in b["src_xyz"]], [c.cpu().numpy() for c in b["tgt_xyz"]])
            L = O.compute_loss(cfg, sd, fwd, reuse["pose"].cpu().numpy(), [m.cpu().numpy() for m in b["src_overlap"]],
                               [m.cpu().numpy() for m in b["tgt_overlap"]])
            L["total"].backward()
            reuse["f64"] = {k: float(sd[k].grad) for k in ("alpha", "beta")}
        return reuse["f64"][name]
    _check_against("reuse", "total", reuse["shared"]["grads"], reuse["shared"]["losses"], g, f64_scalars)


def test_reuse_is_bitwise_reproducible(reuse):
    a, b = reuse["shared"], reuse["again"]
    assert torch.equal(_bits(a["out"]["pose"]), _bits(b["out"]["pose"]))
    n = 0
    for k, x in a["grads"].items():
        assert (x is None) == (b["grads"][k] is None), k
        if x is not None:
            assert torch.equal(_bits(x), _bits(b["grads"][k])), k
            n += 1
    assert n > 100


# ---- 6. Trainer -----------------------------------------------------------------------------------------------------------
def test_trainer_on_a_cloud_batch(reuse):
    cfg, clouds, pose = reuse["cfg"], reuse["clouds"], reuse["pose"]
    shared_batch = lambda: {"clouds": clouds, "pairs": PAIRS, "pose": pose}
    expanded_batch = lambda: {"src_xyz": [clouds[i] for i, _ in PAIRS], "tgt_xyz": [clouds[j] for _, j in PAIRS], "pose": pose}
    m_s, m_e = copy.deepcopy(reuse["model"]), copy.deepcopy(reuse["model"])
    t_s, t_e = Trainer(cfg).setup(m_s), Trainer(cfg).setup(m_e)
    # validate first, on equal weights: the metrics of the expanded batch
    v_s, v_e = t_s.validate(m_s, [shared_batch()]), t_e.validate(m_e, [expanded_batch()])
    for k in ("feature", "T", "overlap", "total"):
        x, y = float(v_s["losses"][k]), float(v_e["losses"][k])
        assert abs(x - y) <= 5e-5 * max(1.0, abs(y)), (k, x, y)
    assert set(v_s["metrics"]) == set(v_e["metrics"]) and v_e["metrics"]
    for k, y in v_e["metrics"].items():
        x = v_s["metrics"][k]
        # d = ||pose - pose'||_F < 1e-5 is _assert_rounding_level's pose bound; 4 ulp of 1 for the float32 evaluation
        # of the metric itself (se3_compare: pred o gt^-1, trace, arc cosine)
        d, ulp = 1e-5, 4 * 2.0 ** -23
        if "_success" in k:
            assert torch.equal(x, y), k
        elif k.startswith("trans_err"):
            # t = t_pred - R_pred R_gt^T t_gt moves by at most d sqrt(1 + |t_gt|^2)
            tol = d * math.sqrt(1.0 + float(pose[:, :, 3].norm(dim=1).max()) ** 2) + ulp
            assert float((x - y).abs().max()) <= tol, (k, float((x - y).abs().max()))
        else:
            # cos = (trace - 1) / 2 moves by at most c = sqrt(3) / 2 d, and the angle is its arc cosine: a pair's angle
            # moves by at most acos(cos - c) - acos(cos + c) (valid next to 0 and 180 degrees, where 1 / sin is not);
            # the mean over the pairs by at most the mean of that
            c = math.sqrt(3.0) / 2.0 * d + ulp
            per_pair = v_e["metrics"][[h for h in v_e["metrics"] if h.startswith("rot_err") and h.endswith("_hist")][0]]
            cos = torch.cos(torch.deg2rad(per_pair.double()))
            tol = torch.rad2deg(torch.acos((cos - c).clamp(-1, 1)) - torch.acos((cos + c).clamp(-1, 1)))
            tol = tol if k.endswith("_hist") else tol.mean()
            rep = 2 * 2.0 ** -23 * 180.0                  # the two angles themselves are float32 numbers of degrees
            assert bool(((x - y).abs().double() <= tol + rep).all()), (k, float((x - y).abs().max()), tol)
    # two steps on the same cloud batch (the views a forward leaves in it are legal on the next one)
    batch = shared_batch()
    l_s = t_s.train_step(m_s, batch)
    l_e = t_e.train_step(m_e, expanded_batch())
    assert "src_overlap" in batch and "_pair_layout" in batch and batch["src_xyz"][2] is clouds[PAIRS[2][0]]
    for k in ("feature", "T", "overlap", "total"):
        x, y = float(l_s[k]), float(l_e[k])
        assert abs(x - y) <= 5e-5 * max(1.0, abs(y)), (k, x, y)
    l_2 = t_s.train_step(m_s, batch)
    assert t_s.global_step == 2 and all(bool(torch.isfinite(v)) for v in l_2.values())
    assert float(l_2["total"]) != float(l_s["total"])      # the optimizer stepped
    assert t_s.fit(m_s, [batch], epochs=1) == 3
    with pytest.raises(ValueError, match="augment"):
        Trainer(cfg, augment=True).setup(m_s).train_step(m_s, shared_batch())
