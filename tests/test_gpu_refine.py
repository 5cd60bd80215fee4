"""GPU: ops.refine_pairs (spr_refine_pairs) -- the config-off refinements for all pairs in one call -- against the
float64 replica (tests/refine_replica.py), the reference's outputs (tests/golden/refine_ops.npz) and the per-pair
route it replaces (parent_loop below: the former RegTR._refined_pose, kept here as the yardstick).

Pose tolerance.  The former route's distance from the float64 replica is measured on the same inputs, case by case;
the one-call route may be at most twice that far (its reductions could be ordered differently), and never further than
the 1e-3 of test_refinement_switches_match_the_reference.  Measured on the MI355X: both routes are bit-equal on every
case here (the kernel shares the Procrustes solve and the residual arithmetic), 2e-8 .. 8e-8 from the replica.
Selections are compared exactly on every entry the ratio / median / overlap steps left > 0; the inputs keep the gaps
the issue asks for (asserted through the replica's trace)."""
import numpy as np
import pytest
import torch

import refine_replica
from conftest import load_golden
from oracle.gen_golden import REFINE_CASES
from superpoints_registration_amd import get_config, ops
from superpoints_registration_amd.regtr import RegTR

pytestmark = pytest.mark.gpu

REPLICA_KW = {"use_ratio_test": "ratio", "threshold_corr": "median", "remove_outliers_overlap": "overlap",
              "use_overlap_as_weights": "overlap_w"}
ALL = dict(use_ratio_test=True, threshold_corr=True, remove_outliers_overlap=True, remove_points_from_val=True,
           use_lgr=True)


def make_cfg(flags):
    cfg = get_config("kitti")
    cfg.update(flags)
    return cfg


def parent_loop(cfg, xyz_c, overlap, val, val2, ind, cu_host, B, sk_pose=None, k_list=None):
    """RegTR._refined_pose as it was before ops.refine_pairs: pair by pair, a string of torch operators and one-pair
    library calls.  Only the Sinkhorn solve (now an argument) and the optional explicit k differ from the original."""
    dev = xyz_c.device
    out = {k: [] for k in ('pose', 'val', 'ind', 'src_pts', 'tgt_pts')}
    for b in range(B):
        s0, s1, t0, t1 = cu_host[b], cu_host[b + 1], cu_host[B + b], cu_host[B + b + 1]
        N, M = s1 - s0, t1 - t0
        src_xyz, tgt_xyz = xyz_c[s0:s1], xyz_c[t0:t1]
        ov_s, ov_t = overlap[s0:s1, 0], overlap[t0:t1, 0]
        own = slice(t0, t1) if N > M else slice(s0, s1)
        v, i = val[own].clone(), ind[own].long()
        if cfg.get('use_ratio_test', False):
            v = torch.where(val2[own] / v < cfg.lowe_thres, v, torch.zeros_like(v))
        if cfg.get('threshold_corr', False):
            v = torch.where(v > torch.median(v), v, torch.zeros_like(v))
        if N > M:
            src_pts = src_xyz if cfg.use_sinkhorn else src_xyz[i]
            tgt_pts = tgt_xyz
        else:
            src_pts = src_xyz
            tgt_pts = tgt_xyz if cfg.use_sinkhorn else tgt_xyz[i]
        ov = None
        if cfg.get('remove_outliers_overlap', False):
            ov = (ov_s[i] * ov_t) if N > M else (ov_s * ov_t[i])
            if not cfg.get('use_overlap_as_weights', False):
                v = v * ov
        if cfg.get('remove_points_from_val', False):
            k = int(cfg.val_threshold * (M if N > M else N)) if k_list is None else k_list[b]
            v, i = torch.topk(v, k)
            src_pts, tgt_pts = src_pts[i], tgt_pts[i]
            if ov is not None:
                ov = ov[i]
        one = torch.tensor([0, src_pts.shape[0]], dtype=torch.int32, device=dev)
        if cfg.use_sinkhorn:
            T = sk_pose[b]
        else:
            wts = ov if cfg.get('use_overlap_as_weights', False) else v
            T = ops.weighted_procrustes(src_pts.contiguous(), tgt_pts.contiguous(), wts.contiguous(), one)[0]
        if cfg.get('use_lgr', False):
            wl = v
            for _ in range(int(cfg.num_refinement_steps)):
                res = ops.pose_residuals(T[None].contiguous(), src_pts.contiguous(), tgt_pts.contiguous(), one)
                wl = wl * (res < cfg.acceptance_radius).float()
                T = ops.weighted_procrustes(src_pts.contiguous(), tgt_pts.contiguous(), wl.contiguous(), one)[0]
        for k_, v_ in (('pose', T), ('val', v), ('ind', i), ('src_pts', src_pts), ('tgt_pts', tgt_pts)):
            out[k_].append(v_)
    out['pose'] = torch.stack(out['pose'])
    return out


def new_route(cfg, xyz_c, overlap, val, val2, ind, cu, cu_host, B, sk_pose=None, k_list=None):
    on = lambda f: bool(cfg.get(f, False))
    k = None
    if on('remove_points_from_val'):
        k = k_list if k_list is not None else [
            int(cfg.val_threshold * min(cu_host[b + 1] - cu_host[b], cu_host[B + b + 1] - cu_host[B + b]))
            for b in range(B)]
    r = ops.refine_pairs(val, val2, ind, overlap, xyz_c, cu, cu_host, B, k, ratio=on('use_ratio_test'),
                         median=on('threshold_corr'), overlap_prune=on('remove_outliers_overlap'),
                         overlap_as_weights=on('use_overlap_as_weights'),
                         lgr_steps=int(cfg.num_refinement_steps) if on('use_lgr') else 0,
                         lowe_thres=float(cfg.lowe_thres), acceptance_radius=float(cfg.acceptance_radius),
                         pose_in=sk_pose, sinkhorn=bool(cfg.use_sinkhorn))
    oc = r['out_cu']
    out = {k_: [r[k_][oc[b]:oc[b + 1]] for b in range(B)] for k_ in ('val', 'ind', 'src_pts', 'tgt_pts')}
    out['pose'], out['status'] = r['pose'], r['status']
    return out


def replica_route(cfg, xyz_c, overlap, val, val2, ind, cu_host, B, sk_pose=None, k_list=None, traces=None):
    on = lambda f: bool(cfg.get(f, False))
    xyz, ov = xyz_c.cpu().numpy(), overlap.cpu().numpy().reshape(-1)
    val, ind = val.cpu().numpy(), ind.cpu().numpy()
    val2 = val2.cpu().numpy() if val2 is not None else None
    outs = []
    for b in range(B):
        s0, s1, t0, t1 = cu_host[b], cu_host[b + 1], cu_host[B + b], cu_host[B + b + 1]
        own = slice(t0, t1) if s1 - s0 > t1 - t0 else slice(s0, s1)
        k = None
        if on('remove_points_from_val'):
            k = k_list[b] if k_list is not None else int(cfg.val_threshold * min(s1 - s0, t1 - t0))
        tr = {}
        outs.append(refine_replica.refine_pair(
            val[own], None if val2 is None else val2[own], ind[own], ov[s0:s1], ov[t0:t1], xyz[s0:s1], xyz[t0:t1],
            k=k, lgr_steps=int(cfg.num_refinement_steps) if on('use_lgr') else 0, lowe_thres=float(cfg.lowe_thres),
            radius=float(cfg.acceptance_radius), pose_in=None if sk_pose is None else sk_pose[b].cpu().numpy(),
            sinkhorn=bool(cfg.use_sinkhorn), trace=tr, **{REPLICA_KW[f]: True for f in REPLICA_KW if on(f)}))
        if traces is not None:
            traces.append(tr)
    return outs


def assert_gaps(cfg, traces):
    """The discrete choices keep their distance in float64: >= 1e-5 for every ratio, >= 1e-4 relative for every LGR
    residual -- otherwise float32 routes may legitimately differ and the comparison means nothing."""
    for tr in traces:
        if "ratios" in tr:
            r = tr["ratios"][np.isfinite(tr["ratios"])]
            assert r.size == 0 or np.abs(r - np.float32(cfg.lowe_thres)).min() >= 1e-5
        for res in tr.get("residuals", []):
            assert (np.abs(res - cfg.acceptance_radius) >= 1e-4 * cfg.acceptance_radius).all()


def check_routes(cfg, xyz_c, overlap, val, val2, ind, cu, cu_host, B, sk_pose=None, k_list=None, label="",
                 well_posed=True, with_parent=True):
    """new route == replica on the selections (exactly, on entries > 0), == parent route likewise; poses within
    min(2 x parent's distance from the replica, 1e-3)."""
    traces = []
    rep = replica_route(cfg, xyz_c, overlap, val, val2, ind, cu_host, B, sk_pose, k_list, traces)
    assert_gaps(cfg, traces)
    new = new_route(cfg, xyz_c, overlap, val, val2, ind, cu, cu_host, B, sk_pose, k_list)
    par = parent_loop(cfg, xyz_c, overlap, val, val2, ind, cu_host, B, sk_pose, k_list) if with_parent else None
    assert int(new['status'].abs().max()) == 0
    assert torch.isfinite(new['pose']).all()
    for b in range(B):
        T64, v, i, a, bb = rep[b]
        nv, ni = new['val'][b].cpu().numpy(), new['ind'][b].cpu().numpy()
        na, nb = new['src_pts'][b].cpu().numpy(), new['tgt_pts'][b].cpu().numpy()
        assert nv.shape == v.shape and ni.dtype == np.int64
        live = v > 0
        # the replica orders ties like the kernel (lower position first), so zeroed entries agree as well
        assert np.array_equal(nv.view(np.uint32), v.view(np.uint32)), f"{label} pair {b}: values"
        assert np.array_equal(ni, i), f"{label} pair {b}: indices"
        assert np.array_equal(na, a) and np.array_equal(nb, bb), f"{label} pair {b}: points"
        d_new = np.linalg.norm(new['pose'][b].cpu().numpy().astype(np.float64) - T64)
        msg = f"{label} pair {b}: new route {d_new:.3e} from the replica"
        if par is not None:
            pv, pi = par['val'][b].cpu().numpy(), par['ind'][b].cpu().numpy()
            assert pv.shape == nv.shape
            assert np.array_equal(pv > 0, live)
            assert np.array_equal(pv[live].view(np.uint32), nv[live].view(np.uint32)), f"{label} pair {b}: parent values"
            assert np.array_equal(pi[live], ni[live]), f"{label} pair {b}: parent indices"
            assert np.array_equal(par['src_pts'][b].cpu().numpy()[live], na[live])
            assert np.array_equal(par['tgt_pts'][b].cpu().numpy()[live], nb[live])
            d_par = np.linalg.norm(par['pose'][b].cpu().numpy().astype(np.float64) - T64)
            msg += f", parent route {d_par:.3e}"
        print(msg)
        if well_posed:
            if par is not None:
                assert d_new <= min(2 * d_par, 1e-3), msg
            else:
                assert d_new < 1e-3, msg
        elif par is not None:     # rotation undetermined (fewer than 3 weighted points): the routes must still agree
            assert torch.equal(new['pose'][b], par['pose'][b]), msg
    return new, par, rep


# ---- golden cases through the matching head -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_batch(device):
    g = load_golden("refine_ops.npz")
    B = int(g["B"])
    feat = torch.from_numpy(np.concatenate([g[f"fs{b}"] for b in range(B)] + [g[f"ft{b}"] for b in range(B)])).to(device)
    xyz = torch.from_numpy(np.concatenate([g[f"src{b}"] for b in range(B)] + [g[f"tgt{b}"] for b in range(B)])).to(device)
    ov = torch.from_numpy(np.concatenate([g[f"ov_s{b}"] for b in range(B)] + [g[f"ov_t{b}"] for b in range(B)]))
    ov = ov.to(device)[:, None].contiguous()
    lens = [g[f"src{b}"].shape[0] for b in range(B)] + [g[f"tgt{b}"].shape[0] for b in range(B)]
    cu_host = [0] + list(np.cumsum(lens))
    cu_host = [int(c) for c in cu_host]
    cu = ops.lengths_to_cu(lens, device)
    val, val2, ind = ops.match_dualsoftmax_top2(feat, cu, cu_host, B)
    return dict(g=g, B=B, feat=feat, xyz=xyz, ov=ov, cu=cu, cu_host=cu_host, val=val, val2=val2, ind=ind)


@pytest.mark.parametrize("case", list(REFINE_CASES))
def test_golden_cases_through_the_matching_head(golden_batch, case):
    G = golden_batch
    g, B = G['g'], G['B']
    cfg = make_cfg(REFINE_CASES[case])
    for key in ("lowe_thres", "acceptance_radius", "val_threshold"):
        assert float(cfg[key]) == float(g[key])
    assert int(cfg.num_refinement_steps) == int(g["num_refinement_steps"])
    val2 = G['val2'] if cfg.get('use_ratio_test', False) else None
    new, _, _ = check_routes(cfg, G['xyz'], G['ov'], G['val'], val2, G['ind'], G['cu'], G['cu_host'], B, label=case)
    for b in range(B):        # and the reference's own outputs (its matching head ran in torch on the CPU)
        rv, ri = g[f"{case}.val{b}"], g[f"{case}.ind{b}"]
        live = rv > 0
        nv, ni = new['val'][b].cpu().numpy(), new['ind'][b].cpu().numpy()
        assert nv.shape == rv.shape and np.array_equal(nv > 0, live)
        assert np.array_equal(ni[live], ri[live])
        assert np.allclose(nv[live], rv[live], rtol=5e-3, atol=1e-7)     # the tolerance of the existing golden test
        assert np.array_equal(new['src_pts'][b].cpu().numpy()[live], g[f"{case}.src_corr{b}"][live])
        assert np.array_equal(new['tgt_pts'][b].cpu().numpy()[live], g[f"{case}.tgt_corr{b}"][live])
        err = np.linalg.norm(new['pose'][b].cpu().numpy() - g[f"{case}.pose"][b])
        assert err < 1e-3, f"{case} pair {b}: {err:.2e} from the reference"


@pytest.mark.parametrize("lgr", [False, True])
def test_sinkhorn_pose_stands_and_topk_prunes(golden_batch, lgr):
    """use_sinkhorn + remove_points_from_val (the reference cannot run this pair of switches; replica and parent route
    are the yardsticks): no solve, the points are the clouds' own at the top-k positions, LGR starts from pose_in."""
    G = golden_batch
    B = G['B']
    cfg = make_cfg(dict(remove_points_from_val=True, use_lgr=lgr, use_sinkhorn=True))
    w, t_hat = ops.sinkhorn_correspondences(G['feat'], G['xyz'], G['cu'], G['cu_host'], B, 1.0, 1.0, 3, True)
    sk = ops.weighted_procrustes(G['xyz'][:G['cu_host'][B]], t_hat, w, G['cu'][:B + 1].contiguous())
    new, _, _ = check_routes(cfg, G['xyz'], G['ov'], G['val'], None, G['ind'], G['cu'], G['cu_host'], B, sk_pose=sk,
                             label=f"sinkhorn lgr={lgr}")
    if not lgr:
        assert torch.equal(new['pose'], sk)


# ---- synthetic inputs fed to the operator directly -----------------------------------------------------------------
def synth_pair(rng, n_src, n_tgt, dup=False, dead=False):
    """One pair's own-side val / val2 / ind and both clouds: 80 % of the entries point at the rigidly moved own point
    (3 cm noise), the rest at a partner metres away; ratios sit in [0.3, 0.8] or [0.95, 1.0], far from lowe_thres."""
    on_tgt = n_src > n_tgt
    n, plen = min(n_src, n_tgt), max(n_src, n_tgt)
    ang = 0.2
    R = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]])
    t = np.array([0.7, -0.4, 0.3])
    own = rng.uniform(-10, 10, (n, 3))
    partner = rng.uniform(-10, 10, (plen, 3)) + 30.0
    ind = rng.permutation(plen)[:n]
    good = rng.random(n) < 0.8
    moved = own @ (R if on_tgt else R.T) + (-t if on_tgt else t)    # either direction is a rigid motion
    partner[ind[good]] = moved[good] + rng.normal(0, 0.03, (int(good.sum()), 3))
    partner[ind[~good]] = moved[~good] + rng.uniform(2.0, 5.0, (int((~good).sum()), 3))
    val = rng.uniform(0.05, 0.95, n)
    val[~good] *= 0.2
    if dup:      # exact duplicates straddling the median and the top-k (n // 4) boundary
        srt = np.sort(val)
        val[np.argsort(val)[(n - 1) // 2 - 2:(n - 1) // 2 + 3]] = srt[(n - 1) // 2]
        top = np.argsort(-val)
        val[top[n // 4 - 2:n // 4 + 2]] = val[top[n // 4]]
    ratio = np.where(rng.random(n) < 0.7, rng.uniform(0.3, 0.8, n), rng.uniform(0.95, 1.0, n))
    if dead:
        ratio = rng.uniform(0.95, 1.0, n)
    val = val.astype(np.float32)
    d = dict(val=val, val2=(val * ratio.astype(np.float32)).astype(np.float32), ind=ind.astype(np.int32))
    d['src'], d['tgt'] = ((partner, own) if on_tgt else (own, partner))
    d['ov_s'], d['ov_t'] = rng.uniform(0.3, 1.0, n_src), rng.uniform(0.3, 1.0, n_tgt)
    return d


def pack(pairs, device):
    B = len(pairs)
    lens = [p['src'].shape[0] for p in pairs] + [p['tgt'].shape[0] for p in pairs]
    cu_host = [0] + [int(c) for c in np.cumsum(lens)]
    T = cu_host[-1]
    val, val2, ind = np.zeros(T, np.float32), np.zeros(T, np.float32), np.zeros(T, np.int32)
    for b, p in enumerate(pairs):
        n, m = p['src'].shape[0], p['tgt'].shape[0]
        o = cu_host[B + b] if n > m else cu_host[b]
        k = min(n, m)
        val[o:o + k], val2[o:o + k], ind[o:o + k] = p['val'], p['val2'], p['ind']
    xyz = np.concatenate([p['src'] for p in pairs] + [p['tgt'] for p in pairs]).astype(np.float32)
    ov = np.concatenate([p['ov_s'] for p in pairs] + [p['ov_t'] for p in pairs]).astype(np.float32)
    to = lambda a: torch.from_numpy(a).to(device)
    return dict(xyz=to(xyz), ov=to(ov)[:, None].contiguous(), val=to(val), val2=to(val2), ind=to(ind),
                cu=ops.lengths_to_cu(lens, device), cu_host=cu_host, B=B)


def run_synth(P, cfg, **kw):
    val2 = P['val2'] if cfg.get('use_ratio_test', False) else None
    return check_routes(cfg, P['xyz'], P['ov'], P['val'], val2, P['ind'], P['cu'], P['cu_host'], P['B'], **kw)


@pytest.mark.parametrize("n", [63, 64, 65])
def test_sizes_around_one_wave(device, n):
    rng = np.random.default_rng(n)
    # own side src, the tie, own side tgt -- all with n entries
    P = pack([synth_pair(rng, n, n + 9), synth_pair(rng, n, n), synth_pair(rng, n + 70, n)], device)
    run_synth(P, make_cfg(dict(ALL, use_overlap_as_weights=False)), label=f"n={n} all")
    run_synth(P, make_cfg(dict(threshold_corr=True, remove_outliers_overlap=True, use_overlap_as_weights=True)),
              label=f"n={n} median+overlap_w")


def test_one_entry(device):
    rng = np.random.default_rng(1)
    P = pack([synth_pair(rng, 1, 6), synth_pair(rng, 5, 1), synth_pair(rng, 1, 1)], device)
    P['val2'].zero_()             # one matched point per pair: make it survive the ratio test
    run_synth(P, make_cfg(dict(use_ratio_test=True, threshold_corr=False, remove_outliers_overlap=True, use_lgr=True)),
              label="n=1", well_posed=False)
    # the median of one entry zeroes it (v > v fails): all-zero weights, identity-like finite pose
    new, par, _ = run_synth(P, make_cfg(dict(threshold_corr=True)), label="n=1 median", well_posed=False)
    assert all(float(v.abs().sum()) == 0 for v in new['val'])


@pytest.mark.parametrize("k", [0, 1, "n"])
def test_topk_counts(device, k):
    rng = np.random.default_rng(5)
    pairs = [synth_pair(rng, 40, 47), synth_pair(rng, 90, 33)]
    P = pack(pairs, device)
    k_list = [min(p['src'].shape[0], p['tgt'].shape[0]) if k == "n" else k for p in pairs]
    # pose_residuals refuses an empty set, so the former route cannot run LGR with k = 0
    cfg = make_cfg(dict(use_ratio_test=True, remove_outliers_overlap=True, remove_points_from_val=True, use_lgr=k != 0))
    new, par, _ = run_synth(P, cfg, k_list=k_list, label=f"k={k}", well_posed=k == "n")
    assert [v.numel() for v in new['val']] == k_list


def test_ratio_test_that_zeroes_everything(device):
    """Every ratio fails: all weights are 0 and the pose is what ops.weighted_procrustes gives on zero weights."""
    rng = np.random.default_rng(9)
    P = pack([synth_pair(rng, 50, 61, dead=True), synth_pair(rng, 30, 41)], device)
    cfg = make_cfg(dict(use_ratio_test=True, use_lgr=True))
    new, par, _ = run_synth(P, cfg, label="dead ratio", well_posed=False)
    assert float(new['val'][0].abs().sum()) == 0 and float(new['val'][1].abs().sum()) > 0
    assert torch.isfinite(new['pose']).all()
    one = torch.tensor([0, 50], dtype=torch.int32, device=device)
    zero = ops.weighted_procrustes(new['src_pts'][0].contiguous(), new['tgt_pts'][0].contiguous(),
                                   torch.zeros(50, device=device), one)[0]
    assert torch.equal(new['pose'][0], zero)


def test_duplicates_at_the_median_and_the_topk_boundary(device):
    rng = np.random.default_rng(13)
    pairs = [synth_pair(rng, 64, 80, dup=True), synth_pair(rng, 150, 101, dup=True)]
    P = pack(pairs, device)
    # the duplicated values are really there, on both sides of both cuts
    for p in pairs:
        n = p['val'].size
        srt = np.sort(p['val'])
        assert srt[(n - 1) // 2] == srt[(n - 1) // 2 - 1] == srt[(n - 1) // 2 + 1]
        top = -np.sort(-p['val'])
        assert top[n // 4 - 1] == top[n // 4]
    run_synth(P, make_cfg(dict(threshold_corr=True)), label="dup median")
    # top-k among equal values: the kernel and the replica take the lower position, torch.topk any -- the parent
    # route is compared on values only (check_routes compares its indices on live entries, so it is left out here)
    new, _, rep = run_synth(P, make_cfg(dict(remove_points_from_val=True, use_lgr=True)), label="dup topk",
                            with_parent=False)
    par = parent_loop(make_cfg(dict(remove_points_from_val=True, use_lgr=True)), P['xyz'], P['ov'], P['val'], None,
                      P['ind'], P['cu_host'], P['B'])
    for b in range(P['B']):
        assert torch.equal(par['val'][b], new['val'][b])          # the same multiset in the same (descending) order


def test_workspace_path(device):
    """4 100 entries: above the 4 096 the kernel keeps in LDS."""
    rng = np.random.default_rng(17)
    P = pack([synth_pair(rng, 4100, 4111), synth_pair(rng, 70, 52)], device)
    assert ops._lib.lib().spr_refine_pairs_workspace_bytes(2, 4100) > 0
    run_synth(P, make_cfg(ALL), label="n=4100")


def test_batch_invariance(device):
    """A pair alone and as element 0, 2 and 4 of a five-pair batch: bit-equal outputs."""
    rng = np.random.default_rng(21)
    target = synth_pair(rng, 130, 97)
    others = [synth_pair(rng, 40, 55), synth_pair(rng, 64, 64), synth_pair(rng, 300, 20), synth_pair(rng, 77, 200)]
    cfg = make_cfg(ALL)
    alone = run_synth(pack([target], device), cfg, label="alone")[0]
    for place in (0, 2, 4):
        pairs = list(others)
        pairs.insert(place, target)
        P = pack(pairs, device)
        new = new_route(cfg, P['xyz'], P['ov'], P['val'], P['val2'], P['ind'], P['cu'], P['cu_host'], P['B'])
        assert torch.equal(new['pose'][place], alone['pose'][0])
        for key in ('val', 'ind', 'src_pts', 'tgt_pts'):
            assert torch.equal(new[key][place], alone[key][0]), (place, key)


def test_bad_index_is_a_status_not_a_wild_read(device):
    rng = np.random.default_rng(25)
    P = pack([synth_pair(rng, 20, 31), synth_pair(rng, 45, 28)], device)
    P['ind'][3] = 10 ** 6
    P['ind'][P['cu_host'][3] + 2] = -7
    new = new_route(make_cfg(ALL), P['xyz'], P['ov'], P['val'], P['val2'], P['ind'], P['cu'], P['cu_host'], 2)
    assert new['status'].tolist() == [ops.REFINE_BAD_INDEX, ops.REFINE_BAD_INDEX]
    assert torch.isfinite(new['pose']).all()
    with pytest.raises(ValueError, match="expected"):
        ops.refine_pairs(P['val'][:-1], None, P['ind'], P['ov'], P['xyz'], P['cu'], P['cu_host'], 2)


def test_regtr_refuses_what_the_former_route_could_not_run(device):
    """Before any launch, with a message: overlap weights without the overlap switch; LGR over the unpruned Sinkhorn
    sets of unequal length."""
    rng = np.random.default_rng(29)
    P = pack([synth_pair(rng, 20, 31)], device)
    args = (P['xyz'], P['ov'], P['val'], P['val2'], P['ind'], P['cu'], P['cu_host'], 1, None)
    model = RegTR(make_cfg(dict(use_overlap_as_weights=True)))
    with pytest.raises(ValueError, match="remove_outliers_overlap"):
        model._refined_pose(*args)
    model = RegTR(make_cfg(dict(use_sinkhorn=True, use_lgr=True)))
    with pytest.raises(ValueError, match="equal length"):
        model._refined_pose(*args)
