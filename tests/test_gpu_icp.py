"""GPU: the `icp` subpackage (csrc/icp.hip) against the float64 replica of its contract (tests/icp_replica.py) on the
cases of tests/icp_cases.py, and its two call sites.

Integers are pinned exactly: corr, count, iterations and status equal the replica's, fitness equals it as float64 --
tests/test_icp_host.py shows that the cases' integers survive a relative 2^-40 on every solved pose, so a disagreement
here is the kernel's.  With max_iter = 0 that holds for any input, because T_0 is given.  pose64 and inlier_rmse depend
on the order of the moment sums and on the SVD (one-sided Jacobi here, LAPACK there): they are held to 16 x the largest
difference measured on the MI355X over all cases (profiles/icp_bench.txt: pose64 MEASURED_POSE, inlier_rmse
MEASURED_RMSE), which may never exceed 1e-9 -- the replica's own sensitivity to the 2^-40 perturbation is 1.3e-12
(5e-9 for `far`, whose coordinates are 1e4), so anything near 1e-9 is a bug, not rounding.
Every pair's outputs are a function of the pair alone: bit-equal alone, inside a batch, inside the reversed batch, on
a second call, and beside a pair that needs more passes (a converged pair is frozen)."""
import numpy as np
import pytest
import torch

import icp_cases as C
from superpoints_registration_amd import get_config, icp, kitti, synthetic
from superpoints_registration_amd.regtr import RegTR

pytestmark = pytest.mark.gpu
T = torch.from_numpy
MEASURED_POSE = 1.973e-14      # largest |pose64 - replica| over all cases, MI355X (profiles/icp_bench.txt): `far`
MEASURED_RMSE = 4.626e-13      # largest |inlier_rmse - replica|: `far`; every other case <= 2.9e-15 / 1.9e-16
POSE_BOUND = min(16 * MEASURED_POSE, 1e-9)
RMSE_BOUND = min(16 * MEASURED_RMSE, 1e-9)
KEYS = ("pose", "pose64", "fitness", "inlier_rmse", "iterations", "count", "status")


def run(name, device, max_iter=None, pairs=None, max_dist=None, put=lambda t: t):
    """icp_pairs_raw on the pairs `pairs` (default: all, in order) of a case."""
    c = C.case(name)
    pairs = list(range(len(c["src"]))) if pairs is None else list(pairs)
    return icp.icp_pairs_raw([put(T(c["src"][b]).to(device)) for b in pairs], [put(T(c["tgt"][b]).to(device)) for b in pairs],
                             put(T(c["pose"][pairs]).to(device)), c["max_dist"] if max_dist is None else max_dist,
                             c["max_iter"] if max_iter is None else max_iter)


def pair_of(out, b):
    """Pair b of a result, as host arrays."""
    d = {k: out[k][b].cpu().numpy() for k in KEYS}
    d["corr"] = out["corr"][b].cpu().numpy()
    return d


def same_bits(a, b, what):
    for k in KEYS + ("corr",):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: {k} differs"


def check_against_replica(name, out, ref, exact_pose=False):
    worst_pose = worst_rmse = 0.0
    for b, r in enumerate(ref):
        g = pair_of(out, b)
        what = f"{name} pair {b}"
        assert int(g["status"]) == r["status"], what
        assert np.array_equal(g["corr"], r["corr"]), f"{what}: corr differs in {int((g['corr'] != r['corr']).sum())} rows"
        assert int(g["count"]) == r["count"] and int(g["iterations"]) == r["iterations"], \
            (what, int(g["count"]), r["count"], int(g["iterations"]), r["iterations"])
        assert float(g["fitness"]) == r["fitness"], what
        assert g["pose"].tobytes() == g["pose64"].astype(np.float32).tobytes(), f"{what}: pose is not pose64 rounded"
        if r["status"] == 0:
            worst_pose = max(worst_pose, float(np.abs(g["pose64"] - r["pose64"]).max()))
            worst_rmse = max(worst_rmse, abs(float(g["inlier_rmse"]) - r["inlier_rmse"]))
        else:
            assert g["pose64"].tobytes() == np.ascontiguousarray(r["pose64"]).tobytes(), f"{what}: pose is not pose_init"
    print(f"icp {name}: max |pose64 - replica| = {worst_pose:.3e}, max |inlier_rmse - replica| = {worst_rmse:.3e}")
    if exact_pose:
        assert worst_pose == 0.0, name
    assert worst_pose <= POSE_BOUND and worst_rmse <= RMSE_BOUND, (name, worst_pose, worst_rmse)


@pytest.mark.parametrize("name", C.CASES)
def test_matches_the_replica(device, name):
    check_against_replica(name, run(name, device), C.replica(name))


@pytest.mark.parametrize("name", C.CASES)
def test_pure_evaluation_matches_the_replica(device, name):
    """max_iter = 0: T_0 is given, so the integers hold for any input and pose64 is pose_init itself."""
    out = run(name, device, max_iter=0)
    check_against_replica(name, out, C.replica(name, 0.0, 0), exact_pose=True)
    assert not bool(out["iterations"].any())


def test_evaluate_is_the_zero_iteration_form(device):
    c = C.case("slide")
    src, tgt, pose = [T(c["src"][0]).to(device)], [T(c["tgt"][0]).to(device)], T(c["pose"])
    a, b = icp.evaluate(src, tgt, pose, c["max_dist"]), icp.icp_pairs(src, tgt, pose, c["max_dist"], max_iter=0)
    assert sorted(a) == sorted(b) == sorted(KEYS[:-1] + ("corr",))
    for k in KEYS[:-1]:
        assert torch.equal(a[k], b[k])
    assert int(a["count"][0]) == 633 and torch.equal(a["pose64"].cpu(), pose)


def test_every_pair_is_independent_of_its_batch(device):
    n = len(C.case("ragged")["src"])
    whole, rev = run("ragged", device), run("ragged", device, pairs=range(n - 1, -1, -1))
    for b in range(n):
        alone = pair_of(run("ragged", device, pairs=[b]), 0)
        same_bits(alone, pair_of(whole, b), f"ragged pair {b} alone / in the batch")
        same_bits(alone, pair_of(rev, n - 1 - b), f"ragged pair {b} alone / in the reversed batch")


@pytest.mark.parametrize("name", ["ragged", "slide"])
def test_a_second_call_gives_the_same_bits(device, name):
    a, b = run(name, device), run(name, device)
    for p in range(len(C.case(name)["src"])):
        same_bits(pair_of(a, p), pair_of(b, p), f"{name} pair {p}, second call")


def test_a_converged_pair_is_frozen(device):
    """snap's pair beside slide's in one call (slide's max_dist): snap stops first and keeps the outputs of its solo run
    while slide goes on; both orders."""
    s, t = C.case("snap"), C.case("slide")
    md = t["max_dist"]

    def call(cases):
        return icp.icp_pairs_raw([T(c["src"][0]).to(device) for c in cases], [T(c["tgt"][0]).to(device) for c in cases],
                                 T(np.concatenate([c["pose"] for c in cases])), md, 30)
    snap, slide = pair_of(call([s]), 0), pair_of(call([t]), 0)
    assert int(snap["iterations"]) < int(slide["iterations"]) == C.replica("slide")[0]["iterations"]
    for order, at in (([s, t], 0), ([t, s], 1)):          # at: where snap stands
        both = call(order)
        same_bits(snap, pair_of(both, at), "snap beside slide")
        same_bits(slide, pair_of(both, 1 - at), "slide beside snap")


def test_a_nonfinite_pair_is_refused_alone(device):
    out = run("nonfinite", device)
    assert out["status"].tolist() == [0, -1, 0]
    for b in (0, 2):
        same_bits(pair_of(run("nonfinite", device, pairs=[b]), 0), pair_of(out, b), f"pair {b} beside the refused one")
    c = C.case("nonfinite")
    with pytest.raises(ValueError, match="pair 1"):
        icp.icp_pairs([T(x).to(device) for x in c["src"]], [T(x).to(device) for x in c["tgt"]], c["pose"], c["max_dist"])
    bad_pose = c["pose"].copy()
    bad_pose[2, 1, 3] = np.inf
    with pytest.raises(ValueError, match=r"pair 1 \(and in pairs \[2\]\)"):
        icp.icp_pairs([T(x).to(device) for x in c["src"]], [T(x).to(device) for x in c["tgt"]], bad_pose, c["max_dist"])


def _scans(device):
    """Two synthetic 4-column scans of about 2 000 points and a pose near the one that relates them."""
    rng = np.random.default_rng(41)
    gt = C.rigid((0, 0, 1), 4.0, (0.8, -0.3, 0.05))
    src = np.concatenate([rng.uniform(-12, 12, (2000, 2)), rng.uniform(-1.5, 1.0, (2000, 1))], 1)
    tgt = (C.apply(gt, src)[rng.permutation(2000)[:1900]] + rng.normal(0, 0.01, (1900, 3)))
    refl = lambda n: rng.uniform(0, 1, (n, 1))
    s4, t4 = np.hstack([src, refl(2000)]).astype(np.float32), np.hstack([tgt, refl(1900)]).astype(np.float32)
    init = C.R.compose(C.rigid((0, 1, 0), 0.1, (0.03, -0.02, 0.01)), gt).astype(np.float32)
    return T(s4).to(device), T(t4).to(device), T(init)[None].to(device)


def test_prepare_pairs_refines_the_pose_on_the_raw_scans(device):
    s4, t4, pose = _scans(device)
    cfg = get_config("kitti")
    plain = kitti.prepare_pairs([s4], [t4], cfg, pose=pose)
    out = kitti.prepare_pairs([s4], [t4], cfg, pose=pose, refine_pose=True, icp_distance=0.2, icp_max_iter=200)
    ref = icp.icp_pairs([s4[:, :3].contiguous()], [t4[:, :3].contiguous()], pose, 0.2, 200)
    assert torch.equal(out["pose"], ref["pose"]) and out["pose"].dtype == torch.float32
    assert torch.equal(out["icp_fitness"], ref["fitness"]) and torch.equal(out["icp_rmse"], ref["inlier_rmse"])
    assert 0 < int(ref["iterations"][0]) < 200 and float(ref["fitness"][0]) > 0.9
    assert float(ref["inlier_rmse"][0]) < float(icp.evaluate([s4[:, :3].contiguous()], [t4[:, :3].contiguous()], pose,
                                                              0.2)["inlier_rmse"][0])
    assert sorted(set(out) - set(plain)) == ["icp_fitness", "icp_rmse"] and plain["pose"] is pose
    for k in ("src_xyz", "tgt_xyz", "src_index", "tgt_index"):
        assert all(torch.equal(a, b) for a, b in zip(out[k], plain[k])), k


def test_regtr_polishes_its_pose(device):
    src, tgt, _ = synthetic.make_pair(1024, seed=3, extent=0.6, jitter=0.002)
    batch = {"src_xyz": [T(src).to(device)], "tgt_xyz": [T(tgt).to(device)]}
    outs = []
    for over in ({}, dict(icp_refine=True, icp_distance=0.05, icp_max_iter=30)):
        model = RegTR(get_config("3dmatch", **over))
        synthetic.fill_parameters(model, seed=0)
        outs.append(model.to(device).eval()(dict(batch)))
    plain, out = outs
    assert "pose_coarse" not in plain and "icp_fitness" not in plain
    assert torch.equal(out["pose_coarse"], plain["pose"])
    ref = icp.icp_pairs(batch["src_xyz"], batch["tgt_xyz"], out["pose_coarse"], 0.05, 30)
    assert torch.equal(out["pose"], ref["pose"])
    assert torch.equal(out["icp_fitness"], ref["fitness"]) and torch.equal(out["icp_rmse"], ref["inlier_rmse"])
