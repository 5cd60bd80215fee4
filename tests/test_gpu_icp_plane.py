"""GPU: the `icp_plane` subpackage (csrc/icp.hip: k_icp_assoc_plane, k_icp_solve_plane) against the float64 replica of
its contract (tests/icp_plane_replica.py) on the cases of tests/icp_plane_cases.py, and its call sites.

Integers are pinned exactly: corr, count, iterations and status equal the replica's, fitness equals it as float64 --
tests/test_icp_plane_host.py shows that every case's integers survive a relative 2^-40 on every solved pose, so a
disagreement here is the kernel's.  pose64 and inlier_rmse depend on the order of the sums and on the device's sin and
cos: they are held to 16 x the replica's OWN sensitivity to that perturbation, per case (icp_plane_cases.bounds, computed
on the CPU: a few 1e-11 for the cases at the origin, 1.5e-7 / 8.5e-9 for `far`), every case but `far` capped at 1e-9.
The observed maxima are printed and recorded in profiles/icp_plane_bench.txt.
Every pair's outputs are a function of the pair alone: bit-equal alone, inside a batch, inside the reversed batch, on a
second call, and beside a pair that needs more passes (a converged pair is frozen)."""
import numpy as np
import pytest
import torch

import icp_cases as C0
import icp_plane_cases as C
from superpoints_registration_amd import get_config, icp, icp_plane, kitti, normals, synthetic
from superpoints_registration_amd.regtr import RegTR

pytestmark = pytest.mark.gpu
T = torch.from_numpy
KEYS = ("pose", "pose64", "fitness", "inlier_rmse", "iterations", "count", "status")


def run(name, device, max_iter=None, pairs=None, put=lambda t: t, nrm_sign=1.0, kernel=None, kernel_k=None):
    """icp_pairs_raw on the pairs `pairs` (default: all, in order) of a case."""
    c = C.case(name)
    pairs = list(range(len(c["src"]))) if pairs is None else list(pairs)
    dev = lambda key, b, s=1.0: put(T(np.ascontiguousarray(s * c[key][b])).to(device))
    return icp_plane.icp_pairs_raw([dev("src", b) for b in pairs], [dev("tgt", b) for b in pairs],
                                   [dev("nrm", b, np.float32(nrm_sign)) for b in pairs],
                                   put(T(c["pose"][pairs]).to(device)), c["max_dist"],
                                   c["max_iter"] if max_iter is None else max_iter,
                                   kernel=c["kernel"] if kernel is None else kernel,
                                   kernel_k=c["kernel_k"] if kernel_k is None else kernel_k)


def pair_of(out, b):
    """Pair b of a result, as host arrays."""
    d = {k: out[k][b].cpu().numpy() for k in KEYS if k in out}
    d["corr"] = out["corr"][b].cpu().numpy()
    return d


def same_bits(a, b, what):
    for k in KEYS + ("corr",):
        if k not in a and k not in b:
            continue
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
    pose_bound, rmse_bound = C.bounds(name)
    print(f"icp_plane {name}: max |pose64 - replica| = {worst_pose:.3e} (bound {pose_bound:.3e}), "
          f"max |inlier_rmse - replica| = {worst_rmse:.3e} (bound {rmse_bound:.3e})")
    if exact_pose:
        assert worst_pose == 0.0, name
    assert worst_pose <= pose_bound and worst_rmse <= rmse_bound, (name, worst_pose, worst_rmse)


@pytest.mark.parametrize("name", C.CASES)
def test_matches_the_replica(device, name):
    check_against_replica(name, run(name, device), C.replica(name))


def test_the_flat_patch_keeps_its_pose_bit_for_bit(device):
    g = pair_of(run("plane", device), 0)
    assert int(g["iterations"]) == 1 and int(g["count"]) == 257
    assert g["pose64"].tobytes() == np.ascontiguousarray(C.case("plane")["pose"][0]).tobytes()


@pytest.mark.parametrize("name", ["corner_slide", "ragged", "zero_normals", "robust_huber", "robust_tukey", "far"])
def test_negated_normals_give_the_same_bits(device, name):
    a, b = run(name, device), run(name, device, nrm_sign=-1.0)
    for p in range(len(C.case(name)["src"])):
        same_bits(pair_of(a, p), pair_of(b, p), f"{name} pair {p}, normals negated")


@pytest.mark.parametrize("name", ["corner_slide", "ragged", "robust_tukey", "nonfinite"])
def test_zero_iterations_is_the_point_to_point_evaluation(device, name):
    """max_iter = 0: E(T_0) is that of the `icp` subpackage, bit for bit (a NaN normal refuses a pair only here)."""
    c = C.case(name)
    out = run(name, device, max_iter=0)
    ref = icp.icp_pairs_raw([T(x).to(device) for x in c["src"]], [T(x).to(device) for x in c["tgt"]], T(c["pose"]),
                            c["max_dist"], 0)
    for p in range(len(c["src"])):
        if name == "nonfinite" and p == 1:
            assert int(out["status"][p]) == -1 and int(ref["status"][p]) == 0
            continue
        same_bits(pair_of(out, p), pair_of(ref, p), f"{name} pair {p}, max_iter = 0")
    assert not bool(out["iterations"].any())
    check_against_replica(name, out, C.replica(name, 0.0, 0), exact_pose=True)


@pytest.mark.parametrize("name", ["corner_slide", "ragged", "robust_l2"])
def test_huber_above_every_residual_is_l2(device, name):
    k = 4.0 * C.case(name)["max_dist"]                  # |r| <= |a - b| |n| < max_dist (1 + 1e-6): the normals are unit
    assert all(float(np.abs(np.linalg.norm(n, axis=1) - 1).max(initial=0)) < 1e-6 for n in C.case(name)["nrm"])
    a, b = run(name, device, kernel="l2"), run(name, device, kernel="huber", kernel_k=k)
    for p in range(len(C.case(name)["src"])):
        same_bits(pair_of(a, p), pair_of(b, p), f"{name} pair {p}, huber with k = {k}")


def test_every_pair_is_independent_of_its_batch(device):
    n = len(C.case("ragged")["src"])
    whole, rev = run("ragged", device), run("ragged", device, pairs=range(n - 1, -1, -1))
    for b in range(n):
        alone = pair_of(run("ragged", device, pairs=[b]), 0)
        same_bits(alone, pair_of(whole, b), f"ragged pair {b} alone / in the batch")
        same_bits(alone, pair_of(rev, n - 1 - b), f"ragged pair {b} alone / in the reversed batch")


@pytest.mark.parametrize("name", ["ragged", "corner_slide", "robust_huber"])
def test_a_second_call_gives_the_same_bits(device, name):
    a, b = run(name, device), run(name, device)
    for p in range(len(C.case(name)["src"])):
        same_bits(pair_of(a, p), pair_of(b, p), f"{name} pair {p}, second call")


def test_a_converged_pair_is_frozen(device):
    """The snap start beside the slide start in one call (slide's max_dist): snap stops first and keeps the outputs of
    its solo run while slide goes on; both orders."""
    s, t = C.case("corner_snap"), C.case("corner_slide")
    md = t["max_dist"]

    def call(cases):
        return icp_plane.icp_pairs_raw([T(c["src"][0]).to(device) for c in cases], [T(c["tgt"][0]).to(device) for c in cases],
                                       [T(c["nrm"][0]).to(device) for c in cases],
                                       T(np.concatenate([c["pose"] for c in cases])), md, 30)
    snap, slide = pair_of(call([s]), 0), pair_of(call([t]), 0)
    assert int(snap["iterations"]) < int(slide["iterations"]) == C.replica("corner_slide")[0]["iterations"]
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
        icp_plane.icp_pairs([T(x).to(device) for x in c["src"]], [T(x).to(device) for x in c["tgt"]],
                            [T(x).to(device) for x in c["nrm"]], c["pose"], c["max_dist"])


def test_estimated_normals_are_returned_and_used(device):
    """The convenience form: normals.estimate on the packed targets, returned as 'tgt_normals'; the same call by hand."""
    c = C.case("ragged")
    src, tgt = [T(c["src"][b]).to(device) for b in (0, 2)], [T(c["tgt"][b]).to(device) for b in (0, 2)]
    out = icp_plane.icp_pairs(src, tgt, None, c["pose"][[0, 2]], c["max_dist"], normals_radius=0.6, normals_limit=16)
    nrm = normals.estimate(torch.cat(tgt), [len(t) for t in tgt], 0.6, 16)
    assert torch.equal(torch.cat(out["tgt_normals"]), nrm) and [len(n) for n in out["tgt_normals"]] == [300, 275]
    ref = icp_plane.icp_pairs(src, tgt, list(torch.split(nrm, [300, 275])), c["pose"][[0, 2]], c["max_dist"])
    assert sorted(set(out) - set(ref)) == ["tgt_normals"] and sorted(ref) == sorted(KEYS[:-1] + ("corr",))
    for k in KEYS[:-1]:
        assert torch.equal(out[k], ref[k]), k
    # estimated normals are blurred at the corner's edges: nearer the ground truth than the start (0.052), not at it
    assert C.pose_error(out["pose64"][0].cpu().numpy()) < 0.5 * C.pose_error(c["pose"][0])


def _scans(device):
    """Two synthetic 4-column scans of about 2 000 points on a ground plane and two walls, and a pose near the one that
    relates them."""
    rng = np.random.default_rng(41)
    gt = C0.rigid((0, 0, 1), 4.0, (0.8, -0.3, 0.05))
    u = rng.uniform(-12, 12, (2000, 2))
    src = np.concatenate([np.column_stack([u[:1000], np.full(1000, -1.5)]),
                          np.column_stack([u[1000:1500, 0], np.full(500, 9.0), 0.2 * u[1000:1500, 1]]),
                          np.column_stack([np.full(500, -10.0), u[1500:, 0], 0.2 * u[1500:, 1]])])
    tgt = (C0.apply(gt, src)[rng.permutation(2000)[:1900]] + rng.normal(0, 0.005, (1900, 3)))
    refl = lambda n: rng.uniform(0, 1, (n, 1))
    s4, t4 = np.hstack([src, refl(2000)]).astype(np.float32), np.hstack([tgt, refl(1900)]).astype(np.float32)
    init = C0.R.compose(C0.rigid((0, 1, 0), 0.1, (0.03, -0.02, 0.01)), gt).astype(np.float32)
    return T(s4).to(device), T(t4).to(device), T(init)[None].to(device)


def test_prepare_pairs_refines_by_point_to_plane_on_the_raw_scans(device):
    s4, t4, pose = _scans(device)
    cfg = get_config("kitti")
    before = kitti.prepare_pairs([s4], [t4], cfg, pose=pose, refine_pose=True, icp_distance=0.5, icp_max_iter=30)
    default = kitti.prepare_pairs([s4], [t4], cfg, pose=pose, refine_pose=True, icp_distance=0.5, icp_max_iter=30,
                                  icp_method="point_to_point")
    out = kitti.prepare_pairs([s4], [t4], cfg, pose=pose, refine_pose=True, icp_distance=0.5, icp_max_iter=30,
                              icp_method="point_to_plane", icp_normals_radius=1.5, icp_kernel="huber", icp_kernel_k=0.05)
    src, tgt = s4[:, :3].contiguous(), t4[:, :3].contiguous()
    nrm = normals.estimate(tgt, [len(tgt)], 1.5, 40, viewpoint=torch.zeros((1, 3), device=device))
    ref = icp_plane.icp_pairs([src], [tgt], [nrm], pose, 0.5, 30, kernel="huber", kernel_k=0.05)
    assert torch.equal(out["pose"], ref["pose"]) and out["pose"].dtype == torch.float32
    assert torch.equal(out["icp_fitness"], ref["fitness"]) and torch.equal(out["icp_rmse"], ref["inlier_rmse"])
    assert 0 < int(ref["iterations"][0]) < 30 and float(ref["fitness"][0]) > 0.9
    assert not torch.equal(out["pose"], before["pose"])
    assert sorted(out) == sorted(before) == sorted(default)
    for k in before:                                     # the default path is what it was: bit for bit, key for key
        a, b = before[k], default[k]
        assert all(torch.equal(x, y) for x, y in zip(a, b)) if isinstance(a, list) else torch.equal(a, b), k
    for k in ("src_xyz", "tgt_xyz", "src_index", "tgt_index"):
        assert all(torch.equal(a, b) for a, b in zip(out[k], before[k])), k


def test_regtr_polishes_its_pose_by_point_to_plane(device):
    src, tgt, _ = synthetic.make_pair(1024, seed=3, extent=0.6, jitter=0.002)
    batch = {"src_xyz": [T(src).to(device)], "tgt_xyz": [T(tgt).to(device)]}
    outs = []
    for over in (dict(icp_refine=True, icp_distance=0.05), dict(icp_refine=True, icp_distance=0.05, icp_method="point_to_point"),
                 dict(icp_refine=True, icp_distance=0.05, icp_method="point_to_plane", icp_kernel="tukey", icp_kernel_k=0.02)):
        model = RegTR(get_config("3dmatch", **over))
        synthetic.fill_parameters(model, seed=0)
        outs.append(model.to(device).eval()(dict(batch)))
    before, default, out = outs
    assert sorted(before) == sorted(default) == sorted(out)            # forward returns the same keys as before
    for k in ("pose", "pose_coarse", "icp_fitness", "icp_rmse"):
        assert torch.equal(before[k], default[k]), k
    assert torch.equal(out["pose_coarse"], before["pose_coarse"])
    radius = 2.5 * get_config("3dmatch").first_subsampling_dl           # icp_normals_radius = None
    ref = icp_plane.icp_pairs(batch["src_xyz"], batch["tgt_xyz"], None, out["pose_coarse"], 0.05, 30, kernel="tukey",
                              kernel_k=0.02, normals_radius=radius)
    assert torch.equal(out["pose"], ref["pose"])
    assert torch.equal(out["icp_fitness"], ref["fitness"]) and torch.equal(out["icp_rmse"], ref["inlier_rmse"])
