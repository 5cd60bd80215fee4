"""GPU: surface normals as input features -- the estimator against the float64 restatement of include/spr.h, the
gather + rotate operator against its float64 restatement bit for bit, and the wiring through augment.augment_batch,
Trainer, modelnet.make_pairs, kitti.prepare_pairs and RegTR.  The restatements and every bound are in
tests/normals_cases.py.

Shapes.  Clouds of 840 to 2 340 points: 26 to 74 workgroups of 32 points, none a multiple of 32, so the last group of
lanes of the last wave is partly dead; neighbour rows of 12 to 40 columns cover a lane with 1, 2 and 5 columns and a
row that is no multiple of the 8-lane group or of the 4-column step."""
import numpy as np
import pytest
import torch

import normals_cases as NC
from superpoints_registration_amd import augment, get_config, kitti, modelnet, normals, ops, overlap, synthetic
from superpoints_registration_amd.regtr import RegTR
from superpoints_registration_amd.training import Trainer

pytestmark = pytest.mark.gpu
T = torch.from_numpy
F32 = np.float32


def _bits(t):
    return t.contiguous().view(torch.int32)


def _box():
    return np.ascontiguousarray(synthetic.make_pair(1500, seed=3)[0], dtype=F32)


def _sphere():
    return np.ascontiguousarray(synthetic.make_sphere_pair(1200, seed=1)[0], dtype=F32)


# name -> (clouds, radius, limit)
CASES = {
    "box r0.15 k40": lambda: ([_box()], 0.15, 40),
    "box r0.10 k37": lambda: ([_box()], 0.10, 37),              # rows with 1 and 2 neighbours: the m < 3 branch
    "sphere r0.12 k40": lambda: ([_sphere()], 0.12, 40),
    "sphere r0.12 k37": lambda: ([_sphere()], 0.12, 37),
    "batch box+sphere r0.15 k40": lambda: ([_box(), _sphere()], 0.15, 40),
    "box at (100,-50,20) r0.15 k40": lambda: ([(_box() + np.array([100, -50, 20], F32)).astype(F32)], 0.15, 40),
}


def _search(device, clouds, radius, limit, exact_width=True):
    pts = T(np.concatenate(clouds)).to(device)
    lens = [len(c) for c in clouds]
    cu = ops.lengths_to_cu(lens, device)
    nbr, _ = ops.radius_neighbors(pts, pts, cu, cu, radius, limit, exact_width=exact_width)
    return pts, lens, cu, nbr


def _views(clouds):
    """One viewpoint per cloud, a few extents off its first point and different for every cloud."""
    return np.stack([c[0] + np.array([0.3 + b, 0.2, 3.0], F32) for b, c in enumerate(clouds)]).astype(F32)


# ---- the estimator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", [False, True], ids=["no-view", "view"])
@pytest.mark.parametrize("name", list(CASES))
def test_estimator_against_float64(device, name, view):
    clouds, radius, limit = CASES[name]()
    pts, lens, cu, nbr = _search(device, clouds, radius, limit)
    vp = _views(clouds) if view else None
    nrm, curv = normals.from_neighbors(pts, nbr, cu, None if vp is None else T(vp).to(device), curvature=True)
    ref = NC.check(np.concatenate(clouds), nbr.cpu().numpy(), lens, vp, nrm.cpu().numpy(), curv.cpu().numpy(), name)
    if "r0.10" in name:
        assert int((ref['m'] < 3).sum()) > 0 and int((ref['m'] == 2).sum()) > 0
    # estimate() is the search followed by the same kernel, with lengths or cu, with and without the curvature
    est = normals.estimate(pts, lens, radius, limit, viewpoint=vp)
    est2, curv2 = normals.estimate(pts, cu, radius, limit, viewpoint=None if vp is None else T(vp), curvature=True)
    assert torch.equal(_bits(est), _bits(nrm)) and torch.equal(_bits(est2), _bits(nrm)) and torch.equal(_bits(curv2), _bits(curv))


def test_a_column_slice_is_taken_as_it_is(device):
    clouds, radius, limit = CASES["batch box+sphere r0.15 k40"]()
    pts, lens, cu, wide = _search(device, clouds, radius, limit, exact_width=False)
    assert wide.shape[1] == 40
    for kmax in (12, 1):
        sl = wide[:, :kmax]
        assert sl.stride(0) == 40 and not sl.is_contiguous()
        nrm, curv = normals.from_neighbors(pts, sl, curvature=True)
        again, curv2 = normals.from_neighbors(pts, sl.contiguous(), curvature=True)
        assert torch.equal(_bits(nrm), _bits(again)) and torch.equal(_bits(curv), _bits(curv2))
        if kmax > 1:
            NC.check(np.concatenate(clouds), sl.cpu().numpy(), lens, None, nrm.cpu().numpy(), curv.cpu().numpy(),
                     f"slice {kmax} of 40")
        else:
            assert not bool(nrm.any()) and not bool(curv.any())          # one neighbour, itself: m < 3 everywhere


@pytest.mark.parametrize("name", ["box r0.15 k40", "sphere r0.12 k37"])
def test_shadows_between_valid_entries(device, name):
    """A hand-made matrix: shuffled columns, 30 % of the entries shadows of every kind (N, N + 5, -1, INT_MIN, INT_MAX)."""
    clouds, radius, limit = CASES[name]()
    pts, lens, cu, nbr = _search(device, clouds, radius, limit)
    host = NC.punch_shadows(nbr.cpu().numpy(), len(clouds[0]), seed=5)
    vp = _views(clouds)
    nrm, curv = normals.from_neighbors(pts, T(host).to(device), cu, T(vp).to(device), curvature=True)
    ref = NC.check(clouds[0], host, lens, vp, nrm.cpu().numpy(), curv.cpu().numpy(), f"punched {name}")
    if name.startswith("box"):
        assert int((ref['m'] < 3).sum()) > 0


def test_empty_input_and_empty_rows(device):
    none = torch.empty((0, 3), dtype=torch.float32, device=device)
    nrm, curv = normals.estimate(none, [0], 0.1, curvature=True)
    assert nrm.shape == (0, 3) and curv.shape == (0,)
    nrm = normals.estimate(none, [], 0.1)
    assert nrm.shape == (0, 3)
    pts = T(_box()[:33]).to(device)
    nrm, curv = normals.from_neighbors(pts, torch.empty((33, 0), dtype=torch.int32, device=device), curvature=True)
    assert nrm.shape == (33, 3) and not bool(nrm.any()) and not bool(curv.any())
    assert normals.point_feats([], 0.1) == []


def test_equivariance_under_a_rigid_motion(device):
    """normals(R cloud + t, R view + t) = R normals(cloud, view) on the SAME neighbour matrix, within twice the
    eigenvector bound of every gap row: each side is within one bound of its own float64 reference, and the two
    references differ only by the float32 rounding of the moved points (|p| <= 2 here: d changes by 2^-24 |p| / r
    relative, an order below the bound)."""
    clouds, radius, limit = CASES["box r0.15 k40"]()
    pts, lens, cu, nbr = _search(device, clouds, radius, limit)
    vp = _views(clouds)
    R, t = NC.rot_matrix(11), np.array([0.3, -0.2, 0.1])
    moved = (clouds[0].astype(np.float64) @ R.T + t).astype(F32)
    vp2 = (vp.astype(np.float64) @ R.T + t).astype(F32)
    a = normals.from_neighbors(pts, nbr, cu, T(vp).to(device)).cpu().numpy()
    b = normals.from_neighbors(T(moved).to(device), nbr, cu, T(vp2).to(device)).cpu().numpy()
    ref = NC.check(clouds[0], nbr.cpu().numpy(), lens, vp, a, None, "equivariance, at rest")
    ref2 = NC.check(moved, nbr.cpu().numpy(), lens, vp2, b, None, "equivariance, moved")
    rows = ref['gap_rows'] & ref2['gap_rows'] & ~ref['tie'] & ~ref2['tie']
    assert rows.sum() > 0.9 * len(a)
    diff = np.linalg.norm(b.astype(np.float64) - a.astype(np.float64) @ R.T, axis=1)[rows]
    bound = 2 * ref['K'] * NC.U / np.minimum(ref['gap'], ref2['gap'])[rows] + 4 * 2.0 ** -23
    print(f"equivariance: max |n' - R n| / bound = {(diff / bound).max():.4f}")
    assert np.all(diff <= bound)


# ---- gather + rotate -------------------------------------------------------------------------------------------------
LENS_OUT = [0, 70, 0, 129, 1, 57]          # empty clouds first and between


def _gr_case(c, seed, lens_out=LENS_OUT, n_in=300):
    rng = np.random.default_rng(seed)
    feats = (rng.normal(0, 1, (n_in, c)) * 10.0 ** rng.uniform(-3, 3, (n_in, c))).astype(F32)
    rows = rng.integers(0, n_in, sum(lens_out)).astype(np.int64)
    rot = np.stack([np.eye(3) if b % 3 == 1 else NC.rot_matrix(seed + b) for b in range(len(lens_out))]).astype(F32)
    return feats, rows, rot


@pytest.mark.parametrize("c,cols", [(3, (0,)), (4, (0,)), (4, (1,)), (5, (0,)), (5, (1,)), (5, (2,)), (8, (0,)), (8, (1,)),
                                    (8, (5,)), (8, (0, 5)), (8, (4, 1))])
def test_gather_rotate_is_the_float64_restatement(device, c, cols):
    feats, rows, rot = _gr_case(c, 100 + c)
    cu = ops.lengths_to_cu(LENS_OUT, device)
    want = NC.gather_rotate(feats, rows, LENS_OUT, rot, cols)
    for r_dev, rows_dev in ((T(rot).to(device), T(rows).to(device)), (rot, T(rows.astype(np.int32)).to(device))):
        got = normals.gather_rotate(T(feats).to(device), rows_dev, cu, r_dev, cols)
        assert got.shape == want.shape and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    plain = feats[rows]
    scalar = [j for j in range(c) if not any(s <= j < s + 3 for s in cols)]
    assert np.array_equal(want[:, scalar].view(np.uint32), plain[:, scalar].view(np.uint32))
    assert not np.array_equal(want, plain)
    # identity rotations everywhere: a gather
    eye = np.broadcast_to(np.eye(3, dtype=F32), (len(LENS_OUT), 3, 3))
    got = normals.gather_rotate(T(feats).to(device), T(rows).to(device), cu, eye, cols)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), plain.view(np.uint32))


@pytest.mark.parametrize("c", [3, 4, 5, 8])
def test_gather_rotate_without_triples_is_index_select(device, c):
    feats, rows, rot = _gr_case(c, 200 + c)
    f, r = T(feats).to(device), T(rows).to(device)
    got = normals.gather_rotate(f, r, ops.lengths_to_cu(LENS_OUT, device), rot)
    assert torch.equal(_bits(got), _bits(f.index_select(0, r)))


def test_gather_rotate_of_nothing(device):
    feats, _, rot = _gr_case(4, 7)
    for lens in ([0, 0], []):
        got = normals.gather_rotate(T(feats).to(device), torch.empty((0,), dtype=torch.int64, device=device),
                                    ops.lengths_to_cu(lens, device), rot[:len(lens)], (1,))
        assert got.shape == (0, 4) and got.dtype == torch.float32


# ---- wiring ----------------------------------------------------------------------------------------------------------
def _labelled_batch(device):
    made = [synthetic.make_pair(700 + 130 * i, seed=60 + i, extent=0.45, jitter=0.002, trans=(0.03, -0.02, 0.01)) for i in range(2)]
    batch = {"src_xyz": [T(np.ascontiguousarray(p[0][:650 - 90 * i])).to(device) for i, p in enumerate(made)],
             "tgt_xyz": [T(np.ascontiguousarray(p[1])).to(device) for p in made],
             "pose": T(np.stack([p[2] for p in made])).to(device)}
    overlap.label_batch(batch, 0.0375)
    assert all(int(c.shape[1]) > 0 for c in batch["correspondences"])
    return batch


def _direction_feats(lens, seed, device):
    """[1, nx, ny, nz]: unit directions."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lens:
        v = rng.normal(size=(n, 3))
        out.append(T(np.concatenate([np.ones((n, 1)), v / np.linalg.norm(v, axis=1, keepdims=True)], 1).astype(F32)).to(device))
    return out


@pytest.mark.parametrize("mode", ["small", "large"])
def test_augment_batch_rotates_the_listed_triples(device, mode):
    cfg = get_config("3dmatch")
    cfg.perturb_pose = mode
    base = _labelled_batch(device)
    lens = [int(c.shape[0]) for c in base["src_xyz"] + base["tgt_xyz"]]
    feats = _direction_feats(lens, 9, device)
    with_feats = dict(base, src_point_feats=feats[:2], tgt_point_feats=feats[2:])
    seed, keys = 31, [5, 6]
    bare = augment.augment_batch(base, cfg, seed, keys)
    plain = augment.augment_batch(with_feats, cfg, seed, keys)
    empty = augment.augment_batch(with_feats, cfg, seed, keys, direction_cols=())
    rotated = augment.augment_batch(with_feats, cfg, seed, keys, direction_cols=(1,))
    psrc, swap, perturb = ops.augment_draw(seed, keys, mode)
    changed = 0
    for b in range(2):
        for key in ("src_xyz", "tgt_xyz", "src_overlap", "tgt_overlap", "correspondences"):
            for other in (plain, rotated):
                assert torch.equal(other[key][b], bare[key][b]), key
        for side, own, foreign in (("src", feats[b], feats[2 + b]), ("tgt", feats[2 + b], feats[b])):
            key = f"{side}_point_feats"
            origin = foreign if bool(swap[b]) else own
            perm = rotated[f"{side}_perm"][b]
            assert torch.equal(perm, plain[f"{side}_perm"][b])
            # today's output, bit for bit, with the empty default
            assert torch.equal(_bits(plain[key][b]), _bits(origin[perm])) and torch.equal(_bits(empty[key][b]), _bits(plain[key][b]))
            from_src = (side == "src") != bool(swap[b])                   # the caller's cloud this one came from
            turned = from_src == bool(psrc[b])
            R = perturb[b, :, :3] if turned else np.eye(3, dtype=F32)
            want = NC.gather_rotate(origin.cpu().numpy(), perm.cpu().numpy(), [len(perm)], R[None], (1,))
            got = rotated[key][b].cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (b, side)
            changed += int(turned and not np.array_equal(got, plain[key][b].cpu().numpy()))
    assert torch.equal(_bits(rotated["pose"]), _bits(bare["pose"])) and torch.equal(_bits(plain["pose"]), _bits(bare["pose"]))
    assert changed == 2                                                    # one cloud per pair was perturbed


def test_augment_batch_in_mode_none_rotates_nothing(device):
    cfg = get_config("3dmatch")
    cfg.perturb_pose = "none"
    base = _labelled_batch(device)
    feats = _direction_feats([int(c.shape[0]) for c in base["src_xyz"] + base["tgt_xyz"]], 9, device)
    with_feats = dict(base, src_point_feats=feats[:2], tgt_point_feats=feats[2:])
    plain = augment.augment_batch(with_feats, cfg, 3, [1, 2])
    rotated = augment.augment_batch(with_feats, cfg, 3, [1, 2], direction_cols=(1,))
    for key in ("src_point_feats", "tgt_point_feats"):
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(plain[key], rotated[key]))


def test_make_pairs_carries_and_rotates_the_dataset_normals(device):
    cfg = get_config("modelnet")
    rng = np.random.default_rng(4)
    v = rng.normal(size=(4, 256, 3))
    raw = np.concatenate([rng.uniform(-1, 1, (4, 256, 3)), v / np.linalg.norm(v, axis=2, keepdims=True)], axis=2).astype(F32)
    seed, keys = 17, [3, 4, 5, 6]
    without = modelnet.make_pairs(T(raw).to(device), cfg, seed, keys)
    got = modelnet.make_pairs(T(raw).to(device), cfg, seed, keys, normals=True)
    listed = modelnet.make_pairs([T(r).to(device) for r in raw], cfg, seed, keys, normals=True)
    assert sorted(got) == sorted(list(without) + ["src_point_feats", "tgt_point_feats"])
    for key, val in without.items():
        for a, b in zip(val if isinstance(val, list) else [val], got[key] if isinstance(val, list) else [got[key]]):
            assert a.dtype == b.dtype and torch.equal(a, b), key
    _, tf = modelnet.modelnet_draw(seed, keys, float(cfg.rot_mag), float(cfg.trans_mag))
    eye = np.eye(3, dtype=F32)
    for b in range(4):
        for side, R in (("src", tf[b, :, :3]), ("tgt", eye)):
            idx = got[f"{side}_index"][b].cpu().numpy()
            packed = np.concatenate([np.ones((256, 1), F32), raw[b, :, 3:6]], axis=1)
            want = NC.gather_rotate(packed, idx, [len(idx)], R[None], (1,))
            f = got[f"{side}_point_feats"][b]
            assert f.shape == (717, 4) and np.array_equal(f.cpu().numpy().view(np.uint32), want.view(np.uint32)), (b, side)
            assert torch.equal(_bits(f), _bits(listed[f"{side}_point_feats"][b]))
        assert np.array_equal(got["tgt_point_feats"][b].cpu().numpy()[:, 1:], raw[b][got["tgt_index"][b].cpu().numpy(), 3:6])


def test_trainer_step_with_rotated_normals(device):
    cfg = get_config("3dmatch", in_feats_dim=4)
    model = RegTR(cfg)
    synthetic.fill_parameters(model, seed=0)
    model = model.to(device)
    made = [synthetic.make_pair(900 + 90 * i, seed=40 + i, extent=0.45, jitter=0.002, trans=(0.03, -0.02, 0.01)) for i in range(2)]
    src = [T(np.ascontiguousarray(p[0])).to(device) for p in made]
    tgt = [T(np.ascontiguousarray(p[1])).to(device) for p in made]
    feats = normals.point_feats(src + tgt, 0.05, 40)
    assert all(f.shape == (c.shape[0], 4) for f, c in zip(feats, src + tgt))
    batch = {"src_xyz": src, "tgt_xyz": tgt, "pose": T(np.stack([p[2] for p in made])).to(device),
             "src_point_feats": feats[:2], "tgt_point_feats": feats[2:]}
    seen = []
    hook = model.register_forward_pre_hook(lambda m, args: seen.append(args[0]))
    tr = Trainer(cfg, augment=True, seed=23, direction_cols=(1,)).setup(model)
    losses = tr.train_step(model, batch)
    hook.remove()
    assert len(losses) > 0 and all(bool(torch.isfinite(v).all()) for v in losses.values()), losses
    psrc, swap, perturb = ops.augment_draw(23, tr._pair_keys(2), cfg.perturb_pose)
    for b in range(2):                                   # the model saw the rotated normals
        side = "src" if bool(psrc[b]) != bool(swap[b]) else "tgt"
        origin = feats[b] if bool(psrc[b]) else feats[2 + b]
        perm = seen[0][f"{side}_perm"][b]
        want = NC.gather_rotate(origin.cpu().numpy(), perm.cpu().numpy(), [len(perm)], perturb[b:b + 1, :, :3], (1,))
        assert np.array_equal(seen[0][f"{side}_point_feats"][b].cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_kitti_pair_with_normals_runs_end_to_end(device):
    """Raw scans -> kitti.prepare_pairs(normals_radius=) -> RegTR(in_feats_dim = 4): the features are what
    normals.point_feats gives for the kept points with the sensor origin as the viewpoint, unit or zero, and face the
    sensor."""
    cfg = get_config("kitti", in_feats_dim=4)
    model = RegTR(cfg)
    synthetic.fill_parameters(model, seed=0)
    model = model.to(device).eval()
    src, tgt, pose = synthetic.make_lidar_pair(n=20000, seed=5)
    rng = np.random.default_rng(3)
    raw = [T(np.concatenate([c, rng.random((c.shape[0], 1)).astype(F32)], 1)).to(device) for c in (src, tgt)]
    plain = kitti.prepare_pairs([raw[0]], [raw[1]], cfg, pose=T(pose[None]).to(device))
    batch = kitti.prepare_pairs([raw[0]], [raw[1]], cfg, pose=T(pose[None]).to(device), normals_radius=0.9, normals_limit=37)
    clouds = batch["src_xyz"] + batch["tgt_xyz"]
    assert all(torch.equal(a, b) for a, b in zip(clouds, plain["src_xyz"] + plain["tgt_xyz"])) and "src_point_feats" not in plain
    feats = normals.point_feats(clouds, 0.9, 37, viewpoints=np.zeros((2, 3), F32))
    for f, g, c in zip(feats, batch["src_point_feats"] + batch["tgt_point_feats"], clouds):
        assert f.shape == (c.shape[0], 4) and torch.equal(_bits(f), _bits(g)) and torch.equal(f[:, 0], torch.ones_like(f[:, 0]))
        length = f[:, 1:].double().norm(dim=1)
        assert bool(((length - 1).abs() <= 4 * 2.0 ** -23).logical_or(length == 0).all()) and float((length > 0).float().mean()) > 0.5
        assert bool(((f[:, 1:].double() * -c.double()).sum(1) >= -1e-3 * c.double().norm(dim=1)).all())
    both = kitti.prepare_pairs([raw[0]], [raw[1]], cfg, intensity=True, normals_radius=0.9, normals_limit=37)
    f = both["src_point_feats"][0]
    assert f.shape[1] == 5 and torch.equal(f[:, 1], raw[0][both["src_index"][0], 3]) and torch.equal(_bits(f[:, 2:]), _bits(feats[0][:, 1:]))
    out = model({"src_xyz": batch["src_xyz"], "tgt_xyz": batch["tgt_xyz"], "src_point_feats": feats[:1], "tgt_point_feats": feats[1:]})
    assert out["pose"].shape == (1, 3, 4) and bool(torch.isfinite(out["pose"]).all())
