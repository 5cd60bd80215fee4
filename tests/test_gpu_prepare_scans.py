"""GPU: ops.prepare_scans / kitti.prepare_pairs -- the KITTI loader's point path (data_loaders/kitti_pred.py:203-230)
for all raw scans of a batch in one library call.

Anchor 1: per cloud, oracle.torch_oracle.voxel_down_sample (the pinned restatement of kiss-icp's filter) followed by
the loader's two numpy masks in float64, written as the loader writes them.  The oracle returns points, not indices;
a kept point is the first of its voxel and every point with the same bits lies in the same voxel, so its index is the
first occurrence of its bits in the cloud.  Anchor 2: the per-cloud loop of ops.voxel_downsample plus torch masks (the
route the library offered before).  xyz, idx and out_cu must be equal exactly.

Every shape is there because a specific thing breaks at it (the comment beside each case).  The compaction works in
tiles of 1024 points, four per thread of a 256-thread workgroup."""
import ctypes
import fractions
import functools

import numpy as np
import pytest
import torch

from oracle.torch_oracle import voxel_down_sample
from superpoints_registration_amd import _lib, get_config, kitti, ops, synthetic
from superpoints_registration_amd.regtr import RegTR
from workspace_arena import GUARD, GUARD_BYTE

pytestmark = pytest.mark.gpu


# ---- the anchors ------------------------------------------------------------------------------------------------------
def _first_occurrence(cloud, kept):
    """Index in `cloud` [n,3] of every row of `kept` (rows of cloud, see the module docstring)."""
    first = {}
    for i, row in enumerate(np.ascontiguousarray(cloud)):
        first.setdefault(row.tobytes(), i)
    return np.array([first[row.tobytes()] for row in np.ascontiguousarray(kept)], dtype=np.int64).reshape(-1)


def loader_route(clouds, voxel, crop_radius, remove_ground):
    """kitti_pred.py:203-230 per cloud -> (xyz [m,3] f32, out_cu list, idx [m])."""
    xyz, idx, cu = [], [], [0]
    for c in clouds:
        c = np.ascontiguousarray(c[:, :3])
        pcd_input = voxel_down_sample(c, voxel)
        where = _first_occurrence(c, pcd_input)
        assert np.all(np.diff(where) > 0)
        pcd_input = pcd_input.astype(np.float64)                 # kiss-icp hands back float64 points
        if crop_radius > 0:
            radius = np.sqrt(pcd_input[:, 0]**2 + pcd_input[:, 1]**2)
            where = where[radius <= crop_radius]
            pcd_input = pcd_input[radius <= crop_radius]
        if remove_ground:
            where = where[pcd_input[:, 2] > -1]
            pcd_input = pcd_input[pcd_input[:, 2] > -1]
        xyz.append(pcd_input.astype(np.float32))
        idx.append(where)
        cu.append(cu[-1] + len(where))
    return np.concatenate(xyz).reshape(-1, 3), cu, np.concatenate(idx)


def per_cloud_route(clouds, voxel, crop_radius, remove_ground, device):
    """The route without the batched call: ops.voxel_downsample and torch masks, cloud by cloud (device tensors)."""
    out = []
    for c in clouds:
        v = ops.voxel_downsample(torch.from_numpy(np.ascontiguousarray(c[:, :3])).to(device), voxel)
        d = v.double()
        if crop_radius > 0:
            keep = torch.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2) <= crop_radius
            v, d = v[keep], d[keep]
        if remove_ground:
            v = v[d[:, 2] > -1]
        out.append(v)
    return out


def run(clouds, voxel, crop_radius, remove_ground, device):
    pts = torch.from_numpy(np.concatenate(clouds)).to(device)
    cu = ops.lengths_to_cu([len(c) for c in clouds], device)
    xyz, out_cu, idx = ops.prepare_scans(pts, cu, voxel, crop_radius, remove_ground)
    assert xyz.dtype == torch.float32 and idx.dtype == torch.int32 and isinstance(out_cu, list)
    return xyz.cpu().numpy(), out_cu, idx.cpu().numpy()


def check(clouds, voxel, crop_radius, remove_ground, device):
    xyz, out_cu, idx = run(clouds, voxel, crop_radius, remove_ground, device)
    ref_xyz, ref_cu, ref_idx = loader_route(clouds, voxel, crop_radius, remove_ground)
    assert out_cu == ref_cu
    assert np.array_equal(idx, ref_idx)
    assert xyz.shape == ref_xyz.shape and np.array_equal(xyz.view(np.uint32), ref_xyz.view(np.uint32))
    loop = per_cloud_route(clouds, voxel, crop_radius, remove_ground, device)
    assert [0] + list(np.cumsum([len(v) for v in loop])) == out_cu
    assert np.array_equal(torch.cat(loop).cpu().numpy().view(np.uint32).reshape(-1, 3), xyz.view(np.uint32))
    return xyz, out_cu, idx


# ---- shapes -------------------------------------------------------------------------------------------------------------
def _uniform(lens, extent, seed, zlo=-3.0, zhi=3.0):
    rng = np.random.default_rng(seed)
    out = []
    for n in lens:
        p = rng.uniform(-extent, extent, (n, 3))
        p[:, 2] = rng.uniform(zlo, zhi, n)
        out.append(p.astype(np.float32))
    return out


def _distinct_voxels(n, voxel, rng, span=40):
    """n points, each the centre of a voxel of its own, in random order."""
    cells = rng.choice(span ** 3, size=n, replace=False)
    ijk = np.stack([cells // span ** 2, cells // span % span, cells % span], 1) - span // 2
    # voxel index t (truncation toward zero) is met at (t + 0.5) voxel for t >= 0 and (t - 0.5) voxel for t < 0
    return ((ijk + np.where(ijk >= 0, 0.5, -0.5)) * voxel).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _big():
    return tuple(_uniform([30000] * 4, 60.0, 7))


def _cases():
    rng = np.random.default_rng(11)
    wrap = [_distinct_voxels(1 + k % 8, 0.3, rng) for k in range(256)]
    one_voxel = (rng.uniform(0.01, 0.29, (1000, 3))).astype(np.float32)
    own = _distinct_voxels(5000, 0.3, rng)
    same = _uniform([700], 2.0, 5)[0]
    raw4 = [np.concatenate([c, np.full((len(c), 1), np.nan, np.float32)], 1) for c in _uniform([300, 1100], 3.0, 6)]
    return {
        "one_point": ([np.array([[0.5, -0.25, 2.0]], np.float32)], 0.3),
        # cloud boundaries inside a workgroup's 256 threads and inside a tile, tile boundaries inside a cloud
        "lens_1_257_1000": (_uniform([1, 257, 1000], 2.0, 1), 0.3),
        "lens_255_1_256_2": (_uniform([255, 1, 256, 2], 2.0, 2), 0.3),
        # a cloud boundary exactly on a tile boundary; n a whole number of tiles (the prefix one past the last tile)
        "lens_1024_1024_1": (_uniform([1024, 1024, 1], 2.0, 3), 0.3),
        "lens_1024_1024": (_uniform([1024, 1024], 2.0, 4), 0.3),
        # table regions at load 1/2 and of 2..16 slots: a probe that reaches a region's end must wrap inside it
        "lens_1_to_8_distinct": (wrap, 0.3),
        # every thread of four workgroups fights for one slot
        "one_voxel_1000": ([one_voxel], 0.3),
        "own_voxel_5000": ([own], 0.3),
        # equal voxels in different clouds must not merge
        "same_points_twice": ([same, same.copy()], 0.3),
        # truncation toward zero: all of these are voxel (0, 0, 0); floor would make three voxels
        "trunc_toward_zero": ([np.array([[0.1, 0.1, 0.1], [-0.1, -0.1, -0.1], [-0.1, 0.1, 0.1], [0.4, 0.1, 0.1]],
                                        np.float32)], 0.3),
        # raw records: the 4th column holds NaN and must never be read into anything
        "stride4_nan_reflectance": (raw4, 0.3),
        "four_clouds_30000": (list(_big()), 0.3),
    }


CASES = _cases()


@pytest.mark.parametrize("crop_radius,remove_ground", [(0.0, False), (1.5, True)], ids=["plain", "crop_ground"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_the_loader_and_the_per_cloud_route(device, name, crop_radius, remove_ground):
    clouds, voxel = CASES[name]
    if name == "four_clouds_30000" and crop_radius > 0:
        crop_radius = 50.0
    xyz, out_cu, idx = check(clouds, voxel, crop_radius, remove_ground, device)
    if crop_radius == 0.0:
        if name == "one_voxel_1000":
            assert idx.tolist() == [0] and out_cu == [0, 1]
        if name == "trunc_toward_zero":
            assert idx.tolist() == [0, 3]
        if name in ("own_voxel_5000", "lens_1_to_8_distinct"):
            assert out_cu[-1] == sum(len(c) for c in clouds)
        if name == "same_points_twice":
            h = out_cu[1]
            assert out_cu[2] == 2 * h and np.array_equal(idx[:h], idx[h:])


# ---- order of the steps, boundaries --------------------------------------------------------------------------------------
def test_a_voxel_whose_first_point_is_masked_yields_nothing(device):
    """The masks act on the filter's output (kitti_pred.py:203 before :221 and :228): the second point of the voxel,
    which would pass the mask, never appears."""
    far_first = np.array([[6.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 25.0]], np.float32)       # voxel 20: 0, 0, 1
    xyz, out_cu, idx = check([far_first], 20.0, 5.0, False, device)
    assert idx.tolist() == [2]
    low_first = np.array([[0.0, 0.0, -2.0], [0.0, 0.0, -0.5], [30.0, 0.0, 0.0]], np.float32)
    xyz, out_cu, idx = check([low_first], 20.0, 0.0, True, device)
    assert idx.tolist() == [2]
    assert check([far_first[::-1].copy()], 20.0, 5.0, False, device)[2].tolist() == [0, 1]    # the control


def test_mask_boundaries(device):
    """radius <= crop_radius keeps the 3-4-5 triangle at 5.0; z > -1 is strict."""
    above = np.nextafter(np.float32(-1.0), np.float32(0.0))
    pts = np.array([[3.0, 4.0, 7.0], [-4.0, 3.0, -1.0], [40.0, 0.0, above], [80.0, 0.0, -1.0]], np.float32)
    assert check([pts], 0.3, 5.0, False, device)[2].tolist() == [0, 1]
    assert check([pts], 0.3, 0.0, True, device)[2].tolist() == [0, 2]
    assert check([pts], 0.3, float(np.nextafter(5.0, 0.0)), True, device)[2].tolist() == []


def _fl(q: fractions.Fraction) -> float:
    return q.numerator / q.denominator           # int / int is correctly rounded: the float64 nearest to q


def test_radius_rounds_once_per_operation(device):
    """The predicate must round like numpy's sqrt(x**2 + y**2): a contracted fma(x, x, y*y) must not move a point across
    the radius.  Searched on the host for a float32 (x, y) whose contracted sum exceeds the two-rounding sum: there is
    none -- a float32 has a 24-bit significand, so x*x and y*y are EXACT in float64 (48 bits) and both forms round
    the same exact sum once; the search below states that, and would hand its find to the check if it had one.  What
    can still differ is the rounding of the sum and of the square root, so for a sample of points the crop radius is
    set to the point's own numpy radius (kept) and to the float64 just below it (dropped)."""
    rng = np.random.default_rng(3)
    xy = rng.uniform(-80.0, 80.0, (4000, 2)).astype(np.float32)
    found = []
    for x, y in xy:
        fx, fy = fractions.Fraction(float(x)), fractions.Fraction(float(y))
        two = _fl(fractions.Fraction(_fl(fx * fx)) + fractions.Fraction(_fl(fy * fy)))
        fma = _fl(fx * fx + fractions.Fraction(_fl(fy * fy)))
        if fma > two:
            found.append((x, y))
    assert not found, found[:3]
    sample = list(found[:8]) + [tuple(p) for p in xy[:24]]
    cloud = np.array([[x, y, 0.0] for x, y in sample], np.float32)
    cloud64 = cloud.astype(np.float64)
    radius = np.sqrt(cloud64[:, 0]**2 + cloud64[:, 1]**2)
    assert len(set(radius.tolist())) == len(sample)
    for k, r in enumerate(radius):
        kept = check([cloud], 0.3, float(r), False, device)[2].tolist()
        assert k in kept and kept == sorted(np.nonzero(radius <= r)[0].tolist())
        below = check([cloud], 0.3, float(np.nextafter(r, 0.0)), False, device)[2].tolist()
        assert k not in below and len(below) == len(kept) - 1


# ---- empty results, errors, repeatability ---------------------------------------------------------------------------------
def test_a_cloud_cropped_to_nothing(device):
    near, far = _uniform([400, 300], 2.0, 8)
    far[:, 0] += 100.0
    cfg = get_config('kitti', crop_radius=10.0)
    xyz, out_cu, idx = check([near, far, near], cfg.first_subsampling_dl, 10.0, False, device)
    assert out_cu[1] == out_cu[2] and out_cu[3] == 2 * out_cu[1] and out_cu[1] > 0
    t = lambda a: torch.from_numpy(a).to(device)
    with pytest.raises(ValueError, match="target scan of pair 1"):
        kitti.prepare_pairs([t(near), t(near)], [t(near), t(far)], cfg)
    with pytest.raises(ValueError, match="source scan of pair 0"):
        kitti.prepare_pairs([t(far), t(near)], [t(near), t(near)], cfg)
    ok = kitti.prepare_pairs([t(near), t(near)], [t(near), t(near)], cfg)
    assert [len(c) for c in ok['src_xyz'] + ok['tgt_xyz']] == [out_cu[1]] * 4


@pytest.mark.parametrize("bad", [1e9, float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("axis", [0, 2])
def test_coordinates_outside_the_key_range_raise(device, bad, axis):
    clouds = _uniform([300, 200], 2.0, 9)
    clouds[1][57, axis] = bad
    with pytest.raises(RuntimeError, match=r"2\^20 voxels"):
        run(clouds, 0.3, 0.0, False, device)


def test_two_runs_are_bitwise_equal(device):
    clouds = list(_big())
    a = run(clouds, 0.3, 50.0, True, device)
    b = run(clouds, 0.3, 50.0, True, device)
    assert a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


# ---- scratch discipline ---------------------------------------------------------------------------------------------------
def _c_call(pts, cu, n, nb, voxel, crop_radius, remove_ground, scratch_ptr, scratch_len, device):
    L = _lib.lib()
    xyz = torch.full((n, 3), -7.0, dtype=torch.float32, device=device)
    idx = torch.full((n,), -7, dtype=torch.int32, device=device)
    tail = torch.full((nb + 2,), -7, dtype=torch.int32, device=device)
    rc = L.spr_prepare_scans(pts.data_ptr(), pts.shape[1], cu.data_ptr(), n, nb, voxel, crop_radius, remove_ground,
                             scratch_ptr, scratch_len, xyz.data_ptr(), idx.data_ptr(), tail.data_ptr(),
                             tail.data_ptr() + 4 * (nb + 1), ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    torch.cuda.synchronize()
    return rc, xyz.cpu().numpy(), idx.cpu().numpy(), tail.tolist()


@pytest.mark.parametrize("poison", [0xFF, 0x00])
def test_scratch_of_exactly_the_queried_length_between_guards(device, poison):
    """The operator allocates its scratch itself (torch.empty), so the poisoned-workspace module cannot see it: the C
    entry is called with scratch of exactly spr_prepare_scans_scratch_len ints between two guard bands.  One int less
    is refused before anything is enqueued (the outputs keep their fill)."""
    clouds = _uniform([1500, 1, 900], 3.0, 12)
    n, nb = sum(len(c) for c in clouds), len(clouds)
    pts = torch.from_numpy(np.concatenate(clouds)).to(device)
    cu = ops.lengths_to_cu([len(c) for c in clouds], device)
    need = _lib.lib().spr_prepare_scans_scratch_len(n, nb)
    whole = torch.empty(GUARD + 4 * need + GUARD, dtype=torch.uint8, device=device)
    whole[:GUARD].fill_(GUARD_BYTE)
    whole[GUARD + 4 * need:].fill_(GUARD_BYTE)
    whole[GUARD:GUARD + 4 * need].fill_(poison)
    rc, xyz, idx, tail = _c_call(pts, cu, n, nb, 0.3, 2.5, 1, whole.data_ptr() + GUARD, need, device)
    assert rc == 0 and tail[nb + 1] == 0
    assert bool((whole[:GUARD] == GUARD_BYTE).all()) and bool((whole[GUARD + 4 * need:] == GUARD_BYTE).all())
    ref_xyz, ref_cu, ref_idx = run(clouds, 0.3, 2.5, True, device)
    m = ref_cu[-1]
    assert tail[:nb + 1] == ref_cu and np.array_equal(idx[:m], ref_idx)
    assert np.array_equal(xyz[:m].view(np.uint32), ref_xyz.view(np.uint32))
    rc, xyz, idx, tail = _c_call(pts, cu, n, nb, 0.3, 2.5, 1, whole.data_ptr() + GUARD, need - 1, device)
    assert rc != 0 and b"scratch too small" in _lib.lib().spr_last_error()
    assert bool((xyz == -7.0).all()) and bool((idx == -7).all()) and tail == [-7] * (nb + 2)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_prepare_pairs_feeds_the_forward(device):
    """Two pairs of raw 20 000-point scans (4 columns) -> kitti.prepare_pairs -> RegTR(kitti).eval(): the pose is bitwise
    that of the forward on the same scans prepared cloud by cloud."""
    cfg = get_config('kitti', crop_radius=24.0)
    raw, poses = [], []
    for s in range(2):
        src, tgt, pose = synthetic.make_lidar_pair(20000, seed=40 + s, voxel=1e-3)      # 1 mm: practically raw
        raw.append((src, tgt))
        poses.append(pose)
    refl = lambda c: np.concatenate([c, np.full((len(c), 1), np.nan, np.float32)], 1)
    t = lambda a: torch.from_numpy(a).to(device)
    pose = t(np.stack(poses))
    batch = kitti.prepare_pairs([t(refl(p[0])) for p in raw], [t(refl(p[1])) for p in raw], cfg, pose=pose)
    assert set(batch) == {'src_xyz', 'tgt_xyz', 'pose', 'src_index', 'tgt_index'} and batch['pose'] is pose
    loop = per_cloud_route([p[0] for p in raw] + [p[1] for p in raw], cfg.first_subsampling_dl, cfg.crop_radius,
                           cfg.remove_ground, device)
    for got, want in zip(batch['src_xyz'] + batch['tgt_xyz'], loop):
        assert 1000 < len(got) < 20000 and torch.equal(got, want)
    for k, side in ((0, 'src'), (1, 'tgt')):
        for b in range(2):
            assert torch.equal(t(raw[b][k])[batch[side + '_index'][b]], batch[side + '_xyz'][b])
    model = RegTR(cfg)
    synthetic.fill_parameters(model, 0)
    model = model.to(device).eval()
    out = model(batch)
    ref = model({'src_xyz': loop[:2], 'tgt_xyz': loop[2:], 'pose': pose})
    assert tuple(out['pose'].shape)[-2:] == (3, 4) and bool(torch.isfinite(out['pose']).all())
    assert torch.equal(out['pose'], ref['pose'])
