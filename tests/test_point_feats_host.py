"""CPU: per-point input features on the host side -- the dispatch rule of the small-Cin KPConv kernel (the library's
spr_kpconv_few_supported against stem.few_shape_ok), the workspace carve of its support records, what RegTR refuses
before any launch, the augmentation's feature gather against tests/augment_replica.py's permutations, and the
condition every features case of tests/point_feats_cases.py must keep."""
import numpy as np
import pytest
import torch

import augment_replica as R
import point_feats_cases as pc
from superpoints_registration_amd import _lib, augment, get_config, kitti, regtr, stem


def test_library_rule_is_the_predicates():
    L = _lib.lib()
    for cin in (0, 1, 2, 8, 9, 32):
        for cout in (0, 1, 16, 40, 64, 128):
            for n_kp in (0, 1, 15, 16, 17):
                assert bool(L.spr_kpconv_few_supported(cin, cout, n_kp)) == stem.few_shape_ok(cin, cout, n_kp), (cin, cout, n_kp)
    assert stem.few_shape_ok(4, 64, 15) and not stem.few_shape_ok(1, 64, 15) and not stem.few_shape_ok(9, 64, 15)
    assert not stem.stem_shape_ok(4, 64, 15)            # the fused stem stays Cin = 1


@pytest.mark.parametrize("cin", range(2, 9))
def test_workspace_covers_the_record_buffer(cin):
    """{x, y, z, counted, f_0 .. f_{C-1}} padded to whole 16-byte pieces per support point, on top of what every other
    cin carves (flags, the 16-byte {x, y, z, flag} records, planes, ranges, plan)."""
    L = _lib.lib()
    nq, ns, cout = 1000, 1100, 64
    pieces = 2 if cin <= 4 else 3
    got = L.spr_kpconv_workspace_bytes(nq, ns, cin, cout)
    base = L.spr_kpconv_workspace_bytes(nq, ns, 1, cout) + 2 * 2 * 32 * (cin - 1) * cout    # cin 1: no records, narrower planes
    assert got >= ns * pieces * 16 + ns * 16 + ns
    assert got - base >= ns * pieces * 16 and got - base < ns * pieces * 16 + 1024          # alignment slack only
    grown = L.spr_kpconv_workspace_bytes(nq, 2 * ns, cin, cout) - got
    assert grown >= ns * (pieces * 16 + 16)                                                  # both record buffers grow with ns
    # the query never falls with cin (tests/test_workspace_sizes_host.py): wider inputs keep cin = 8's region
    assert L.spr_kpconv_workspace_bytes(nq, ns, 9, cout) >= L.spr_kpconv_workspace_bytes(nq, ns, 8, cout)


def _clouds(lens):
    return [torch.zeros((n, 3)) for n in lens]


def test_batch_keys_are_checked_on_the_host():
    lens = [5, 7, 6, 4]
    clouds = _clouds(lens)
    names = [f"clouds[{i}]" for i in range(4)]
    good = [torch.ones((n, 4)) for n in lens]
    assert regtr.check_point_feats(4, clouds, good, names) == good
    assert regtr.check_point_feats(1, clouds, None, names) is None              # the column of ones
    assert len(regtr.check_point_feats(1, clouds, [torch.ones((n, 1)) for n in lens], names)) == 4
    with pytest.raises(ValueError, match="in_feats_dim = 4"):
        regtr.check_point_feats(4, clouds, None, names)
    with pytest.raises(ValueError, match=r"clouds\[2\].*expected \[n, 4\]"):
        regtr.check_point_feats(4, clouds, good[:2] + [torch.ones((6, 3))] + good[3:], names)
    with pytest.raises(ValueError, match=r"clouds\[1\].*8 rows for a cloud of 7"):
        regtr.check_point_feats(4, clouds, good[:1] + [torch.ones((8, 4))] + good[2:], names)
    with pytest.raises(ValueError, match=r"clouds\[3\].*float64"):
        regtr.check_point_feats(4, clouds, good[:3] + [torch.ones((4, 4), dtype=torch.float64)], names)
    with pytest.raises(ValueError, match=r"clouds\[0\].*meta"):
        regtr.check_point_feats(4, clouds, [torch.ones((5, 4), device="meta")] + good[1:], names)
    with pytest.raises(ValueError, match="3 entries for 4 clouds"):
        regtr.check_point_feats(4, clouds, good[:3], names)
    with pytest.raises(ValueError, match=r"clouds\[0\].*expected"):
        regtr.check_point_feats(4, clouds, [np.ones((5, 4), np.float32)] + good[1:], names)


def test_batch_forms_name_the_pair_or_the_cloud():
    src, tgt = _clouds([5, 7]), _clouds([6, 4])
    fs, ft = [torch.ones((5, 2)), torch.ones((7, 2))], [torch.ones((6, 2)), torch.ones((4, 2))]
    batch = {"src_xyz": src, "tgt_xyz": tgt, "src_point_feats": fs, "tgt_point_feats": ft}
    out = regtr.batch_point_feats(2, batch)
    assert [o.shape[0] for o in out] == [5, 7, 6, 4] and out[2] is ft[0]          # _encode's order: sources, then targets
    with pytest.raises(ValueError, match="the target of pair 1"):
        regtr.batch_point_feats(2, {**batch, "tgt_point_feats": [ft[0], torch.ones((4, 3))]})
    with pytest.raises(ValueError, match="the source of pair 0"):
        regtr.batch_point_feats(2, {**batch, "src_point_feats": [torch.ones((6, 2)), fs[1]]})
    with pytest.raises(ValueError, match="come together"):
        regtr.batch_point_feats(2, {"src_xyz": src, "tgt_xyz": tgt, "src_point_feats": fs})
    with pytest.raises(ValueError, match="in_feats_dim = 2"):
        regtr.batch_point_feats(2, {"src_xyz": src, "tgt_xyz": tgt})
    assert regtr.batch_point_feats(1, {"src_xyz": src, "tgt_xyz": tgt}) is None
    clouds = src + tgt
    shared = (clouds, [0, 1], [2, 3])
    got = regtr.batch_point_feats(2, {"cloud_point_feats": fs + ft}, shared)
    assert got[1] is fs[1]
    with pytest.raises(ValueError, match=r"clouds\[3\]"):
        regtr.batch_point_feats(2, {"cloud_point_feats": fs + [ft[0], torch.ones((5, 2))]}, shared)
    with pytest.raises(ValueError, match="in_feats_dim = 2"):
        regtr.batch_point_feats(2, {}, shared)


def test_model_refuses_before_any_launch():
    """in_feats_dim > 1 without features: ValueError from forward() and encode() on CPU tensors -- no device is touched
    (the same calls with features would go on to refuse the CPU clouds)."""
    model = regtr.RegTR(get_config("3dmatch", in_feats_dim=4)).eval()
    assert tuple(model.kpf_encoder.encoder_blocks[0].KPConv.weights.shape) == (15, 4, 64)
    src, tgt = _clouds([50]), _clouds([40])
    with pytest.raises(ValueError, match="in_feats_dim = 4"):
        model({"src_xyz": src, "tgt_xyz": tgt})
    with pytest.raises(ValueError, match=r"the source of pair 0.*expected \[n, 4\]"):
        model({"src_xyz": src, "tgt_xyz": tgt, "src_point_feats": [torch.ones((50, 3))], "tgt_point_feats": [torch.ones((40, 4))]})
    # in_feats_dim > 8 is allowed (the generic kernel): the model builds
    assert tuple(regtr.RegTR(get_config("3dmatch", in_feats_dim=9)).kpf_encoder.encoder_blocks[0].KPConv.weights.shape) == (15, 9, 64)


@pytest.mark.parametrize("max_pts", [30000, 40])
def test_augmentation_gathers_features_by_the_replica_permutation(max_pts):
    """augment.permute_point_feats (what augment_batch applies to the library call's permutations) against the
    permutations of the augmentation's CPU replica: per pair, shuffled, cut at max_pts and sides exchanged on a swap."""
    rng = np.random.default_rng(5)
    lens_s, lens_t, swaps = [33, 64, 50, 7], [41, 20, 50, 90], [False, True, True, False]
    C = 3
    feats_s = [rng.standard_normal((n, C)).astype(np.float32) for n in lens_s]
    feats_t = [rng.standard_normal((n, C)).astype(np.float32) for n in lens_t]
    perms_s, perms_t, want_s, want_t = [], [], [], []
    for b, (n, m, sw) in enumerate(zip(lens_s, lens_t, swaps)):
        pose = np.eye(4, dtype=np.float32)[:3]
        r = R.apply_pair(rng.standard_normal((n, 3)).astype(np.float32), rng.standard_normal((m, 3)).astype(np.float32),
                         pose, pose, False, sw, 'none', 0.0, max_pts, np.zeros((n, 3), np.float32),
                         np.zeros((m, 3), np.float32), rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32),
                         rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32))
        perms_s.append(r['src_perm'])
        perms_t.append(r['tgt_perm'])
        want_s.append((feats_t[b] if sw else feats_s[b])[r['src_perm']])
        want_t.append((feats_s[b] if sw else feats_t[b])[r['tgt_perm']])
    out_s, out_t = augment.output_lengths(lens_s, lens_t, swaps, max_pts)
    assert out_s == [len(p) for p in perms_s] and out_t == [len(p) for p in perms_t]
    got = augment.permute_point_feats([torch.from_numpy(f) for f in feats_s + feats_t],
                                      torch.from_numpy(np.concatenate(perms_s).astype(np.int32)),
                                      torch.from_numpy(np.concatenate(perms_t).astype(np.int32)),
                                      lens_s, lens_t, out_s, out_t, swaps)
    for b in range(4):
        assert np.array_equal(got['src_point_feats'][b].numpy(), want_s[b])          # values untouched: bit for bit
        assert np.array_equal(got['tgt_point_feats'][b].numpy(), want_t[b])
        assert np.array_equal(got['src_perm'][b].numpy(), perms_s[b]) and got['src_perm'][b].dtype == torch.int64
        assert np.array_equal(got['tgt_perm'][b].numpy(), perms_t[b])


def test_kitti_intensity_is_refused_without_a_fourth_column():
    cfg = get_config("kitti")
    xyz = [torch.zeros((10, 3))]
    with pytest.raises(ValueError, match="intensity=True needs"):
        kitti.prepare_pairs(xyz, xyz, cfg, intensity=True)


def test_every_features_case_keeps_the_condition():
    for c in pc.WIDTHS:
        for kind in ("signed", "colour", "negative", "integer"):
            x = pc.features(350, c, 900 + c, kind)
            integer = pc.check_conditions(x)
            assert x.dtype == np.float32 and x.shape == (350, c)
            if kind == "integer":
                assert integer.all() and np.all(x[:87].sum(1) == 0) and np.all(x[87:175].sum(1) == -1)
            if kind == "negative":
                assert np.all(x.sum(1) < 0)
            if kind == "signed":                           # rows of both signs: counted and uncounted neighbours
                frac = float((x.astype(np.float64).sum(1) > 0).mean())
                assert 0.1 < frac < 0.9, frac
            if kind == "colour":
                assert np.all(x[:, 0] == 1.0)
        x, mags = pc.magnitude_features(350, c, 950 + c)
        pc.check_conditions(x)
        assert mags.max() / mags.min() >= 1e23
    for nq, ns, kmax, c, cout, kind, srt, n_kp in pc.SHAPE_CASES:
        q, s, nb, x, w, kp, ext = pc.kernel_case(nq, ns, kmax, c, cout, 1000 + nq, kind, rows_sorted=srt, n_kp=n_kp)
        pc.check_conditions(x)
        assert stem.few_shape_ok(c, cout, n_kp) and w.shape == (n_kp, c, cout) and kp.shape == (n_kp, 3)
    for t in pc.golden_inputs()[2:]:
        pc.check_conditions(t)
    with pytest.raises(AssertionError):
        pc.check_conditions(np.array([[1.0, -1.0, 2.0 ** -30, 0.5], [1.0, -1.0, 2.0 ** -30, 0.0]], np.float32))
