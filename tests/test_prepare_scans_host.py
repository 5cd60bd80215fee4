"""CPU: spr_prepare_scans' size query and argument checks (include/spr.h).  Everything here is answered on the host
before any HIP call, so it runs on a machine without a GPU; the kernels are checked in tests/test_gpu_prepare_scans.py."""
import ctypes

import pytest

from superpoints_registration_amd import _lib, get_config
from test_workspace_sizes_host import HUGE, INT_MAX, sweep_points

N_MAX = INT_MAX - 1024          # the entry point's own limit on n (spr.h)


def test_symbols_are_exported_and_bound():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("spr_prepare_scans", "spr_prepare_scans_scratch_len"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["spr_prepare_scans_scratch_len"] == (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int])
    assert len(_lib.SIGNATURES["spr_prepare_scans"][1]) == 15
    assert hasattr(_lib.lib(), "spr_prepare_scans")


def test_scratch_len_is_monotone_in_n_and_nb():
    q = _lib.lib().spr_prepare_scans_scratch_len
    for i, limit in enumerate((N_MAX, INT_MAX)):
        prev = None
        for v in sweep_points(limit):
            args = [1000, 3]
            args[i] = v
            r = q(*args)
            assert r < HUGE, (args, r)
            assert prev is None or r >= prev, (args, prev, r)
            prev = r
    # the table alone is two ints per point: the count is of ints, not bytes
    assert 2 * 120000 <= q(120000, 2) < 3 * 120000
    assert q(N_MAX, 1) >= 2 * N_MAX


def test_scratch_len_gives_no_huge_value_for_non_positive_sizes():
    q = _lib.lib().spr_prepare_scans_scratch_len
    for i in range(2):
        one = [1000, 3]
        one[i] = 1
        cap = max(q(*one), q(1000, 3))
        for v in (0, -1, -(1 << 31)):
            args = [1000, 3]
            args[i] = v
            assert q(*args) <= cap, (args, q(*args), cap)


def _call(**over):
    """spr_prepare_scans with plausible arguments (host addresses that are never dereferenced: every case below is
    refused before the first HIP call) and the overrides; returns (rc, message)."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    a = dict(pts=p, stride=3, cu=p, n=1000, nb=2, voxel_size=0.3, crop_radius=0.0, remove_ground=0, scratch=p,
             scratch_len=L.spr_prepare_scans_scratch_len(1000, 2), out_xyz=p, out_idx=p, out_cu=p, status=p, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    rc = L.spr_prepare_scans(a['pts'], a['stride'], a['cu'], a['n'], a['nb'], a['voxel_size'], a['crop_radius'],
                             a['remove_ground'], a['scratch'], a['scratch_len'], a['out_xyz'], a['out_idx'], a['out_cu'],
                             a['status'], a['stream'])
    return rc, L.spr_last_error()


@pytest.mark.parametrize("name", ["pts", "cu", "scratch", "out_xyz", "out_idx", "out_cu", "status"])
def test_null_pointers_are_refused(name):
    rc, msg = _call(**{name: None})
    assert rc != 0 and b"prepare_scans" in msg and b"null" in msg


@pytest.mark.parametrize("over,word", [
    (dict(stride=2), b"stride"), (dict(stride=5), b"stride"), (dict(stride=0), b"stride"),
    (dict(voxel_size=0.0), b"voxel_size"), (dict(voxel_size=-0.3), b"voxel_size"),
    (dict(voxel_size=float("nan")), b"voxel_size"),
    (dict(n=0), b"at least 1"), (dict(n=-5), b"at least 1"), (dict(nb=0), b"at least 1"), (dict(nb=-1), b"at least 1"),
    (dict(nb=1001), b"clouds"), (dict(n=INT_MAX, nb=1), b"exceeds"),
])
def test_bad_sizes_are_refused(over, word):
    rc, msg = _call(**over)
    assert rc != 0 and b"prepare_scans" in msg and word in msg, msg


def test_short_scratch_is_refused_without_a_launch():
    need = _lib.lib().spr_prepare_scans_scratch_len(1000, 2)
    for short in (need - 1, 1, 0):
        rc, msg = _call(scratch_len=short)
        assert rc != 0 and b"scratch too small" in msg, msg


def test_kitti_config_carries_the_loaders_crop_keys():
    cfg = get_config('kitti')
    assert cfg.crop_radius == 0.0 and cfg.remove_ground is False          # conf/qk_regtr_full_kitti.yaml
    assert get_config('kitti', crop_radius=50.0, remove_ground=True).crop_radius == 50.0
