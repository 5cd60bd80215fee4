"""GPU: grid subsampling with features and labels (subsample_attrs.grid_subsample, spr_grid_subsample_attrs) on the
cases of tests/subsample_attrs_cases.py -- bit for bit against the reference's results (tests/golden/subsample_attrs.npz)
where the reference is defined and in its row order, against the numpy restatement (tests/subsample_attrs_replica.py)
everywhere and in both order modes, and against ops.grid_subsample for the points and lengths.  Exact by construction:
equality of bits is the only tolerance."""
import functools

import numpy as np
import pytest
import torch

import subsample_attrs_cases as sc
import subsample_attrs_replica as R
from conftest import load_golden
from superpoints_registration_amd import kpconv, ops, subsample_attrs

pytestmark = pytest.mark.gpu
T = torch.tensor           # copies: the cases hand out read-only arrays
ORDERS = {"reference": ops.ORDER_REFERENCE, "canonical": ops.ORDER_CANONICAL}


@pytest.fixture(scope="module")
def gold():
    return load_golden("subsample_attrs.npz")


@functools.lru_cache(maxsize=None)
def expected(name, order):
    c = sc.cases()[name]
    return R.grid_subsample(c.pts, c.lens, c.dl, c.max_p, order, c.feat, c.lab)


def run(c, device, order, lab=None):
    """The device call on case c (lab: another form of its labels); returns the result tuple and the plain call's."""
    pts, cu = T(c.pts).to(device), ops.lengths_to_cu(list(c.lens), device)
    feat = None if c.feat is None else T(c.feat).to(device)
    if lab is None and c.lab is not None:
        lab = T(c.lab)
    lab = None if lab is None else lab.to(device)
    got = subsample_attrs.grid_subsample(pts, cu, c.dl, max_p=c.max_p, order=ORDERS[order], features=feat, labels=lab)
    plain = ops.grid_subsample(pts, cu, c.dl, max_p=c.max_p, order=ORDERS[order])
    return got, plain


def bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def unpack(c, got):
    """(points, lens, features or None, labels or None) as host arrays from the result tuple of case c."""
    assert len(got) == 2 + (c.feat is not None) + (c.lab is not None)
    rest = list(got[2:])
    feat = rest.pop(0) if c.feat is not None else None
    lab = rest.pop(0) if c.lab is not None else None
    return got[0], got[1], feat, lab


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("name", sc.NAMES)
def test_case_matches_reference_replica_and_plain_call(gold, device, name, order):
    c = sc.cases()[name]
    got, plain = run(c, device, order)
    sub, lens, feat, lab = unpack(c, got)
    m = sub.shape[0]
    assert all(t.is_cuda for t in got) and int(lens.sum()) == m
    # points and lengths: the plain call's bits
    assert np.array_equal(bits(sub), bits(plain[0])) and np.array_equal(bits(lens), bits(plain[1]))
    # the restatement, everywhere
    e_sub, e_lens, e_feat, e_lab = expected(name, order)
    assert np.array_equal(bits(lens), e_lens) and np.array_equal(bits(sub), e_sub.view(np.uint32))
    if feat is not None:
        assert feat.shape == (m, sc.fdim(c)) and feat.dtype == torch.float32
        assert np.array_equal(bits(feat), e_feat.view(np.uint32))
    if lab is not None:
        assert lab.shape == (m, sc.ldim(c)) and lab.dtype == torch.int32
        assert np.array_equal(bits(lab), e_lab)
    # the reference, where it is defined and in its own order
    if order == "reference" and name in sc.REFERENCE_DEFINED:
        assert np.array_equal(bits(lens), gold[f"{name}.lens"])
        assert np.array_equal(bits(sub), gold[f"{name}.pts"].view(np.uint32))
        if feat is not None:
            assert np.array_equal(bits(feat), gold[f"{name}.feat"].view(np.uint32))
        if lab is not None:
            assert np.array_equal(bits(lab), gold[f"{name}.lab"])
    # a second run gives the same bits
    again = unpack(c, run(c, device, order)[0])
    for a, b in zip((sub, lens, feat, lab), again):
        assert (a is None and b is None) or np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("name", ["extremes", "ties.k3", "sizes.nb3.a", "max_p"])
def test_label_forms_keep_rank_and_dtype(device, name):
    """[N] and [N, 1], int32 and int64: the same votes, in the rank and dtype of the input."""
    c = sc.cases()[name]
    want = expected(name, "reference")[3]
    for dtype in (torch.int32, torch.int64):
        for flat in (False, True):
            lab = T(c.lab).to(dtype)
            got, _ = run(c, device, "reference", lab=lab[:, 0].contiguous() if flat else lab)
            out = got[-1]
            assert out.dtype == dtype and out.shape == ((want.shape[0],) if flat else want.shape)
            assert np.array_equal(out.cpu().numpy().reshape(want.shape), want)


def test_labels_alone_features_alone_and_neither(device):
    c = sc.cases()["dims.f3.l1"]
    pts, cu = T(c.pts).to(device), ops.lengths_to_cu(list(c.lens), device)
    feat, lab = T(c.feat).to(device), T(c.lab).to(device)
    _, _, e_feat, e_lab = expected("dims.f3.l1", "reference")
    both = subsample_attrs.grid_subsample(pts, cu, c.dl, features=feat, labels=lab)
    only_f = subsample_attrs.grid_subsample(pts, cu, c.dl, features=feat)
    only_l = subsample_attrs.grid_subsample(pts, cu, c.dl, labels=lab)
    neither = subsample_attrs.grid_subsample(pts, cu, c.dl)
    assert (len(both), len(only_f), len(only_l), len(neither)) == (4, 3, 3, 2)
    assert np.array_equal(bits(only_f[2]), e_feat.view(np.uint32)) and np.array_equal(bits(both[2]), bits(only_f[2]))
    assert np.array_equal(bits(only_l[2]), e_lab) and np.array_equal(bits(both[3]), bits(only_l[2]))
    plain = ops.grid_subsample(pts, cu, c.dl)
    for res in (both, only_f, only_l, neither):
        assert np.array_equal(bits(res[0]), bits(plain[0])) and np.array_equal(bits(res[1]), bits(plain[1]))


def test_batch_grid_subsampling_kpconv_returns_the_reference_tuples(gold, device):
    """kpconv.py:187-214: (points, lengths, features), (points, lengths, labels) or all four; labels [M, ldim] int32
    as the reference's wrapper returns them, also for labels of shape [N]."""
    name = "sizes.nb3.a"
    c = sc.cases()[name]
    pts, lens = T(c.pts).to(device), torch.tensor(c.lens, dtype=torch.int32)
    feat, lab = T(c.feat).to(device), T(c.lab[:, 0].copy()).to(device)
    for fn in (kpconv.batch_grid_subsampling_kpconv, kpconv.batch_grid_subsampling_kpconv_gpu):
        s_pts, s_len, s_feat, s_lab = fn(pts, lens, features=feat, labels=lab, sampleDl=c.dl)
        assert np.array_equal(bits(s_pts), gold[f"{name}.pts"].view(np.uint32))
        assert np.array_equal(bits(s_len), gold[f"{name}.lens"])
        assert np.array_equal(bits(s_feat), gold[f"{name}.feat"].view(np.uint32))
        assert s_lab.dtype == torch.int32 and np.array_equal(bits(s_lab), gold[f"{name}.lab"])
        three = fn(pts, lens, features=feat, sampleDl=c.dl)
        assert len(three) == 3 and np.array_equal(bits(three[2]), bits(s_feat))
        three = fn(pts, lens, labels=lab, sampleDl=c.dl)
        assert len(three) == 3 and three[2].shape == s_lab.shape and np.array_equal(bits(three[2]), bits(s_lab))
        two = fn(pts, lens, sampleDl=c.dl)
        assert len(two) == 2 and np.array_equal(bits(two[0]), bits(s_pts))
    cut = kpconv.batch_grid_subsampling_kpconv(pts, lens, features=feat, labels=lab, sampleDl=c.dl, max_p=5)
    assert cut[1].tolist() == [5, 1, 5] and cut[2].shape == (11, 4) and cut[3].shape == (11, 1)


def test_host_side_refusals(device):
    c = sc.cases()["dims.f3.l1"]
    pts, cu = T(c.pts).to(device), ops.lengths_to_cu(list(c.lens), device)
    with pytest.raises(RuntimeError, match="device"):
        subsample_attrs.grid_subsample(pts, cu, c.dl, features=T(c.feat))
    with pytest.raises(RuntimeError, match=r"\(N, d\)"):
        subsample_attrs.grid_subsample(pts, cu, c.dl, features=T(c.feat[:-1]).to(device))
    with pytest.raises(RuntimeError, match="int32 or int64"):
        subsample_attrs.grid_subsample(pts, cu, c.dl, labels=T(c.feat[:, :1]).to(device))
    far = torch.tensor([[0.01, 0.01, 0.01], [7.0e4, 7.0e4, 0.01]], device=device)     # keys beyond 2^40: the -1 code
    with pytest.raises(RuntimeError, match="40-bit"):
        subsample_attrs.grid_subsample(far, ops.lengths_to_cu([2], device), 0.025, labels=torch.zeros(2, dtype=torch.int32,
                                                                                                    device=device))
