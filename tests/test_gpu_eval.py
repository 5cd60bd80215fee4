"""GPU: the `evaluation` subpackage (csrc/evaluate.hip) against the float64 replica of its contract
(tests/eval_replica.py) on the cases of tests/eval_cases.py, against the reference's own outputs
(tests/golden/eval_modelnet.npz), and end to end behind RegTR.

d2_* and nn_* are determined exactly by the contract: they equal the replica's bit for bit, and so does inlier_count.
The metric columns are held to 1e-12 relative: the two Chamfer means are sums of at most 4096 non-negative float64
terms in another order than the replica's exactly rounded sum ((n - 1) 2^-53 <= 4.6e-13); the pose columns see the
same float64 operations in the same order up to the last bits of atan2 / asin / acos / sqrt (a few 2^-53 on angles
whose differences are never below 1e-3 of the angles themselves in these cases).  A column that is exactly 0 in the
replica is exactly 0 here.
Every pair's outputs are a function of the pair alone: bit-equal alone, at another position of a batch and on a second
call.  Case sizes sit around the kernel's two tile constants, which the subpackage exports and
test_tile_constants pins: T targets per LDS tile, Q queries per workgroup."""
import numpy as np
import pytest
import torch

import eval_cases as C
import eval_replica as R
from superpoints_registration_amd import evaluation as E, get_config, modelnet, synthetic
from superpoints_registration_amd.regtr import RegTR
from superpoints_registration_amd.se3 import se3_compare
from test_eval_host import check_against_fixture, fixture_pairs

pytestmark = pytest.mark.gpu
T = torch.from_numpy
REL = 1e-12
NN_KEYS = ("d2_src", "nn_src", "d2_ref", "nn_ref")


def run(name, device, pairs=None, put=lambda t: t, raw=True, corr=True, case=None):
    """eval_pairs_raw on the pairs `pairs` (default: all, in order) of a case."""
    c = C.case(name) if case is None else case
    pairs = list(range(len(c["src"]))) if pairs is None else list(pairs)
    up = lambda xs: [put(T(xs[b]).to(device)) for b in pairs]
    use_raw, use_corr = raw and c["raw"] is not None, corr and c["corr"] is not None
    return E.eval_pairs_raw(up(c["src"]), up(c["ref"]), put(T(c["gt"][pairs]).to(device)),
                            put(T(c["pred"][pairs]).to(device)), raw_list=up(c["raw"]) if use_raw else None,
                            corr=(up(c["corr"][0]), up(c["corr"][1])) if use_corr else None,
                            acceptance_radius=c["radius"] if use_corr else None)


def pair_of(out, b):
    """Pair b of a result, as host arrays."""
    d = {"metrics": out["metrics"][b].cpu().numpy(), "status": out["status"][b].cpu().numpy()}
    for k in NN_KEYS:
        if k in out:
            d[k] = out[k][b].cpu().numpy()
    return d


def same_bits(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: {k} differs"


def check_against_replica(name, out, ref):
    worst = 0.0
    assert tuple(out["metrics"].shape) == (len(ref), len(E.COLUMNS)) and out["metrics"].dtype == torch.float64
    for b, r in enumerate(ref):
        g = pair_of(out, b)
        what = f"{name} pair {b}"
        assert int(g["status"]) == r["status"], what
        for k in NN_KEYS:
            if k in r:
                want = np.ascontiguousarray(r[k], dtype=np.float64 if k[0] == "d" else np.int32)
                assert g[k].dtype == want.dtype and g[k].tobytes() == want.tobytes(), \
                    f"{what}: {k} differs in {int((g[k] != want).sum())} of {len(want)} rows"
            else:
                assert k not in g, what
        for i, k in enumerate(E.COLUMNS):
            x, y = float(g["metrics"][i]), float(r[k])
            assert float(out[k][b]) == x, f"{what}: the named view {k} is not its column"
            if y == 0.0 or k == "inlier_count":
                assert x == y, f"{what}: {k} = {x!r}, the contract says {y!r}"
            else:
                worst = max(worst, abs(x - y) / abs(y))
                assert abs(x - y) <= REL * abs(y), f"{what}: {k} = {x!r} vs {y!r} (relative {abs(x - y) / abs(y):.3e})"
    print(f"evaluation {name}: largest relative difference of a column to the replica = {worst:.3e}")


def test_tile_constants():
    assert (E.TILE, E.QUERIES) == (256, 128)
    sizes = {tuple(len(x) for x in (s, t, r)) for s, t, r in zip(*(C.case("tiles")[k] for k in ("src", "ref", "raw")))}
    assert {s[2] for s in sizes} == {255, 256, 257, 515} and {s[0] for s in sizes} == {s[1] for s in sizes} == {127, 128, 129}


@pytest.mark.parametrize("name", C.CASES)
def test_matches_the_replica(device, name):
    check_against_replica(name, run(name, device), C.replica(name))


def test_edge_rules(device):
    out = run("boundary", device)
    assert out["inlier_count"].tolist() == [1.0] and out["inlier_ratio"].tolist() == [0.25]
    t = run("ties", device)
    for b, raw in enumerate(C.case("ties")["raw"]):
        assert int(t["nn_src"][b].max()) < len(raw) // 2 and int(t["nn_ref"][b].max()) < len(raw) // 2
    s = run("same", device)
    assert not bool(s["metrics"][0].any()) and s["metrics"][1, :4].tolist() == [0.0] * 4
    assert not bool(s["d2_src"][0].any()) and not bool(s["d2_ref"][0].any())
    e = run("emptyraw", device)
    assert e["status"].tolist() == [0, -2, 0] and e["metrics"][1, 7:10].tolist() == [0.0] * 3
    assert float(e["err_t"][1]) > 0 and set(e["nn_src"][1].tolist()) == {-1}
    c = C.case("emptyraw")
    with pytest.raises(ValueError, match="pair 1: an empty raw cloud"):
        E.eval_pairs([T(x).to(device) for x in c["src"]], [T(x).to(device) for x in c["ref"]], c["gt"], c["pred"],
                     raw_list=[T(x).to(device) for x in c["raw"]])


def test_parts_that_are_not_asked_for(device):
    """raw=None / corr=None: the columns of that part are 0, no neighbour lists, every other column unchanged."""
    full = run("ragged", device)
    no_raw, no_corr, neither = (run("ragged", device, raw=r, corr=c) for r, c in ((False, True), (True, False), (False, False)))
    assert not any(k in no_raw for k in NN_KEYS) and all(k in no_corr for k in NN_KEYS)
    assert torch.equal(no_raw["metrics"][:, :7], full["metrics"][:, :7]) and not bool(no_raw["metrics"][:, 7:10].any())
    assert torch.equal(no_raw["metrics"][:, 10:], full["metrics"][:, 10:])
    assert torch.equal(no_corr["metrics"][:, :10], full["metrics"][:, :10]) and not bool(no_corr["metrics"][:, 10:].any())
    assert torch.equal(neither["metrics"][:, :7], full["metrics"][:, :7]) and not bool(neither["metrics"][:, 7:].any())
    for k in NN_KEYS:
        assert all(torch.equal(a, b) for a, b in zip(no_corr[k], full[k])), k
    c = C.case("ragged")
    ir = E.inlier_ratio([T(x).to(device) for x in c["corr"][0]], [T(x).to(device) for x in c["corr"][1]], c["gt"], c["radius"])
    assert torch.equal(ir, full["inlier_ratio"]) and ir.dtype == torch.float64
    assert float(E.feature_matching_recall(ir)) == float((ir > 0.05).double().mean())


def test_every_pair_is_independent_of_its_batch(device):
    n = len(C.case("ragged")["src"])
    whole, rev, again = run("ragged", device), run("ragged", device, pairs=range(n - 1, -1, -1)), run("ragged", device)
    for b in range(n):
        alone = pair_of(run("ragged", device, pairs=[b]), 0)
        same_bits(alone, pair_of(whole, b), f"ragged pair {b} alone / in the batch")
        same_bits(alone, pair_of(rev, n - 1 - b), f"ragged pair {b} alone / in the reversed batch")
        same_bits(pair_of(again, b), pair_of(whole, b), f"ragged pair {b}, second call")
    tiles, tiles2 = run("tiles", device), run("tiles", device)
    for b in range(4):
        same_bits(pair_of(tiles, b), pair_of(tiles2, b), f"tiles pair {b}, second call")
        same_bits(pair_of(tiles, b), pair_of(run("tiles", device, pairs=[3, b]), 1), f"tiles pair {b} behind pair 3")


def test_a_nonfinite_pair_is_refused_alone(device):
    out = run("nonfinite", device)
    assert out["status"].tolist() == [0, -1, 0]
    assert not bool(out["metrics"][1].any()) and set(out["nn_ref"][1].tolist()) == {-1} and not bool(out["d2_src"][1].any())
    for b in (0, 2):
        same_bits(pair_of(run("nonfinite", device, pairs=[b]), 0), pair_of(out, b), f"pair {b} beside the refused one")
    c = dict(C.case("nonfinite"))
    up = lambda xs: [T(x).to(device) for x in xs]
    with pytest.raises(ValueError, match="pair 1: a non-finite coordinate or pose"):
        E.eval_pairs(up(c["src"]), up(c["ref"]), c["gt"], c["pred"], raw_list=up(c["raw"]))
    c["pred"] = c["pred"].copy()
    c["pred"][2, 1, 3] = np.inf
    out = run("nonfinite", device, case=c)
    assert out["status"].tolist() == [0, -1, -1] and not bool(out["metrics"][2].any())
    same_bits(pair_of(run("nonfinite", device, pairs=[0]), 0), pair_of(out, 0), "pair 0 beside two refused ones")
    with pytest.raises(ValueError, match=r"pair 1: .*, pair 2: a non-finite coordinate or pose"):
        E.eval_pairs(up(c["src"]), up(c["ref"]), c["gt"], c["pred"], raw_list=up(c["raw"]))


def test_modelnet_metrics_match_the_reference(device):
    """The fixture's twelve pairs in ONE call (the reference needs one call per pair), float32 poses as it was given."""
    g, pairs = fixture_pairs()
    up = lambda i: [T(p[i]).to(device) for p in pairs]
    m = E.modelnet_metrics(up(0), up(1), up(2), T(g["gt"]).to(device), T(g["pred"]))     # poses: device f32 / host f32
    assert sorted(m) == sorted(E.MODELNET_KEYS) and all(v.dtype == torch.float64 and v.is_cuda for v in m.values())
    check_against_fixture(g, {k: v.cpu().numpy() for k, v in m.items()}, "eval_pairs")
    replica = [R.eval_pair(s, t, gt, pr, raw) for s, t, raw, gt, pr in pairs]
    for k in E.MODELNET_KEYS:
        assert np.allclose(m[k].cpu().numpy(), [r[k] for r in replica], rtol=REL, atol=0.0), k


def test_regtr_output_through_the_evaluator(device):
    """RegTR(modelnet) on two make_pairs pairs of 64-point shapes -> Evaluator: its table is modelnet_metrics called
    directly; trans_err and err_r_deg agree with se3_compare to 1e-5."""
    cfg = get_config("modelnet")                                          # every generated cloud has 717 points
    rng = np.random.default_rng(5)
    v = rng.standard_normal((2, 64, 3))
    shapes = T((v / np.linalg.norm(v, axis=2, keepdims=True) * (0.5 + 0.3 * rng.random((2, 64, 1)))).astype(np.float32))
    shapes = shapes.to(device)
    batch = modelnet.make_pairs(shapes, cfg, seed=7, keys=[0, 1])
    batch["tgt_raw"] = [shapes[0], shapes[1]]
    model = RegTR(cfg)
    synthetic.fill_parameters(model, seed=0)
    pred = model.to(device).eval()({"src_xyz": batch["src_xyz"], "tgt_xyz": batch["tgt_xyz"]})
    ev = E.Evaluator(cfg)
    ev.update(batch, pred)
    ev.update(batch, pred)                                                # a second batch: four pairs in the table
    pose = pred["pose"][-1] if pred["pose"].dim() == 4 else pred["pose"]
    direct = E.modelnet_metrics(batch["src_xyz"], batch["tgt_xyz"], batch["tgt_raw"], batch["pose"], pose)
    table = ev.per_pair()
    for k in E.MODELNET_KEYS:
        want = direct[k].cpu().numpy()
        assert np.array_equal(table[k], np.concatenate([want, want])), k
    s = ev.summary()
    want = E.summarize_metrics({k: np.concatenate([direct[k].cpu().numpy()] * 2) for k in E.MODELNET_KEYS})
    assert all(s[k] == want[k] for k in want) and ev.report() == E.format_metrics(want)
    assert np.array_equal(s["pred_transforms"], np.concatenate([pose.double().cpu().numpy()] * 2))
    cmp = se3_compare(pose.double().cpu(), batch["pose"].double().cpu())
    assert np.allclose(table["trans_err"][:2], cmp["trans"].numpy(), rtol=0, atol=1e-5)
    assert np.allclose(table["err_r_deg"][:2], cmp["rot_deg"].numpy(), rtol=0, atol=1e-5)
