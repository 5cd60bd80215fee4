"""Range and edge cases of deformable / modulated KPConv (csrc/kpconv_deform.hip) and of its regulariser
(csrc/deform_reg.hip): the inputs of tests/test_gpu_deform_range.py, checked without a GPU by
tests/test_deform_range_host.py.

    build(...)               kpconv_modes_cases.cloud_case's geometry (forward_cases.kp_cloud_case: KITTI-like offsets,
                             nearest-first rows, shadow entries; no quadratic search) at the deformable geometry of
                             deform_cases.make_case: search scale R, kernel points of radius R / 2, extent 0.8 R / 2, own
                             offset-convolution kernel points, seeded off_w / off_b.  case['of'] holds the float32-rounded
                             offset features of the float64 offset convolution: what a kernel under test is handed.
    CASES / REG_CASES        name -> Spec (deformable KPConv / regulariser);  get(name) builds a case
    guarded_ref(...)         deform_cases.kpconv_deform_ref with the square root guarded at d2 == 0 (h = 1, no positional
                             gradient there): the torch.where guard of deform_reg_cases.reg_ref
    ref64(case, go)          float64 (out, aux, grads at x, W and the offset features)
    check_conditions(...)    range gap, distance floor and row sums of deform_cases, asserted on every case that compares
                             anything; `zeros` cases hold items at d2 == 0 exactly and assert "every item is exactly 0 or
                             >= DIST_MIN" instead of the floor

Offset seeds: a case's offsets come from off_w / off_b drawn with seed OFFSET_SEED0, OFFSET_SEED0 + 1, ...: the first seed
at which the float64 reference ALONE meets the case's conditions (first_seed; at most MAX_SEEDS tries).  Nothing a kernel
computes takes part in the choice, no row or item is excluded, and the host module asserts the conditions of every case
again on what get() returns.
"""
import functools

import numpy as np
import torch

import deform_cases as dc
import deform_reg_cases as rc
import forward_cases as fc
import kpconv_modes_cases as kc

MOD = [False, True]
mod_id = lambda m: "modulated" if m else "plain"

# route name -> (impl, cin, cout, n_kp): the forward kernels spr_kpconv_deform_fwd dispatches to
ROUTES = {"tile32": (0, 32, 64, 15), "tile64": (0, 64, 64, 15), "simple48": (0, 48, 40, 15), "cin1": (0, 1, 32, 15),
          "impl1": (1, 32, 32, 15), "kp1": (0, 32, 32, 1), "kp7": (0, 32, 32, 7), "kp16": (0, 32, 32, 16)}
ROUTE_KERNEL = {"tile32": "tile32", "tile64": "tile64", "simple48": "simple", "cin1": "simple", "impl1": "simple",
                "kp1": "simple", "kp7": "simple", "kp16": "simple"}
FWD_ROUTES = ("tile32", "tile64", "simple48", "cin1", "impl1")
BWD_ROUTES = ("tile64", "simple48")
TILE_ROUTES = ("tile32", "tile64")
TILE_KP = 15            # kKP
KP_MAX = 16             # kKPmax = kGroup


def deform_route(impl, cin, cout, n_kp):
    """The forward kernel a call reaches, restated from spr_kpconv_deform_fwd's dispatch (csrc/kpconv_deform.hip)."""
    planes = cin > 0 and cin % 32 == 0 and cout > 0 and cout % 32 == 0 and cout <= 256        # plane_shape
    if impl == 0 and n_kp == TILE_KP and planes:
        return "tile64" if cin % 64 == 0 else "tile32"
    return "simple"


# launch_deform_tile: the grid is capped at device_cu_count() * (160 KB / deform_lds_bytes(CC))
TQ, WAVES, SLOT, LDS_BUDGET = 32, 8, 16, 160 * 1024


def deform_lds_bytes(cc):
    return 2 * 2 * TQ * (TILE_KP * cc + 16) + 16 * WAVES * KP_MAX + 4 * WAVES * 64 * SLOT + 4 * WAVES * 64 + 4 * TQ


def residency(cc):
    return max(1, LDS_BUDGET // deform_lds_bytes(cc))


def grid_nq(n_cu, cc):
    """More tiles than the launch's grid: every workgroup's first trip, one full second-trip tile and a tile of one row."""
    return 32 * (n_cu * residency(cc)) + 33


OFFSET_SEED0 = 900
MAX_SEEDS = 200
ODD_COUNTS = kc.ODD_COUNTS
LOGITS = (0.0, 20.0, -20.0, 90.0, -90.0)
# the offset features of these draws are about a tenth: at 8 a kernel point moves about an extent and few rows lose every
# neighbour; so 32 runs beside it, at which a good part of the rows do and some still keep one (asserted per route by
# the host module)
OF_SCALES = (2.0 ** -20, 1.0, 8.0, 32.0)
GO_SCALES = (2.0 ** -20, 1.0, 2.0 ** 13)
DEFORM_WIDTHS = [1, 63, 64, 65, 128, 129]
REG_WIDTHS = [1, 15, 16, 17, 31, 32, 33, 129]
REG_COUNTS = [1, 3, 4, 5, 15, 16, 17, 33]
REG_BIG_NQ = 16 * 256 + 17
HOST_CU = 256           # the MI355X's compute units: the grid case the host module checks


def kernel_points(radius, seed, n_kp):
    """n_kp <= 15: kpconv_modes_cases.kernel_points_15 cut; 16: one more point at 0.5 .. 1 of the radius."""
    kp = kc.kernel_points_15(radius, seed)
    if n_kp <= 15:
        return kp[:n_kp].contiguous()
    more = fc.random_kernel_points(radius / 1.5, seed + 7, n_kp - 14)[1:]
    return torch.cat([kp, torch.from_numpy(more)], 0).contiguous()


@functools.lru_cache(maxsize=8)
def _cloud(nq, ns, kmax, offset, ext, seed, rows_sorted, fill):
    return fc.kp_cloud_case(nq, ns, kmax, offset, ext, seed, rows_sorted=rows_sorted, fill=fill)


def _same_level_cloud(ns, kmax, offset, ext, seed):
    """q IS s; row n holds the kmax nearest supports, itself first (distance 0), every entry real."""
    _, s, _ = _cloud(ns, ns, kmax, offset, ext, seed, True, 1.0)
    d = np.linalg.norm(s[None].astype(np.float64) - s[:, None].astype(np.float64), axis=2)
    nb = np.argsort(d, axis=1, kind="stable")[:, :kmax]
    assert np.array_equal(nb[:, 0], np.arange(ns))
    return s.copy(), s, nb


def build(route, nq, ns, kmax, offset, ext, seed, modulated, of_seed=OFFSET_SEED0, R=1.25, rows_sorted=True, fill=0.7,
          permute=False, same_level=False, cout=None):
    """dict(q, s, idx, x, w, kp, extent, off_w, off_kp, off_b, modulated, of, route): float32 / int32 CPU tensors.
    R is the search scale in units of the cloud parameter ext (the cloud's half-width is 3 ext).  permute: the columns
    of every row in a seeded random order (real neighbours in every staging chunk).  Unless same_level, q[0] is moved off
    s[0] (kp_cloud_case makes them coincide) by a fifth of the extent: no item sits on kernel point 0 at tiny offsets."""
    impl, cin, rcout, n_kp = ROUTES[route]
    cout = cout or rcout
    R = R * ext
    extent = float(0.8 * R / 2)
    if same_level:
        q, s, nb = _same_level_cloud(ns, kmax, offset, ext, seed)
    else:
        q, s, nb = _cloud(nq, ns, kmax, offset, ext, seed, rows_sorted, fill)
        q = q.copy()
        q[0, 0] += np.float32(0.2 * extent)
    nb = nb.copy()
    if permute:
        r = fc.rng_of(505, seed, kmax)
        for i in range(nb.shape[0]):
            nb[i] = nb[i][r.permutation(kmax)]
    x = fc.kp_features(ns, cin, seed + 1)
    sums = x.astype(np.float64).sum(1)
    x[:, 0] += np.where(np.abs(sums) < 0.05, np.where(sums >= 0, 0.1, -0.1), 0.0).astype(np.float32)
    case = kc.case_from_numpy(q, s, nb, x, fc.kp_weights(cin, cout, seed + 2, n_kp), np.zeros((n_kp, 3)), extent)
    case['kp'] = kernel_points(R / 2, seed + 3, n_kp)
    case['off_kp'] = kernel_points(R / 2, seed + 4, n_kp)
    rng = np.random.default_rng(of_seed)
    od = dc.offset_dim(n_kp, modulated)
    case['off_w'] = torch.from_numpy((rng.uniform(-1, 1, (n_kp, cin, od)) * 0.5 / np.sqrt(n_kp * cin)).astype(np.float32))
    case['off_b'] = torch.from_numpy(rng.uniform(-0.1, 0.1, (od,)).astype(np.float32))
    case['modulated'] = bool(modulated)
    case['route'] = route
    f = lambda k: case[k].double()
    case['of'] = (kc.kpconv_ref(f('q'), f('s'), case['idx'], f('x'), f('off_w'), f('off_kp'), extent) + f('off_b')).float()
    return case


# ---- the float64 references -----------------------------------------------------------------------------------------------
def guarded_ref(q_pts, s_pts, neighb_inds, x, weights, kernel_points, kp_extent, modulated, offset_features):
    """deform_cases.kpconv_deform_ref, the square root restated so that an item with d2 == 0 has h = 1 and no positional
    gradient (the reference's own sqrt has none that is finite there).  aux also holds wf [n, p, c]."""
    K = kernel_points.shape[0]
    of = offset_features
    ns = s_pts.shape[0]
    idx = neighb_inds.long()
    valid = (idx >= 0) & (idx < ns)
    safe = torch.where(valid, idx, torch.zeros_like(idx))
    D = kernel_points + kp_extent * of[:, :3 * K].reshape(-1, K, 3)
    m = 2 * torch.sigmoid(of[:, 3 * K:4 * K]) if modulated else torch.ones_like(of[:, :K])
    far = torch.full_like(s_pts[:1], dc.FAR)
    y = torch.where(valid.unsqueeze(2), s_pts[safe], far) - q_pts.unsqueeze(1)
    d2 = ((y.unsqueeze(2) - D.unsqueeze(1)) ** 2).sum(3)
    in_range = (d2 < kp_extent ** 2).any(2) & valid
    pos = d2 > 0
    dist = torch.where(pos, torch.sqrt(torch.where(pos, d2, torch.ones_like(d2))), torch.zeros_like(d2))
    h = torch.clamp(1 - dist / kp_extent, min=0.0) * in_range.unsqueeze(2).to(d2.dtype)
    nx = x[safe] * valid.unsqueeze(2).to(x.dtype)
    wf = torch.einsum('nkp,nkc->npc', h, nx) * m.unsqueeze(2)
    out = torch.einsum('npc,pco->no', wf, weights)
    count = ((nx.sum(-1) > 0.0) & in_range).sum(-1).clamp(min=1)
    aux = dict(offset_features=of, deformed_KP=D, min_d2=d2.min(1)[0], in_range=in_range, count=count, d2=d2, valid=valid,
               wf=wf.detach())
    return out / count.unsqueeze(1).to(out.dtype), aux


def ref64(case, go=None, guarded=False):
    """(out, aux, grads): float64 at the case's own offset features; grads = dict(dx, dw, d_of) by autograd with go (the
    output gradient), else None.  guarded: guarded_ref instead of deform_cases.kpconv_deform_ref."""
    f = lambda k: case[k].double()
    x, w, of = f('x'), f('w'), f('of')
    if go is not None:
        for t in (x, w, of):
            t.requires_grad_(True)
    if guarded:
        out, aux = guarded_ref(f('q'), f('s'), case['idx'], x, w, f('kp'), case['extent'], case['modulated'], of)
    else:
        out, aux = dc.kpconv_deform_ref(f('q'), f('s'), case['idx'], x, w, f('kp'), case['extent'], case['modulated'],
                                        offset_features=of)
    aux = {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in aux.items()}
    if go is None:
        return out.detach(), aux, None
    out.backward(go.double())
    return out.detach(), aux, dict(dx=x.grad, dw=w.grad, d_of=of.grad)


def conditions(case, aux, x_scale=1.0):
    """deform_cases.conditions and: zeros = valid items at d2 == 0 exactly, floor_nz = the floor over the others.
    x_scale: an exact power of two the features were multiplied by (the row-sum condition is the unscaled tensor's)."""
    c = dc.conditions(case, aux)
    c['row_sum'] = c['row_sum'] / x_scale
    d = torch.sqrt(aux['d2']) / case['extent']
    dv = d[aux['valid']]
    c['zeros'] = int((dv == 0).sum())
    c['floor_nz'] = float(dv[dv > 0].min()) if bool((dv > 0).any()) else float('inf')
    return c


def check_conditions(case, aux, zeros=False, x_scale=1.0):
    c = conditions(case, aux, x_scale)
    assert c['gap'] >= dc.GAP_MIN, f"a neighbour within {c['gap']:.2e} e of the range cut"
    assert c['row_sum'] >= dc.SUM_MIN, f"a feature row sums to {c['row_sum']:.2e}"
    if zeros:
        assert c['zeros'] > 0 and c['floor_nz'] >= dc.DIST_MIN, (c['zeros'], c['floor_nz'])
    else:
        assert c['floor'] >= dc.DIST_MIN, f"a neighbour within {c['floor']:.2e} e of a kernel point"
    return c


def _meets(case, zeros):
    _, aux, _ = ref64(case, guarded=zeros)
    try:
        check_conditions(case, aux, zeros)
    except AssertionError:
        return False
    return True


def _reg_meets(case, _zeros=False):
    return rc.argmin_gap(case, case['of']) >= rc.GAP_MIN


class Spec:
    """make(of_seed) -> case; zeros: the case holds items at d2 == 0; meets: the float64 condition the seed is chosen by."""

    def __init__(self, make, zeros=False, meets=_meets):
        self.make, self.zeros, self.meets = make, zeros, meets


_SEEDS = {}


def first_seed(name, spec):
    if name not in _SEEDS:
        for seed in range(OFFSET_SEED0, OFFSET_SEED0 + MAX_SEEDS):
            if spec.meets(spec.make(seed), spec.zeros):
                _SEEDS[name] = seed
                break
        else:
            raise AssertionError(f"{name}: no offset seed in {MAX_SEEDS} meets the float64 conditions")
    return _SEEDS[name]


def get(name, table=None):
    spec = (CASES if table is None else table)[name]
    return spec.make(first_seed(name, spec))


# ---- modifiers (applied after the offsets are formed: the offsets are an input like any other) ------------------------------
def _in_range64(case):
    return ref64(case)[1]['in_range']


def shift_rows(case, rows, shift):
    """The whole kernel of the given rows moved by `shift` extents along every axis: every valid neighbour is cut."""
    K = case['kp'].shape[0]
    case['of'][rows, :3 * K] = float(shift)
    return case


CUT_ROWS = list(range(8, 24))
NEG_ROWS = list(range(4, 16))
DUP_ROWS = list(range(16, 28))


def cut_case(case):
    return shift_rows(case, CUT_ROWS, 40.0)


def odd_in_range_case(case):
    """Row r keeps ODD_COUNTS[r % 4] of its in-range neighbours (float64 in_range), the surplus becomes shadow; rows with
    fewer stay as they are.  The out-of-range valid entries stay in the row, between the kept ones."""
    inr = _in_range64(case)
    ns = case['s'].shape[0]
    for r in range(inr.shape[0]):
        cols = torch.nonzero(inr[r]).flatten()
        case['idx'][r, cols[ODD_COUNTS[r % 4]:]] = ns
    return case


def edge_rows_case(case):
    """NEG_ROWS: every in-range neighbour's feature row is made negative (count clamps at 1, the numerator lives);
    DUP_ROWS: columns 1 and 2 repeat column 0's index; every third shadow entry becomes -1, every third ns + 5."""
    inr = _in_range64(case)
    idx, ns = case['idx'], case['s'].shape[0]
    for r in NEG_ROWS:
        sup = idx[r][inr[r]].long()
        case['x'][sup] = -case['x'][sup].abs() - 0.05
    for r in DUP_ROWS:
        idx[r, 1] = idx[r, 0]
        idx[r, 2] = idx[r, 0]
    sh = torch.nonzero(idx.view(-1) == ns).flatten()
    idx.view(-1)[sh[0::3]] = -1
    idx.view(-1)[sh[1::3]] = ns + 5
    return case


def logits_case(case):
    K = case['kp'].shape[0]
    n = case['of'].shape[0]
    pick = (torch.arange(n).unsqueeze(1) + torch.arange(K).unsqueeze(0)) % len(LOGITS)
    case['of'][:, 3 * K:] = torch.tensor(LOGITS, dtype=torch.float32)[pick]
    return case


def scale_of(case, s):
    case['of'] = case['of'] * float(s)
    return case


def zero_kp0(case):
    """Zero offsets at kernel point 0 (kp[0] == 0): in a same-level case every query is on it, d2 == 0 exactly."""
    case['of'][:, 0:3] = 0.0
    return case


def late_chunk_case(case):
    """Rows of 129 sorted columns under a small kernel moved, per row, onto a far real neighbour (0.3 extents beside it) --
    the last one in the even rows (column 128: the third staging chunk), column 100 in the odd rows (the second): what is
    in range lies about that neighbour, farther from the query than the first 64 columns."""
    K, e = case['kp'].shape[0], case['extent']
    idx, ns = case['idx'].long(), case['s'].shape[0]
    r = fc.rng_of(506, idx.shape[0])
    for n in range(idx.shape[0]):
        cols = torch.nonzero((idx[n] >= 0) & (idx[n] < ns)).flatten()
        if cols.numel() == 0:
            continue
        target = cols[-1] if n % 2 == 0 else cols[min(100, cols.numel() - 1)]
        y = case['s'][idx[n, target]].double() - case['q'][n].double()
        v = r.standard_normal(3)
        shift = y / e + torch.from_numpy(0.3 * v / np.linalg.norm(v))
        case['of'][n, :3 * K] = shift.float().repeat(K)
    return case


def saturating_case(route, edge, of_seed):
    """Same-level rows of 16 copies of the query's own index, zero offset on kernel point 0, logit +90 (m == 2 exactly),
    constant features at 4 or one float32 step from it: wf[n, 0, :] == 2 * 16 * x, the bound the tile kernel scales by."""
    case = zero_kp0(build(route, 65, 65, kc.MAG_KMAX, 1e2, 0.125, 71, True, of_seed, same_level=True))
    K = case['kp'].shape[0]
    case['idx'] = torch.arange(65, dtype=torch.int32).unsqueeze(1).repeat(1, kc.MAG_KMAX)
    case['of'][:, 3 * K:] = 90.0
    four = np.float32(4.0)
    v = {"at": four, "below": np.nextafter(four, np.float32(0)), "above": np.nextafter(four, np.float32(8))}[edge]
    case['x'] = torch.full_like(case['x'], float(v))
    return case


def sparse_rows_case(case):
    """The regulariser's row edges: rows 8..15 all shadow, rows 16..23 a single real neighbour (column 0)."""
    ns = case['s'].shape[0]
    case['idx'][8:16] = ns
    case['idx'][16:24, 1:] = ns
    return case


# ---- the cases --------------------------------------------------------------------------------------------------------------
CASES, REG_CASES = {}, {}
srt_id = lambda s: "sorted" if s else "unsorted"


def _add(table, name, make, zeros=False, meets=_meets):
    assert name not in table, name
    table[name] = Spec(make, zeros, meets)
    return name


def offset_name(route, offset, ext, srt, mod):
    return f"offset {route} {offset:g} {ext:g} {srt_id(srt)} {mod_id(mod)}"


def width_name(route, kmax, variant, mod):
    return f"width {route} {kmax} {variant} {mod_id(mod)}"


def count_name(route, nq, mod):
    return f"count {route} {nq} {mod_id(mod)}"


def grid_name(route):
    return f"grid {route}"


def edge_name(kind, route, mod):
    return f"{kind} {route} {mod_id(mod)}"


def _base(route, mod, seed, nq=64, R=1.25, fill=0.7):
    return lambda s: build(route, nq, 120, 12, 1e2, 0.125, seed, mod, s, R=R, fill=fill)


WIDTH_VARIANTS = ("sorted", "unsorted")
WIDE_VARIANTS = ("late chunk", "full chunk")


def _populate():
    P = functools.partial
    for mod in MOD:
        for route in FWD_ROUTES:
            for offset, ext in kc.OFFSETS:
                for srt in (True, False):
                    _add(CASES, offset_name(route, offset, ext, srt, mod),
                         P(lambda s, route, offset, ext, srt, mod: build(route, 300, 350, 20, offset, ext, 41, mod, s,
                                                                         rows_sorted=srt),
                           route=route, offset=offset, ext=ext, srt=srt, mod=mod))
            for nq in kc.QUERY_COUNTS:
                _add(CASES, count_name(route, nq, mod),
                     P(lambda s, route, nq, mod: build(route, nq, 120, 12, 1e2, 0.125, 49, mod, s), route=route, nq=nq,
                       mod=mod))
            _add(CASES, edge_name("cut", route, mod), P(lambda s, mk: cut_case(mk(s)), mk=_base(route, mod, 57)))
            _add(CASES, edge_name("odd", route, mod),
                 P(lambda s, mk: odd_in_range_case(mk(s)), mk=_base(route, mod, 61, nq=48, R=3.0, fill=1.0)))
            _add(CASES, edge_name("edges", route, mod), P(lambda s, mk: edge_rows_case(mk(s)), mk=_base(route, mod, 59)))
            for sc in OF_SCALES:
                _add(CASES, edge_name(f"of*{sc:g}", route, mod),
                     P(lambda s, mk, sc: scale_of(mk(s), sc), mk=_base(route, mod, 63, nq=100), sc=sc))
        for route in ("tile32", "tile64", "simple48"):
            for kmax in DEFORM_WIDTHS:
                for variant in WIDTH_VARIANTS:
                    _add(CASES, width_name(route, kmax, variant, mod),
                         P(lambda s, route, kmax, variant, mod: build(route, 70, 200, kmax, 1e2, 0.25, 45, mod, s, R=2.0,
                                                                      fill=0.9, permute=variant == "unsorted"),
                           route=route, kmax=kmax, variant=variant, mod=mod))
            _add(CASES, width_name(route, 129, "late chunk", mod),
                 P(lambda s, route, mod: late_chunk_case(build(route, 70, 200, 129, 1e2, 0.25, 45, mod, s, R=0.5, fill=1.0)),
                   route=route, mod=mod))
            _add(CASES, width_name(route, 129, "full chunk", mod),
                 P(lambda s, route, mod: build(route, 70, 200, 129, 1e2, 0.25, 45, mod, s, R=16.0, fill=1.0), route=route,
                   mod=mod))
            _add(CASES, edge_name("zero", route, mod),
                 P(lambda s, route, mod: zero_kp0(build(route, 96, 96, 12, 1e2, 0.125, 65, mod, s, same_level=True)),
                   route=route, mod=mod), zeros=True)
        for route in ("kp1", "kp7", "kp16"):
            _add(CASES, edge_name("points", route, mod), _base(route, mod, 67, nq=37))
        for route in TILE_ROUTES:
            _add(CASES, edge_name("mag", route, mod),
                 P(lambda s, route, mod: build(route, 65, 120, kc.MAG_KMAX, 1e2, 0.125, 71, mod, s), route=route, mod=mod))
    for route in FWD_ROUTES:
        _add(CASES, edge_name("logits", route, True), P(lambda s, mk: logits_case(mk(s)), mk=_base(route, True, 69)))
    for route in TILE_ROUTES:
        for edge in kc.POW2_EDGES:
            _add(CASES, f"saturating {route} {edge}", P(saturating_case, route, edge), zeros=True)
    # the regulariser: q, s, idx, kp, extent and of of the same builders; the condition is the argmin gap
    for mod in MOD:
        for offset, ext in kc.OFFSETS:
            for srt in (True, False):
                _add(REG_CASES, f"reg offset {offset:g} {ext:g} {srt_id(srt)} {mod_id(mod)}",
                     P(lambda s, offset, ext, srt, mod: build("tile32", 300, 350, 20, offset, ext, 41, mod, s, rows_sorted=srt),
                       offset=offset, ext=ext, srt=srt, mod=mod), meets=_reg_meets)
        for sc in OF_SCALES:
            _add(REG_CASES, f"reg of*{sc:g} {mod_id(mod)}",
                 P(lambda s, mk, sc: scale_of(mk(s), sc), mk=_base("tile32", mod, 63, nq=100), sc=sc), meets=_reg_meets)
        for kmax in REG_WIDTHS:
            _add(REG_CASES, f"reg width {kmax} {mod_id(mod)}",
                 P(lambda s, kmax, mod: build("tile32", 40, 200, kmax, 1e2, 0.25, 45, mod, s, R=2.0, fill=0.9, permute=True),
                   kmax=kmax, mod=mod), meets=_reg_meets)
        for nq in REG_COUNTS:
            _add(REG_CASES, f"reg count {nq} {mod_id(mod)}",
                 P(lambda s, nq, mod: build("tile32", nq, 120, 12, 1e2, 0.125, 49, mod, s), nq=nq, mod=mod),
                 meets=_reg_meets)
        for route in ("kp1", "kp16"):
            _add(REG_CASES, f"reg points {route} {mod_id(mod)}", _base(route, mod, 67, nq=37), meets=_reg_meets)
        _add(REG_CASES, f"reg rows {mod_id(mod)}", P(lambda s, mk: sparse_rows_case(mk(s)), mk=_base("tile32", mod, 73)),
             meets=_reg_meets)
    _add(REG_CASES, "reg many workgroups",
         lambda s: build("tile32", REG_BIG_NQ, 200, 5, 1e2, 0.125, 75, True, s), meets=_reg_meets)


_populate()


def grid_case(route, n_cu):
    """(name, Spec) of the forward-only case with more tiles than the tile kernel's grid on a device of n_cu compute
    units: kmax 5, cout 32, modulated."""
    cc = 64 if ROUTES[route][1] % 64 == 0 else 32
    nq = grid_nq(n_cu, cc)
    return f"{grid_name(route)} {nq}", Spec(lambda s: build(route, nq, 200, 5, 1e2, 0.125, 51, True, s, cout=32))


def get_grid(route, n_cu):
    name, spec = grid_case(route, n_cu)
    return spec.make(first_seed(name, spec))
