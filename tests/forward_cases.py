"""Seeded case generators and float64 references of the encoder's non-GEMM forward operators, shared by
tests/test_gpu_forward_range.py (the HIP kernels) and tests/test_forward_range_host.py (which checks, without a GPU,
that these references agree with oracle/torch_oracle.py and that no generated case is vacuous).

Every reference is a float64 restatement of the operation's definition fed the same float32 inputs; every
`*_f32` function is the reference project's own float32 arithmetic on torch-CPU (F.instance_norm, F.layer_norm,
position_embedding.py's expression) -- the baseline of the rule  err <= max(bound * scale, 4 * err32)  that
tests/test_gpu_range.py uses where float32 itself cannot hold a fixed bound."""
import math

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64


def rng_of(*key):
    return np.random.default_rng([int(k) & 0x7FFFFFFF for k in key])


# ---- 1. InstanceNorm (+ add + LeakyReLU) ---------------------------------------------------------------------------
# ragged lengths of one call: 1, 2, 3, the 256-thread edges, one cloud of several 512-row statistics slices, and a last
# cloud that makes the total odd -- n * (c / 4) float4s are then no multiple of kInApplyUnroll * 256 = 1024 for any
# width of IN_WIDTHS (c / 4 <= 64 divides 1024, n odd does not)
IN_LENGTHS = [1, 2, 3, 255, 256, 257, 1300, 77]
IN_LENGTHS_EMPTY = [5, 0, 300, 0, 41]            # zero-length clouds inside a batch
IN_WIDTHS = [4, 32, 64, 68, 128, 192, 256]
IN_REGIMES = [(0.0, 1.0), (1e3, 1e-2), (0.0, 1e-4), (0.0, 1e-20), (0.0, 1e15)]
IN_EPS = 1e-5


def in_data(lengths, c, centre, spread, seed):
    """float32 [sum lengths, c]: per-channel centres around `centre` (so that channels differ), N(0, spread) inside."""
    r = rng_of(101, seed, c)
    n = int(sum(lengths))
    ch = centre * (1.0 + 0.25 * r.uniform(-1, 1, (1, c)))
    return torch.from_numpy((ch + spread * r.standard_normal((n, c))).astype(np.float32))


def in_constant(lengths, c, seed):
    """Every cloud constant per channel: variance exactly 0, eps alone decides the scale."""
    r = rng_of(102, seed, c)
    rows = [np.repeat(r.uniform(-3, 3, (1, c)), l, 0) for l in lengths]
    return torch.from_numpy(np.concatenate(rows, 0).astype(np.float32))


def in_add(n, c, seed):
    return torch.from_numpy(rng_of(103, seed, c).uniform(-1, 1, (n, c)).astype(np.float32))


def _lrelu64(y, slope):
    return torch.where(y >= 0, y, y * slope)


def instnorm_stats_f64(x, lengths, eps=IN_EPS):
    """(mean, rstd) [nb, c] in float64: biased variance, eps inside the root (nn.InstanceNorm1d per cloud); a cloud
    without rows has mean 0 and variance 0."""
    xs = x.to(F64)
    c = x.shape[1]
    mean, rstd, off = [], [], 0
    for l in lengths:
        seg = xs[off:off + l]
        m = seg.sum(0) / l if l > 0 else torch.zeros(c, dtype=F64)
        v = ((seg - m) ** 2).sum(0) / l if l > 0 else torch.zeros(c, dtype=F64)
        mean.append(m)
        rstd.append(1.0 / torch.sqrt(v + eps))
        off += l
    return torch.stack(mean), torch.stack(rstd)


def instnorm_f64(x, lengths, eps=IN_EPS, norm=True, add=None, slope=1.0):
    y = x.to(F64)
    if norm:
        mean, rstd = instnorm_stats_f64(x, lengths, eps)
        seg = torch.repeat_interleave(torch.arange(len(lengths)), torch.as_tensor(lengths))
        y = (y - mean[seg]) * rstd[seg]
    if add is not None:
        y = y + add.to(F64)
    return _lrelu64(y, slope)


def instnorm_f32(x, lengths, eps=IN_EPS, norm=True, add=None, slope=1.0):
    """The reference's arithmetic: F.instance_norm per cloud in float32 (kpconv_blocks.py:510-519), then the add and
    F.leaky_relu.  (torch refuses a one-point cloud in this mode; its normalised value is 0 by definition.)"""
    y = x
    if norm:
        outs, off = [], 0
        for l in lengths:
            seg = x[off:off + l]
            if l == 1:
                outs.append(torch.zeros_like(seg))
            elif l > 1:
                outs.append(F.instance_norm(seg.t().unsqueeze(0), eps=eps).squeeze(0).t())
            off += l
        y = torch.cat(outs, 0)
    if add is not None:
        y = y + add
    return F.leaky_relu(y, slope)


# ---- 2. LayerNorm (+ pos) ------------------------------------------------------------------------------------------
LN_ROWS = [1, 3, 255, 257, 4100]
LN_WIDTHS = [64, 192, 256, 512, 1024]
LN_REGIMES = [(0.0, 3.0), (1e3, 1e-2)]


def ln_data(m, c, centre, spread, seed):
    r = rng_of(201, seed, m, c)
    x = centre + spread * r.standard_normal((m, c))
    return (torch.from_numpy(x.astype(np.float32)), torch.from_numpy(r.uniform(0.5, 1.5, c).astype(np.float32)),
            torch.from_numpy(r.uniform(-1, 1, c).astype(np.float32)),
            torch.from_numpy(r.uniform(-1, 1, (m, c)).astype(np.float32)))


def layernorm_f64(x, gamma, beta, eps=1e-5):
    xs = x.to(F64)
    m = xs.mean(1, keepdim=True)
    v = ((xs - m) ** 2).mean(1, keepdim=True)
    return (xs - m) / torch.sqrt(v + eps) * gamma.to(F64) + beta.to(F64)


def layernorm_f32(x, gamma, beta, eps=1e-5):
    return F.layer_norm(x, (x.shape[1],), gamma, beta, eps)


# ---- 3. max-pool / gather_rows -------------------------------------------------------------------------------------
MP_K = [1, 2, 3, 4, 5, 7, 8, 33]
MP_WIDTHS = [4, 32, 64, 128, 256]
F32_MAX = float(np.finfo(np.float32).max)


def maxpool_np(x, idx):
    """kpconv_blocks.py:127-143: a zero shadow row is appended, every index outside [0, ns) selects it."""
    x = np.asarray(x, np.float32)
    idx = np.asarray(idx, np.int64)
    ns = x.shape[0]
    x_ext = np.concatenate([x, np.zeros((1, x.shape[1]), np.float32)], 0)
    idx = np.where((idx < 0) | (idx >= ns), ns, idx)
    return x_ext[idx].max(1)


def gather_np(x, idx):
    return maxpool_np(x, np.asarray(idx).reshape(-1, 1))


def mp_case(ns, nq, k, c, seed):
    """Features of every sign, and a neighbour matrix whose first rows are the edge rows (the tuple's third entry names
    them): all shadow / negative features with one shadow column / negative features without shadow."""
    r = rng_of(301, seed, k, c)
    x = r.uniform(-2, 1, (ns, c)).astype(np.float32)
    x[:8] = -np.abs(x[:8]) - 0.25                       # support rows 0..7: strictly negative in every channel
    idx = r.integers(0, ns, (nq, k))
    idx[r.random((nq, k)) < 0.2] = ns                   # shadow entries anywhere
    rows = {"all_shadow": 0, "neg_one_shadow": 1, "neg_no_shadow": 2}
    idx[0] = ns
    idx[1] = r.integers(0, 8, k)
    idx[1, k - 1] = ns
    idx[2] = r.integers(0, 8, k)
    return x, idx.astype(np.int64), rows


def mp_extreme(k, c, seed):
    """Features at the ends of the float32 range: rows whose true maximum is -FLT_MAX, lies below -3.0e38, or is -inf;
    rows of +FLT_MAX and +inf; and the same with a shadow column (the zero row then wins or loses)."""
    r = rng_of(302, seed, k, c)
    vals = np.array([-np.inf, -F32_MAX, -3.2e38, -3.0e38, -1e30, 1e30, F32_MAX, np.inf], np.float32)
    ns = 4 * len(vals)
    x = np.empty((ns, c), np.float32)
    for i, v in enumerate(vals):                          # four support rows per value
        x[4 * i:4 * i + 4] = v
    x[1::4, ::2] = r.uniform(-1, 1, x[1::4, ::2].shape)   # mixed rows: every other channel finite
    rows = []
    for i in range(len(vals)):
        rows.append(r.integers(4 * i, 4 * i + 4, k))      # only this value class
        sh = r.integers(4 * i, 4 * i + 4, k)
        sh[r.integers(0, k)] = ns                          # ... and one shadow entry
        rows.append(sh)
    rows.append(r.integers(0, 12, k))                      # -inf, -FLT_MAX and -3.2e38 together
    return x, np.asarray(rows, np.int64)


# ---- 4. sine position embedding ------------------------------------------------------------------------------------
PE_MAGS = [1e-3, 1.0, 10.0, 100.0, 1e3]
PE_ROWS = [1, 255, 257]
PE_EXTRA_SCALES = [0.25, 2.0]   # beside the configs' (all 1.0)
PE_DMODEL = [256, 200]      # 200: npf = 66, 3 * npf = 198 -> 2 padding columns; 256: npf = 84 -> 4


def pe_xyz(n, mag, seed):
    return torch.from_numpy(rng_of(401, seed, n).uniform(-mag, mag, (n, 3)).astype(np.float32))


def posemb_f64(xyz, d_model, scale=1.0, temperature=10000.0):
    """position_embedding.py:29-50 in float64 on the float32 coordinates: channel 3-blocks of npf columns per axis,
    sin at even and cos at odd positions of  x * 2 pi scale / temperature^(2 (i // 2) / npf),  zero padding behind."""
    npf = d_model // 3 // 2 * 2
    i = np.arange(npf)
    dim_t = np.float64(temperature) ** (2.0 * (i // 2) / npf)
    a = xyz.to(F64).numpy()[:, :, None] * (scale * 2.0 * math.pi) / dim_t[None, None, :]
    emb = np.where((i % 2 == 0)[None, None, :], np.sin(a), np.cos(a)).reshape(xyz.shape[0], 3 * npf)
    out = np.zeros((xyz.shape[0], d_model))
    out[:, :3 * npf] = emb
    return torch.from_numpy(out)


def posemb_f32(xyz, d_model, scale=1.0, temperature=10000):
    """The reference's expression in float32 (position_embedding.py:29-50)."""
    npf = d_model // 3 // 2 * 2
    dim_t = torch.arange(npf, dtype=torch.float32)
    dim_t = temperature ** (2 * torch.div(dim_t, 2, rounding_mode='trunc') / npf)
    pos = (xyz * (scale * 2 * math.pi)).unsqueeze(-1) / dim_t
    emb = torch.stack([pos[..., 0::2].sin(), pos[..., 1::2].cos()], dim=-1).reshape(xyz.shape[0], -1)
    return F.pad(emb, (0, d_model - 3 * npf))


# ---- 5. KPConv geometry --------------------------------------------------------------------------------------------
# route name -> (impl, cin, cout, kmax bound): the conditions of ops.kpconv_raw / spr_kpconv_fwd
KP_ROUTES = {
    "ring32": (0, 32, 32), "ring64": (0, 64, 64), "ring32x128": (0, 32, 128),
    "tile_cin128": (0, 128, 64), "tile_big_w": (0, 64, 128), "tile_impl2": (2, 32, 32), "tile_impl2_64": (2, 64, 64),
    "simple_impl1": (1, 32, 32), "cin1": (0, 1, 64), "generic48": (0, 48, 24),
}


def kp_route(impl, cin, cout, kmax, n_kp=15):
    """The kernel a call reaches, restated from spr_kpconv_fwd's dispatch (csrc/kpconv.hip)."""
    if cin == 1 and impl in (0, 2) and n_kp <= 16:
        return "cin1"
    if impl in (0, 2) and n_kp == 15 and cin % 32 == 0 and cout % 32 == 0 and cout <= 256:
        ring = impl == 0 and cin in (32, 64) and cin * cout <= 4096 and 8 % (cout // 16) == 0 and kmax <= 128
        if ring:
            return "ring"
        # the tile kernel's LDS holds neighbour rows of up to 128 entries at 32-channel chunks, 272 at 64
        fits = kmax <= (272 if cin % 64 == 0 else 128)
        if fits and ((cin % 64 == 0 and cout in (64, 128, 256)) or (cin % 64 != 0 and cout in (32, 64, 128))):
            return "tile"
    return "simple"


def lattice_kernel_points(ext):
    """15 kernel points on a lattice of ext / 4: the centre at the origin, 6 axis points at 3/4 ext, 8 cube corners
    at (+-1/2 ext)^3 -- all exactly representable next to coordinates up to 2^10 when ext is a power of two >= 2^-6."""
    a, b = 0.75 * ext, 0.5 * ext
    pts = [(0, 0, 0)]
    for ax in range(3):
        for s in (1, -1):
            p = [0, 0, 0]
            p[ax] = s * a
            pts.append(tuple(p))
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                pts.append((sx * b, sy * b, sz * b))
    return np.asarray(pts, np.float32)


def random_kernel_points(ext, seed, n_kp=15):
    """Centre at the origin + n_kp - 1 points in the ball of radius 1.5 ext (the disposition's scale: radius = 1.5
    extent)."""
    r = rng_of(501, seed)
    v = r.standard_normal((n_kp - 1, 3))
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * (r.uniform(0.5, 1.0, (n_kp - 1, 1)) * 1.5 * ext)
    return np.concatenate([np.zeros((1, 3)), v], 0).astype(np.float32)


def kp_features(ns, cin, seed, integer=False):
    r = rng_of(502, seed, cin)
    if integer:
        return r.integers(-2, 3, (ns, cin)).astype(np.float32)     # small integers: a row sum is exact in any order
    return (r.random((ns, cin)) - 0.4).astype(np.float32)


def kp_weights(cin, cout, seed, n_kp=15):
    return ((rng_of(503, seed, cin, cout).random((n_kp, cin, cout)) - 0.5) * 0.5).astype(np.float32)


def kp_cloud_case(nq, ns, kmax, offset, ext, seed, rows_sorted=True, fill=0.7):
    """KITTI-like geometry: a cloud of diameter ~6 ext around (offset, -offset, offset / 2), queries next to support
    points, the kmax nearest supports as neighbours, `fill` of them valid (shadow = ns, trailing when rows_sorted)."""
    r = rng_of(504, seed, nq, kmax)
    c0 = np.array([offset, -offset, 0.5 * offset])
    s = (c0 + r.uniform(-3 * ext, 3 * ext, (ns, 3))).astype(np.float32)
    q = (s[r.integers(0, ns, nq)].astype(np.float64) + r.normal(0, 0.2 * ext, (nq, 3))).astype(np.float32)
    q[0] = s[0]                                                     # query and support coincident, at index 0
    d = np.linalg.norm(s[None].astype(np.float64) - q[:, None].astype(np.float64), axis=2)
    kk = min(kmax, ns)
    nb = np.full((nq, kmax), ns, np.int64)
    nb[:, :kk] = np.argsort(d, axis=1, kind="stable")[:, :kk]
    valid = r.random((nq, kmax)) < fill
    valid[:, 0] = True
    valid[:, kk:] = False
    if nq > 3:
        valid[3] = False                                            # a row of only shadow entries
    if rows_sorted:
        valid = np.arange(kmax)[None, :] < valid.sum(1)[:, None]
    else:
        valid[:, 0] = r.random(nq) < 0.5                            # shadow entries in front too
        valid[0, 0] = True
    return q, s, np.where(valid, nb, ns)


def kp_exact_case(offset, ext, kmax=8):
    """Exact geometry on a lattice (ext a power of two, kernel points = lattice_kernel_points(ext)).  One query per
    situation, all at the same lattice position; the support points are placed relative to it:
      row 0  the support coincides with the query (influence 1 of the centre kernel point)
      row 1..14  a support exactly on kernel point p (influence exactly 1 there)
      row 15 a support at distance exactly ext from the centre along x (influence exactly 0 of the centre point)
      row 16 / 17  one representable step inside / outside that distance
      row 18 all of the above as one neighbourhood
    Returns (q, s, nb, names)."""
    kp = lattice_kernel_points(ext).astype(np.float64)
    base = np.array([offset, -offset, 0.5 * offset], np.float32).astype(np.float64)
    rel = [kp[p] for p in range(15)]
    rel.append(np.array([ext, 0, 0]))
    x_at = np.float32(base[0] + ext)
    rel.append(np.array([np.float64(np.nextafter(x_at, np.float32(-np.inf))) - base[0], 0, 0]))
    rel.append(np.array([np.float64(np.nextafter(x_at, np.float32(np.inf))) - base[0], 0, 0]))
    s = (base[None] + np.asarray(rel)).astype(np.float32)
    assert np.array_equal(s.astype(np.float64), base[None] + np.asarray(rel)), "lattice not representable"
    ns = s.shape[0]
    nq = ns + 1
    q = np.repeat(base[None].astype(np.float32), nq, 0)
    nb = np.full((nq, max(kmax, ns)), ns, np.int64)
    nb[np.arange(ns), 0] = np.arange(ns)
    nb[ns, :ns] = np.arange(ns)
    names = {"coincident": 0, "on_kp": list(range(1, 15)), "at_extent": 15, "inside": 16, "outside": 17, "all": 18}
    return q, s, nb, names


def kpconv_f64(q, s, nb, x, w, kp, ext):
    """KPConv.forward (rigid, linear influence, sum aggregation; kpconv_blocks.py:309-412) in float64 numpy: shadow
    neighbours carry zero features, influence max(0, 1 - |s - q - kp| / ext), the sum over kernel points of
    (influence-weighted features) @ W[p], divided by max(1, #{neighbours whose feature sum is > 0})."""
    q, s, x, w, kp = (np.asarray(a, np.float64) for a in (q, s, x, w, kp))
    nb = np.asarray(nb, np.int64)
    ns = s.shape[0]
    ok = (nb >= 0) & (nb < ns)
    idx = np.where(ok, nb, 0)
    rel = s[idx] - q[:, None, :]                                               # [nq, K, 3]
    dist = np.sqrt(((rel[:, :, None, :] - kp[None, None]) ** 2).sum(-1))       # [nq, K, 15]
    infl = np.maximum(0.0, 1.0 - dist / ext) * ok[:, :, None]
    nx = x[idx] * ok[:, :, None]                                               # [nq, K, cin]
    wf = np.einsum("nkp,nkc->npc", infl, nx)
    out = np.einsum("npc,pco->no", wf, w)
    cnt = ((nx.sum(-1) > 0) & ok).sum(1)
    return out / np.maximum(cnt, 1)[:, None]
