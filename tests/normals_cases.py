"""Host side of the surface-normal tests: the float64 restatement of include/spr.h ("surface normals") and the checks
tests/test_gpu_normals.py applies to what the device returns.  Nothing here needs a GPU.

The estimator's contract is stated on the neighbour MATRIX, so the reference takes the matrix the device search
returned (or a hand-made one) and the exactly converted float32 points; numpy.linalg.eigh gives eigenvalues in
ascending order and unit eigenvectors.

Bounds, with u = 2^-24 and K = kmax + 8 (the kernel's result is an exact eigenvector of a covariance within K u |C| of
C: kmax / 8 + 3 additions per moment, a product, the mean's subtraction, the scaling by the trace and the Jacobi
rotations are all well inside K roundings):
  every valid row   | |n| - 1 | <= 4 * 2^-23   and   n^T C n <= l0 + 2 K u l2
  gap rows          g = (l1 - l0) / l2 >= 1e-2:   |n x n_ref| <= K u / g   (the eigenvector perturbation bound)
  curvature         |c - c_ref| <= K u
  sign              the rule of the contract, except where the deciding quantity is within 1e-3 relative of a tie.
"""
import numpy as np

U = 2.0 ** -24
GAP = 1e-2
GAP_SHARE_CAP = 0.05
TIE = 1e-3
SHADOWS = np.array([-1, -(1 << 31), (1 << 31) - 1], dtype=np.int64)    # plus N and N + 5, added per case


def rot_matrix(seed: int) -> np.ndarray:
    """A proper rotation, float64, from a seeded QR."""
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q


def reference(points: np.ndarray, nbr: np.ndarray) -> dict:
    """points [N,3] float32, nbr [N,K] integer.  Returns m [N], C [N,3,3], lam [N,3] ascending, vec [N,3] (unit, sign
    arbitrary; zero where m < 3), curv [N], all float64."""
    p = points.astype(np.float64)
    n = len(p)
    nbr = nbr.astype(np.int64)
    ok = (nbr >= 0) & (nbr < n)
    m = ok.sum(1)
    d = p[np.where(ok, nbr, 0)] - p[:, None, :]
    d = d * ok[:, :, None]
    mm = np.maximum(m, 1)[:, None]
    mu = d.sum(1) / mm
    e = (d - mu[:, None, :]) * ok[:, :, None]
    C = np.einsum('nki,nkj->nij', e, e) / mm[:, :, None]
    lam, vecs = np.linalg.eigh(C)
    vec = vecs[:, :, 0].copy()
    tr = lam.sum(1)
    curv = np.where(tr > 0, lam[:, 0] / np.where(tr > 0, tr, 1.0), 0.0)
    few = m < 3
    vec[few] = 0.0
    curv[few] = 0.0
    return {'m': m, 'C': C, 'lam': lam, 'vec': vec, 'curv': curv}


def per_point_view(viewpoint, lens, n):
    """[N,3] float64 viewpoint of every point's cloud, or None."""
    if viewpoint is None:
        return None
    v = np.asarray(viewpoint, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    assert len(v) == len(lens) and sum(lens) == n
    return np.repeat(v, np.asarray(lens, dtype=np.int64), axis=0)


def sign_rule(vec: np.ndarray, points: np.ndarray, view) -> tuple:
    """(s [N] in {+1, -1}: the factor the contract's rule applies to vec; tie [N] bool: the deciding quantity is within
    TIE relative of a tie, so either sign is accepted)."""
    a = np.abs(vec)
    order = np.argsort(-a, axis=1, kind='stable')               # the lowest index among equal magnitudes
    top = np.take_along_axis(vec, order[:, :1], 1)[:, 0]
    a0, a1 = np.take_along_axis(a, order[:, :1], 1)[:, 0], np.take_along_axis(a, order[:, 1:2], 1)[:, 0]
    s = np.where(top < 0, -1.0, 1.0)
    tie = (a0 - a1) <= TIE * a0
    if view is not None:
        w = view - points.astype(np.float64)
        dot = (vec * w).sum(1)
        wn = np.linalg.norm(w, axis=1)
        s = np.where(dot < 0, -1.0, np.where(dot > 0, 1.0, s))
        tie = np.abs(dot) <= TIE * wn                           # an exact 0 falls back to the rule above: also a tie
    return s, tie


def check(points: np.ndarray, nbr: np.ndarray, lens, viewpoint, normals: np.ndarray, curv, what: str,
          cap_gap_share: bool = True) -> dict:
    """Every assertion of the estimator's contract on one result.  Prints the figures before it asserts; returns the
    reference (with 'gap_rows' and 'signed': n_ref under the sign rule)."""
    n, kmax = len(points), nbr.shape[1]
    K = kmax + 8
    ref = reference(points, nbr)
    got = normals.astype(np.float64)
    assert normals.dtype == np.float32 and normals.shape == (n, 3), what
    valid = ref['m'] >= 3
    assert np.array_equal(normals[~valid].view(np.uint32), np.zeros((int((~valid).sum()), 3), np.uint32)), \
        f"{what}: rows with fewer than 3 neighbours are not exactly zero"
    lam, C = ref['lam'], ref['C']
    length = np.linalg.norm(got[valid], axis=1)
    rq = np.einsum('ni,nij,nj->n', got, C, got)[valid]
    slack = 2 * K * U * lam[valid, 2]
    excess = (rq - lam[valid, 0]) / np.maximum(lam[valid, 2], 1e-300)
    gap = (lam[:, 1] - lam[:, 0]) / np.where(lam[:, 2] > 0, lam[:, 2], 1.0)
    gap_rows = valid & (gap >= GAP) & (lam[:, 2] > 0)
    share = 1.0 - gap_rows.sum() / max(int(valid.sum()), 1)
    cross = np.linalg.norm(np.cross(got, ref['vec']), axis=1)
    ratio = (cross[gap_rows] * gap[gap_rows] / (K * U)) if gap_rows.any() else np.zeros(1)
    view = per_point_view(viewpoint, lens, n)
    s_got, tie_got = sign_rule(got, points, view)
    s_ref, tie_ref = sign_rule(ref['vec'], points, view)
    print(f"{what}: N {n} kmax {kmax} valid {int(valid.sum())} m<3 {int((~valid).sum())} small-gap share {share:.4f} "
          f"| max ||n|-1| {np.abs(length - 1).max() / 2.0 ** -23 if valid.any() else 0:.2f} ulp "
          f"| max (n'Cn-l0)/l2 {excess.max() if valid.any() else 0:.3e} of {2 * K * U:.3e} "
          f"| max cross/bound {ratio.max():.4f} | sign ties {int((tie_got & valid).sum())}")
    assert np.all(np.abs(length - 1.0) <= 4 * 2.0 ** -23), f"{what}: unit length"
    assert np.all(rq <= lam[valid, 0] + slack), f"{what}: Rayleigh quotient above l0 + 2 K u l2"
    if cap_gap_share:
        assert share <= GAP_SHARE_CAP, f"{what}: {share:.3f} of the valid rows have a gap below {GAP}"
    assert np.all(ratio <= 1.0), f"{what}: eigenvector outside K u / gap"
    # the sign obeys the rule on the returned vector itself (every valid row) ...
    decided = valid & ~tie_got
    assert np.all(s_got[decided] == 1.0), f"{what}: {int((s_got[decided] != 1).sum())} rows break the sign rule"
    # ... and equals the reference's where the direction is determined
    signed = ref['vec'] * s_ref[:, None]
    both = gap_rows & ~tie_got & ~tie_ref
    assert np.all((got[both] * signed[both]).sum(1) > 0), f"{what}: sign differs from the reference's"
    if curv is not None:
        assert curv.dtype == np.float32 and curv.shape == (n,)
        err = np.abs(curv.astype(np.float64) - ref['curv'])
        print(f"{what}: max curvature error {err.max() if n else 0:.3e} of {K * U:.3e}")
        assert np.all(err <= K * U), f"{what}: curvature"
        assert np.all(curv[~valid] == 0)
    ref.update(gap_rows=gap_rows, signed=signed, tie=tie_got | tie_ref, gap=gap, K=K)
    return ref


def punch_shadows(nbr: np.ndarray, n: int, seed: int, share: float = 0.3) -> np.ndarray:
    """A hand-made matrix: the columns of every row shuffled, then `share` of the entries replaced by shadows of every
    kind (N, N + 5, -1, INT_MIN, INT_MAX) -- shadows between valid entries, at any column."""
    rng = np.random.default_rng(seed)
    out = nbr.astype(np.int64).copy()
    out = np.take_along_axis(out, np.argsort(rng.random(out.shape), axis=1), axis=1)
    kinds = np.concatenate([SHADOWS, [n, n + 5]])
    hit = rng.random(out.shape) < share
    out[hit] = kinds[rng.integers(0, len(kinds), int(hit.sum()))]
    return out.astype(np.int32)


# ---- gather + rotate -------------------------------------------------------------------------------------------------
def gather_rotate(feats: np.ndarray, rows: np.ndarray, lens_out, rot: np.ndarray, cols) -> np.ndarray:
    """float64 restatement: one rounding per operation, ((R_k0 x + R_k1 y) + R_k2 z), then one to float32."""
    out = feats[rows].astype(np.float32).copy()
    if len(rows) == 0:
        return out
    R = np.repeat(np.asarray(rot, dtype=np.float32).astype(np.float64), np.asarray(lens_out, dtype=np.int64), axis=0)
    src = feats[rows].astype(np.float64)
    for s in cols:
        x, y, z = src[:, s], src[:, s + 1], src[:, s + 2]
        for k in range(3):
            out[:, s + k] = ((R[:, k, 0] * x + R[:, k, 1] * y) + R[:, k, 2] * z).astype(np.float32)
    return out
