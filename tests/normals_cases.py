"""Shared restatements for the tests of gsgen_point_normals (k_point_normals in gsgen_amd/csrc/knn.hip: point-cloud normals and
local frames fused with the self search): tests/test_normals_host.py on the CPU emulator, tests/test_gpu_normals.py on the GPU.
NumPy only.  frames64 is the fp64 restatement on a given neighbour list (the brute force of knn_cases.brute: the kernel's fp32
distance formula and (dist2, index) tie rule); the bounds are counted on the kernel's stated operation order, NOT fitted to results.

Notation: eps = 2^-23, u = eps / 2 (one rounding), lambda0 <= lambda1 <= lambda2 the fp64 eigenvalues of the covariance C,
kappa = (sum_k |d_k|^2 / K) / lambda2 >= 1 (how far the neighbourhood lies from the query, in units of its own spread; fp64, per
point: the differences are taken to the query, not to the centroid, so their size is not bounded by lambda2 with a constant).

The backward error E of the computed decomposition, |E|_2 <= C_E eps lambda2, is the sum of

(a) the covariance, per entry C_ab, in units of u lambda2 (with (1/K) sum_k |c_ka| |c_kb| <= sqrt(C_aa C_bb) <= lambda2):
      d_k = p_j - p_i, one rounding per component, in both factors of the product: 2 sqrt(kappa) (Cauchy-Schwarz);
      the mean m: its error shifts every c_k alike, and a covariance about a wrong centre m' is C + (m - m')(m - m')^T: second
        order, ((K + 1) u)^2 kappa, below 1e-8 of a unit for K <= 64: counted as 1 with the division below;
      c_k = d_k - m, one rounding per component, both factors: 2;   the product: 1;   the K-term sum from 0.0f: K - 1;
      the division by K: 1.                                                                   -> K + 3 + 2 sqrt(kappa)
    and |E|_2 <= |E|_F <= 3 max_ab |E_ab|:                                                    -> 3 (K + 3 + 2 sqrt(kappa)) u lambda2
    (the scaling by a power of two is exact)
(b) the solver: 6 sweeps x 3 rotations.  A rotation computes t with 6 roundings behind it (theta: 2, theta^2 + 1: at most 2 more,
    the root 1, the sum 1, the reciprocal 1 -- carried as relative errors) and (c, s) as the exact rotation of atan(t) within
    4 u (t t, + 1, root, reciprocal; s one more).  Applied from both sides, each new element c x -+ s y carries 4 + 3 u of
    |(x, y)|: 2 x 7 = 14 u |A|_F for the two sides; the shortcut a_pp -+ t a_pq and the entry set to zero hold for the exact root
    t only, which costs 6 u |t| (|a_pq| + |a_qq - a_pp| / 2) <= 2 u |A|_F more once |t| <= 1 is used ... counted as 16 u |A|_F per
    rotation, |A|_F <= sqrt(3) lambda2:                                                       -> 18 x 16 sqrt(3) u lambda2 < 500 u lambda2
Together C_E(K, kappa) = (3 (K + 3 + 2 sqrt(kappa)) + 500) / 2 in units of eps.

Eigenvalues (Weyl): |lambda - lambda_ref| <= |E|_2, plus the rounding of the result itself -> c_lambda = C_E + 1.

Directions (Davis-Kahan): sin(angle) <= |E|_2 / (gap - |E|_2) with the absolute gap of the eigenvalue to the rest of the spectrum;
on the rows the bound is applied to, g >= G_MIN = 1e-3, and C_E eps <= 400 eps < 5e-5, so 1 / (g - C_E eps) <= 1.05 / g.  The
eigenvector matrix itself is the product of the 18 computed rotations, each applied with 7 u of the column pair's length, and the
final normalisation adds 4 u: 130 u = 65 eps that do NOT grow with 1 / g (g <= 1 folds them into the same form):
    |n_ref x n| <= c eps / g,   c(K, kappa) = 1.05 C_E + 65,   g = (lambda1 - lambda0) / lambda2;   z: g = (lambda2 - lambda1) / lambda2.
For orientation: c is 350 to 420 on the clouds below, against measured worst ratios of the order of 1 eps / g -- the count is a
worst case over 18 rotations, most of which move nothing once the sweep has converged.  An unrefined closed-form (trigonometric)
solver loses about sqrt(eps) = 2900 eps of lambda2 where two eigenvalues are close, and fails this bound.
"""
import numpy as np

import knn_cases as KC

EPS = 2.0 ** -23
G_MIN = 1e-3
K_LIST = (3, 4, 8, 9, 16, 17, 30, 32, 33, 50, 64)
SKIP_CAP = 0.02      # share of a designated cloud's points with g < G_MIN, per K
UNSIGNED_CAP = 0.25  # share of a designated cloud's points compared only up to sign, per K >= 4
UNIT_TOL = 4 * EPS    # | |n| - 1 |: the normalisation's three roundings and the root
ORTHO_TOL = 128 * EPS  # |n . z|: 65 eps per column from the rotations (above), two columns


def c_e(K, kappa):
    return (3.0 * (K + 3.0 + 2.0 * np.sqrt(kappa)) + 500.0) / 2.0


def c_dir(K, kappa):
    return 1.05 * c_e(K, kappa) + 65.0


def c_lambda(K, kappa):
    return c_e(K, kappa) + 1.0


# ---- clouds ---------------------------------------------------------------------------------------------------------------
def shell(n, seed, noise=0.01):
    """a unit sphere shell with 1 % radial noise"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * (1.0 + noise * rng.normal(size=(n, 1)))).astype(np.float32)


def designated(n=2000):
    rng = np.random.default_rng(5)
    out = {"shell": shell(n, 1)}
    out["shell_far"] = (out["shell"].astype(np.float64) + np.array([300.0, -200.0, 100.0])).astype(np.float32)
    d = rng.normal(size=(n, 3))
    out["ball"] = (d / np.linalg.norm(d, axis=1, keepdims=True) * 0.8 * rng.uniform(size=(n, 1)) ** (1 / 3)).astype(np.float32)
    out["gauss"] = (0.8 * rng.normal(size=(n, 3))).astype(np.float32)
    core = 0.5 * rng.normal(size=(n, 3))
    far = rng.choice(n, n // 50, replace=False)  # 2 % of the points at 100 x the radius: the index's outlier bucket
    core[far] *= 100.0
    out["outliers"] = core.astype(np.float32)
    return out


def degenerate(n=1500):
    rng = np.random.default_rng(6)
    out = {}
    base = rng.uniform(-1, 1, (n // 2, 3))
    dup = np.concatenate([base, base[rng.integers(0, n // 2, n // 3)], base[:50], base[:50]])  # exact duplicates, some three times
    out["duplicates"] = dup[rng.permutation(dup.shape[0])]
    line = np.zeros((n, 3))
    line[:, 0] = rng.uniform(-2, 3, n)
    out["line"] = line @ np.array([[0.6, 0.0, 0.8], [0.0, 1.0, 0.0], [-0.8, 0.0, 0.6]])
    flat = rng.uniform(-1, 1, (n, 3))
    flat[:, 2] = 0.0
    out["plane"] = flat
    out["coincident"] = np.tile(np.array([[0.3, -1.7, 2.5]]), (200, 1))
    nanc = rng.uniform(-1, 1, (n, 3))
    nanc[rng.integers(0, n, 30), rng.integers(0, 3, 30)] = np.nan
    nanc[5, 1] = np.inf
    nanc[17] = -np.inf
    out["nan_rows"] = nanc
    return {k: v.astype(np.float32) for k, v in out.items()}


def n_eq_k_plus_1(K, seed=9):
    return np.random.default_rng(seed + K).uniform(-1, 1, (K + 1, 3)).astype(np.float32)


_BRUTE = {}


def brute_list(tag, pts, K):
    """idx [N, K] of the self search (knn_cases.brute), computed once per tag at the longest list and sliced"""
    if tag not in _BRUTE:
        _BRUTE[tag] = KC.brute(pts, min(64, pts.shape[0]))[1]
    return np.ascontiguousarray(_BRUTE[tag][:, :K])


# ---- the fp64 restatement ---------------------------------------------------------------------------------------------------
def first_negative(v):
    """[..., 3] -> mask: the first non-zero component is negative"""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return np.where(x != 0, x < 0, np.where(y != 0, y < 0, z < 0))


def frames64(pts, idx, K, disambiguate=True):
    """pts [N,3] float32 values, idx [N,K] (-1: none, list order) -> dict: valid [N] (a finite point with K neighbours),
    lam [N,3] ascending, n / y / z [N,3], g_n, g_z (relative gaps), kappa, dmax (max_k |d_k|), d [N,K,3], and with disambiguation
    proj_n / proj_z [N,K] of the FINAL directions.  Rows that are not valid hold zeros."""
    p = np.asarray(pts, np.float32).astype(np.float64)
    N = p.shape[0]
    valid = np.isfinite(p).all(1) & (idx >= 0).all(1)
    j = np.where(idx >= 0, idx, 0)
    d = np.where(valid[:, None, None], p[j] - np.where(valid[:, None], p, 0.0)[:, None, :], 0.0)
    d = np.nan_to_num(d, nan=0.0, posinf=0.0, neginf=0.0)
    m = d.sum(1) / K
    c = d - m[:, None, :]
    C = np.einsum("nka,nkb->nab", c, c) / K
    lam, V = np.linalg.eigh(C)
    n, y, z = V[:, :, 0].copy(), V[:, :, 1].copy(), V[:, :, 2].copy()
    l2 = np.where(lam[:, 2] > 0, lam[:, 2], 1.0)
    out = dict(valid=valid, lam=lam * valid[:, None], d=d, g_n=(lam[:, 1] - lam[:, 0]) / l2, g_z=(lam[:, 2] - lam[:, 1]) / l2,
               kappa=np.maximum((d * d).sum((1, 2)) / K / l2, 1.0), dmax=np.sqrt((d * d).sum(2).max(1)), l2=lam[:, 2] * valid)
    if disambiguate:
        for name, v in (("n", n), ("z", z)):
            proj = np.einsum("na,nka->nk", v, d)
            pos, neg, s = (proj > 0).sum(1), (proj < 0).sum(1), proj.sum(1)
            flip = np.where(2 * pos >= K, False, np.where(2 * neg >= K, True, np.where(s > 0, False, np.where(s < 0, True, first_negative(v)))))
            v *= np.where(flip, -1.0, 1.0)[:, None]
            out["proj_" + name] = proj * np.where(flip, -1.0, 1.0)[:, None]
        y = np.cross(n, z)
    else:
        for v in (n, y, z):
            v *= np.where(first_negative(v), -1.0, 1.0)[:, None]
    for name, v in (("n", n), ("y", y), ("z", z)):
        out[name] = v * valid[:, None]
    return out


def robust_sign(proj, d, K, angle_bound):
    """mask of the rows where the rule's decision for a direction cannot change under the errors of the computed direction: every
    neighbour with |proj_k| <= tol_k = |d_k| (angle_bound + 2 eps) (the direction's error times the lever, plus the dot product's
    three products, two sums and the rounding of d: 4 u |d_k|) may count either way; an exact d_k = 0 (the point itself, its exact
    duplicates) is 0 on both sides.  Robust: the final direction's sure count reaches K / 2 (proj is given for the FINAL direction,
    so only the positive side can); or neither side can reach K / 2 with every unsure neighbour added and the sum of projections
    stays positive by more than the sum of the tolerances and its own K roundings."""
    dn = np.sqrt((d * d).sum(2))
    tol = dn * (angle_bound[:, None] + 2 * EPS)
    zero = dn == 0
    sure_pos = ((proj > tol) & ~zero).sum(1)
    sure_neg = ((proj < -tol) & ~zero).sum(1)
    unsure = ((np.abs(proj) <= tol) & ~zero).sum(1)
    by_count = 2 * sure_pos >= K
    s = proj.sum(1)
    by_sum = (2 * (sure_pos + unsure) < K) & (2 * (sure_neg + unsure) < K) & (s > tol.sum(1) + K * EPS * np.abs(proj).sum(1))
    return by_count | by_sum


def cross_norm(a, b):
    return np.linalg.norm(np.cross(a, b), axis=1)


def check_structure(tag, pts, idx, K, out):
    """what holds on every cloud, degenerate ones included: zero rows exactly where a point is not finite or short of K finite
    neighbours; elsewhere everything finite, n / y / z of unit length and orthogonal, frames[:, :, 0] == normals bit for bit,
    curvature ascending.  -> valid mask"""
    p = np.asarray(pts, np.float32)
    valid = np.isfinite(p).all(1) & (idx >= 0).all(1)
    for name in ("normals", "curvature", "frames"):
        if name in out:
            a = out[name].reshape(len(p), -1)
            assert np.isfinite(a).all(), (tag, K, name, "not finite")
            assert (a[~valid] == 0).all(), (tag, K, name, "a degenerate row must be zero")
    if "frames" in out:
        f = out["frames"][valid].astype(np.float64)
        for c in range(3):
            assert (np.abs(np.linalg.norm(f[:, :, c], axis=1) - 1) <= (UNIT_TOL if c != 1 else ORTHO_TOL)).all(), (tag, K, "column", c, "length")
        for a, b in ((0, 1), (0, 2), (1, 2)):
            assert (np.abs((f[:, :, a] * f[:, :, b]).sum(1)) <= ORTHO_TOL).all(), (tag, K, "columns", a, b, "not orthogonal")
        if "normals" in out:
            assert np.array_equal(np.ascontiguousarray(out["frames"][:, :, 0]).view(np.uint32), out["normals"].view(np.uint32)), (tag, K)
    if "normals" in out:
        assert (np.abs(np.linalg.norm(out["normals"][valid].astype(np.float64), axis=1) - 1) <= UNIT_TOL).all(), (tag, K, "normal length")
    if "curvature" in out:
        cv = out["curvature"][valid]
        assert (np.diff(cv, axis=1) >= 0).all(), (tag, K, "curvature not ascending")
    return valid


def check_against_fp64(tag, pts, idx, K, disambiguate, out, is_designated=False):
    """the kernel's normals / curvature / frames (out: dict of arrays) against frames64 on the list idx.  Eigenvalues within
    c_lambda eps lambda2 on every valid row; n and z within c eps / g of the restatement's where g >= G_MIN: with their sign where
    the disambiguation's decision is robust (robust_sign; never at K = 3, where every projection of n vanishes), up to sign
    elsewhere and without disambiguation (then the kernel's own sign rule is checked on its output).  On a designated cloud the
    shares of the normals left out (g < G_MIN) and compared up to sign are capped.  Prints the worst ratios; -> dict of the shares."""
    valid = check_structure(tag, pts, idx, K, out)
    r = frames64(pts, idx, K, disambiguate)
    assert np.array_equal(valid, r["valid"])
    kap = r["kappa"]
    lam_err = np.abs(out["curvature"].astype(np.float64) - r["lam"]).max(1)
    lam_bound = c_lambda(K, kap) * EPS * r["l2"]
    w = int(np.argmax(np.where(valid, lam_err / np.maximum(lam_bound, 1e-300), 0)))
    line = f"{tag} K={K} dis={int(bool(disambiguate))} N={len(pts)}: lambda worst err/bound {lam_err[w] / max(lam_bound[w], 1e-300):.4f}"
    assert (lam_err[valid] <= lam_bound[valid]).all(), (tag, K, "curvature", w, lam_err[w], lam_bound[w])
    shares = {}
    f = out["frames"].astype(np.float64)
    for name, col, g in (("n", 0, r["g_n"]), ("z", 2, r["g_z"])):
        got, ref = f[:, :, col], r[name]
        use = valid & (g >= G_MIN)
        bound = c_dir(K, kap) * EPS / np.maximum(g, G_MIN)
        err = cross_norm(ref, got)
        ww = int(np.argmax(np.where(use, err / bound, 0)))
        skipped = float((valid & ~use).sum()) / max(int(valid.sum()), 1)
        line += f"; {name}: skipped {skipped:.4f}, worst err/bound {err[ww] / bound[ww]:.4f} (x eps/g: {err[ww] * g[ww] / EPS:.2f})"
        assert (err[use] <= bound[use]).all(), (tag, K, name, "direction", ww, err[ww], bound[ww], g[ww])
        dot = (ref * got).sum(1)
        if disambiguate and K >= 4:
            rob = use & robust_sign(r["proj_" + name], r["d"], K, bound)
            assert (dot[rob] > 0).all(), (tag, K, name, "sign", int(np.nonzero(rob & (dot <= 0))[0][0]))
            unsigned = float((use & ~rob).sum()) / max(int(use.sum()), 1)
        else:
            unsigned = 1.0
        if not disambiguate:
            assert not first_negative(got[valid]).any(), (tag, K, name, "sign rule without disambiguation")
        line += f", up to sign {unsigned:.4f}"
        shares[name] = (skipped, unsigned)
        if is_designated and name == "n":  # (the caps are the normal's; z lies in the tangent plane, where neighbours balance)
            assert skipped <= SKIP_CAP, (tag, K, name, "share with g < G_MIN", skipped)
            if disambiguate and K >= 4:
                assert unsigned <= UNSIGNED_CAP, (tag, K, name, "share compared up to sign", unsigned)
    if disambiguate:  # y = n x z
        y = np.cross(f[:, :, 0], f[:, :, 2])
        assert (np.abs(y - f[:, :, 1])[valid] <= 4 * EPS).all(), (tag, K, "y is not n x z")
    else:
        assert not first_negative(f[valid][:, :, 1]).any(), (tag, K, "y", "sign rule without disambiguation")
    print(line)
    return shares
