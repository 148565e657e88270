"""Shared restatements for the tests of gsgen_density_points (gsgen_amd/csrc/knn.hip: the density field at points of the caller's
own, with its gradient and a term-weighted colour): tests/test_density_points_host.py on the CPU emulator,
tests/test_gpu_density_points.py and tests/test_gpu_mesh_attributes.py on the GPU.  field64 is the fp64 restatement on a given
neighbour list, with rounding bounds counted on the kernel's code in the manner of density_cases.C_OPS, NOT fitted to results."""
import numpy as np

import density_cases as DC

EPS = DC.EPS
TINY = 2.0 ** -126

# rho_k = 1/2 C_OPS eps Mbar_k + 4 eps is the relative error of a term t_k (density_cases: the quadratic form through the rotation,
# exp, the product with the opacity, one running add).
#
# The gradient, grad_a = sum_k -(t_k g_ka), g_ka = (A_a0 dx + A_a1 dy) + A_a2 dz, against gbar_ka = sum_j |A_aj| |d_j|.  The kernel
# takes the row's A from rec_g: k_density_prep evaluates the closed form in fp64 from the fp32 inputs and rounds each entry once.
#   an entry of A: its one rounding to fp32, 1.  The fp64 chain before it carries the lattice's count in units of 2^-53, at most
#   48 * 2^-53 sum_k |R_ak R_jk| w_k: below one eps of |A_aj| unless the three terms cancel to 2^-23 of their size; counted as 1. -> 2
#   d_j = q_j - mean_j: 1; the product A_aj d_j: 1; the two adds of the row, both on the path of its first term: 2.              -> 4
#   the product t_k g_ka: 1 (relative to |t_k g_ka| <= t_k gbar_ka).                                                              -> 1
C_G = 7
# (With the lattice's fp32 record in the row the count would be 48 + 4 + 1 = 53 under that record's own premise, "of the size of
# |A_ij| for generic rotations", and it does not hold: an off-diagonal entry that is the remainder of three cancelling terms
# carries 100 - 500 eps of its own size, and with one neighbour and d nearly along an axis that entry's product is the row.  The
# form missed by up to 1.49 x at K = 1; that is why the gradient has a record of its own.)
# The running sum over the K kept entries starts from an exact 0: K - 1 roundings, each at most eps times the sum of the
# magnitudes: (K - 1) eps sum_k t_k |g_ka|.  An underflowing product loses at most 2^-126 per entry.
#   |delta grad_a| <= sum_k t_k (rho_k |g_ka| + C_G eps gbar_ka) + (K - 1) eps sum_k t_k |g_ka| + 2^-126 K
#
# The colour, rgb_c = num_c / den, num_c = sum_k t_k c_k, den = sum_k t_k over the Ks entries, omega_k = t_k / den.  The errors of
# the t_k move the weighted mean by sum_k omega_k delta_k (c_k - rgb_c) / (1 + sum_k omega_k delta_k), |delta_k| <= rho_k: at most
# (1 + 2 max rho) sum_k omega_k rho_k |c_k - rgb_c| while max rho <= 1/4.  Roundings of the colour's own chain, in units of
# eps sum_k omega_k |c_k| (which is >= |rgb_c|): the product t_k c_k 1, the running sum of num Ks - 1, that of den Ks - 1, the
# division 1: 2 Ks.
def c_r(Ks):
    return 2 * Ks


def field64(mean, qvec, scale, opacity, color, pts, idx, K, skip):
    """The fp64 restatement at pts [Q,3] (fp32 values, or fp64 for finite differences) on the neighbour LIST idx [Q, K + skip]
    (-1: none; list order).  The field keeps columns skip .. skip + K - 1, the colour takes all of them.  -> dict:
    value [Q], value_bound [Q] (density_cases.density64's), grad [Q,3], grad_bound [Q,3], den [Q] (the colour's denominator),
    rgb [Q,3] (NaN where den == 0), rgb_bound [Q,3]"""
    Ks = K + skip
    assert idx.shape[1] == Ks
    A = DC.sigma_inv64(qvec, scale)
    ok = idx >= 0
    j = np.where(ok, idx, 0)
    d = np.asarray(pts, np.float64)[:, None, :] - np.asarray(mean, np.float32).astype(np.float64)[j]
    d = np.where(ok[..., None], d, 0.0)  # (a missing entry: no NaN from a NaN centre 0)
    Aj = A[j]
    m = np.einsum("pki,pkij,pkj->pk", d, Aj, d)
    mbar = np.einsum("pki,pkij,pkj->pk", np.abs(d), np.abs(Aj), np.abs(d))
    with np.errstate(under="ignore"):
        t = np.where(ok, np.asarray(opacity, np.float32).astype(np.float64)[j] * np.exp(-0.5 * m), 0.0)
    rho = 0.5 * DC.C_OPS * EPS * mbar + 4 * EPS
    g = np.einsum("pkij,pkj->pki", Aj, d)
    gbar = np.einsum("pkij,pkj->pki", np.abs(Aj), np.abs(d))
    kept = slice(skip, Ks)
    tk, gk = t[:, kept, None], g[:, kept]
    out = {"t": t, "value": t[:, kept].sum(1), "value_bound": (t[:, kept] * rho[:, kept]).sum(1) + TINY * K}
    with np.errstate(under="ignore"):
        out["grad"] = -(tk * gk).sum(1)
        mag = (tk * np.abs(gk)).sum(1)
        out["grad_bound"] = (tk * (rho[:, kept, None] * np.abs(gk) + C_G * EPS * gbar[:, kept])).sum(1) + (K - 1) * EPS * mag + TINY * K
        den = t.sum(1)
        out["den"] = den
        if color is not None:
            c = np.asarray(color, np.float32).astype(np.float64)[j]
            safe = np.where(den > 0, den, 1.0)
            w = t / safe[:, None]
            rgb = (w[..., None] * c).sum(1)
            rmax = np.where(ok, rho, 0.0).max(1)
            bound = ((1 + 2 * rmax)[:, None] * (w[..., None] * rho[..., None] * np.abs(c - rgb[:, None, :])).sum(1)
                     + c_r(Ks) * EPS * (w[..., None] * np.abs(c)).sum(1) + (TINY * Ks / safe)[:, None])
            out["rgb"] = np.where(den[:, None] > 0, rgb, np.nan)
            out["rgb_bound"] = bound
    return out


def fields_for(points, seed):
    """qvec, scale, opacity, color for a cloud of centres: scales of the order of the cloud's own spacing (0.5 .. 3 x the median
    distance to the third neighbour), so that queries near the cloud see several overlapping Gaussians"""
    rng = np.random.default_rng(seed)
    p = np.asarray(points, np.float32)
    fin = p[np.isfinite(p).all(1)]
    d, _ = DC.brute_query(fin, fin[:400], 4)
    s0 = float(np.median(np.sqrt(d[:, 3].astype(np.float64))))
    N = p.shape[0]
    return dict(mean=p, qvec=rng.normal(size=(N, 4)).astype(np.float32), scale=(s0 * rng.uniform(0.5, 3.0, (N, 3))).astype(np.float32),
                opacity=rng.uniform(0.05, 1.0, N).astype(np.float32), color=rng.uniform(0.0, 1.0, (N, 3)).astype(np.float32))


def gap_free(g, queries, ks_list, lo=1e-50, hi=1e-30, idx=None):
    """mask of the queries whose colour denominator, in fp64 on the brute-force list (idx [Q, max(ks_list)], computed here when not
    given), lies outside [lo, hi] for every list length of ks_list: whether such a query takes the colour's fallback is then a
    property of the inputs, not of fp32 rounding.  (The band is m / 2 in 69 .. 115: a thin shell around the cloud; a query
    generator drops what falls into it.)"""
    kmax = max(ks_list)
    if idx is None:
        _, idx = DC.brute_query(g["mean"], queries, kmax)
    assert idx.shape[1] == kmax
    q = np.asarray(queries, np.float32)
    fin = np.isfinite(q).all(1)
    t = field64(g["mean"], g["qvec"], g["scale"], g["opacity"], None, np.where(fin[:, None], q, 0), idx, kmax, 0)["t"]
    cum = np.cumsum(t, axis=1)
    good = np.ones(len(queries), bool)
    for ks in ks_list:
        den = cum[:, ks - 1]
        good &= (den < lo) | (den > hi)
    return good


def check_against_fp64(tag, g, queries, idx, K, skip, density, grad, rgb):
    """kernel outputs at `queries` against field64 on the list idx [Q, K + skip]: density within density64's bound, gradient and
    colour within their counted bounds; the colour's fallback (fp64 denominator < 1e-50) bit-equal to the colour of list entry 0;
    non-finite queries all zero.  The denominators must lie outside 1e-50 .. 1e-30 (asserted).  Prints the worst ratios with the
    worst query; returns the number of rows in the colour's fallback."""
    q = np.asarray(queries, np.float32)
    fin = np.isfinite(q).all(1)
    f = field64(g["mean"], g["qvec"], g["scale"], g["opacity"], g["color"], np.where(fin[:, None], q, 0).astype(np.float32),
                np.where(fin[:, None], idx, -1), K, skip)
    for name, arr in (("density", density), ("grad", grad), ("rgb", rgb)):
        assert (np.asarray(arr)[~fin] == 0).all(), (tag, name, "a non-finite query must write 0")
    v64, vb = DC.density64(g["mean"], g["qvec"], g["scale"], g["opacity"], q[fin], DC.kept(idx[fin], K, skip))
    np.testing.assert_allclose(f["value"][fin], v64, rtol=1e-12, atol=1e-300)  # (field64's value IS density64's)
    rows = np.nonzero(fin)[0]
    derr = np.abs(density.astype(np.float64) - f["value"])[fin]
    gerr = np.abs(grad.astype(np.float64) - f["grad"])[fin]
    gb = f["grad_bound"][fin]
    wd = int(np.argmax(derr / vb))
    wg = np.unravel_index(int(np.argmax(gerr / gb)), gerr.shape)
    den = f["den"]
    assert ((den[fin] < 1e-50) | (den[fin] > 1e-30)).all(), (tag, "a query's colour denominator lies in 1e-50 .. 1e-30")
    low = fin & (den < 1e-50)
    has = idx[:, 0] >= 0
    want = np.where((low & has)[:, None], g["color"][np.where(has, idx[:, 0], 0)], np.float32(0))
    assert np.array_equal(rgb[low].view(np.uint32), want[low].view(np.uint32)), (tag, "fallback colour is not list entry 0's")
    hi = fin & (den > 1e-30)
    cerr = np.abs(rgb.astype(np.float64) - np.where(hi[:, None], f["rgb"], 0.0))[hi]
    cb = f["rgb_bound"][hi]
    line = (f"{tag} K={K} skip={skip} Q={len(q)}: mass at {int((f['value'] > 1e-30).sum())}, fallback colour at {int(low.sum())}; worst "
            f"err/bound density {derr[wd] / vb[wd]:.3f}, grad {gerr[wg] / gb[wg]:.3f} (query {rows[wg[0]]} axis {wg[1]} err "
            f"{gerr[wg]:.3e} bound {gb[wg]:.3e})")
    if hi.any():
        wc = np.unravel_index(int(np.argmax(cerr / cb)), cerr.shape)
        line += f", rgb {cerr[wc] / cb[wc]:.3f} (err {cerr[wc]:.3e})"
    print(line)
    assert (derr <= vb).all(), (tag, "density", rows[wd], derr[wd], vb[wd])
    assert (gerr <= gb).all(), (tag, "grad", f"{int((gerr > gb).sum())} components over", "worst query", int(rows[wg[0]]), "axis",
                                int(wg[1]), "err", float(gerr[wg]), "bound", float(gb[wg]))
    if hi.any():
        assert (cerr <= cb).all(), (tag, "rgb", np.nonzero(hi)[0][wc[0]], wc[1], cerr[wc], cb[wc])
    return int(low.sum())
