"""Shared restatements for the query-kNN and density-lattice tests (tests/test_knn_query_host.py on the CPU emulator,
tests/test_gpu_knn_query.py on the GPU) and for tests/golden/make_golden_density.py: the fp32 brute-force search in the kernel's
formula and tie rule, the fp64 density with its per-point rounding bound, and an fp32 NumPy walk through the kernel's own chain."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "density", "density_grid.npz")
EPS = 2.0 ** -24

# Operation count behind the bound |delta| <= sum_k t_k (1/2 C_OPS eps Mbar_k + 4 eps) + 2^-126 K  (t_k = o exp(-m_k / 2),
# m_k = d^T A d, Mbar_k = sum_ij |d_i| |A_ij| |d_j|, eps = 2^-24), counted on gsgen_amd/csrc/knn.hip, NOT fitted to its results:
#   an entry of R (k_density_prep): q / n carries 4 roundings (three adds of four squares under a square root -> 3, the division
#   1); a product 2 x y carries 4 + 4 + 1 = 9; a diagonal entry 1 - (tyy + tzz) sums two such products of total size <= 2 and
#   subtracts: 2 (9 + 1) + 1 = 21 units of eps for |R| <= 1; an off-diagonal entry txy - twz, total size <= 1: 9 + 1 = 10.  Take 21.
#   w_k = 1 / (s s): 2.
#   a term R_ik R_jk w_k of A_ij: 21 + 21 + 2 + two products 2 = 46; the two adds of the three terms: 2.            -> 48
#   the quadratic form: d_i and d_j one subtraction each 2, the two products a d_i d_j 2, then three adds on the longest path
#   (two inside diag / off, one joining them; the factor 2 is exact): 3.                                                 ->  7
# The R errors are absolute (in units of |R| <= 1), so the count holds relative to sum_k |R_ik R_jk| w_k, which is of the size of
# |A_ij| for the generic rotations of these tests.  The 4 eps per term cover exp (<= 1 ulp = 2 eps), the product with the opacity
# and the running sum.
C_OPS = 55


def brute_query(points, queries, K):
    """fp32, d = p_j - q, (dx*dx + dy*dy) + dz*dz; order (dist2, j); a non-finite point is nobody's neighbour, a non-finite query's
    row is (-1, +inf) -> (dist2 [Q,K] float32, idx [Q,K] int32)"""
    p, q = np.asarray(points, np.float32), np.asarray(queries, np.float32)
    N, Q = p.shape[0], q.shape[0]
    finp, finq = np.isfinite(p).all(1), np.isfinite(q).all(1)
    d = np.full((Q, K), np.inf, np.float32)
    idx = np.full((Q, K), -1, np.int32)
    top = np.iinfo(np.uint64).max
    for a in range(0, Q, 512):
        qq = q[a:a + 512]
        with np.errstate(invalid="ignore", over="ignore"):
            dx = p[None, :, 0] - qq[:, None, 0]
            dy = p[None, :, 1] - qq[:, None, 1]
            dz = p[None, :, 2] - qq[:, None, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(N, dtype=np.uint64)[None, :]
        key[:, ~finp] = top
        key[~finq[a:a + 512]] = top
        k = np.sort(key, axis=1)[:, :K]
        ok = k != top
        idx[a:a + 512][ok] = (k[ok] & np.uint64(0xFFFFFFFF)).astype(np.int32)
        d[a:a + 512][ok] = (k[ok] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return d, idx


def lattice(ax, ay, az):
    """[nx*ny*nz, 3] float32, x slowest (torch.meshgrid's "ij" order, the kernel's output order)"""
    g = np.stack(np.meshgrid(np.asarray(ax, np.float32), np.asarray(ay, np.float32), np.asarray(az, np.float32), indexing="ij"), -1)
    return np.ascontiguousarray(g.reshape(-1, 3))


def rotmat64(qvec):
    q = np.asarray(qvec, np.float32).astype(np.float64)
    q = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def sigma_inv64(qvec, scale):
    """R diag(1 / s^2) R^T in fp64 from the fp32 inputs (kornia 0.6.0 quaternion, w first)"""
    R = rotmat64(qvec)
    w = 1.0 / np.asarray(scale, np.float32).astype(np.float64) ** 2
    return np.einsum("nik,nk,njk->nij", R, w, R)


def density64(mean, qvec, scale, opacity, pts, idx):
    """the fp64 restatement on given neighbours idx [P,K] (-1: none) -> (value [P], bound [P]): the rounding bound of the header"""
    A = sigma_inv64(qvec, scale)
    ok = idx >= 0
    j = np.where(ok, idx, 0)
    d = np.asarray(pts, np.float32).astype(np.float64)[:, None, :] - np.asarray(mean, np.float32).astype(np.float64)[j]
    m = np.einsum("pki,pkij,pkj->pk", d, A[j], d)
    mbar = np.einsum("pki,pkij,pkj->pk", np.abs(d), np.abs(A[j]), np.abs(d))
    t = np.where(ok, np.asarray(opacity, np.float32).astype(np.float64)[j] * np.exp(-0.5 * m), 0.0)
    bound = (t * (0.5 * C_OPS * EPS * mbar + 4 * EPS)).sum(1) + 2.0 ** -126 * idx.shape[1]
    return t.sum(1), bound


def density32_chain(mean, qvec, scale, opacity, pts, idx):
    """the kernel's chain in NumPy fp32, rounded where the kernel rounds (every operation its own rounding, same order)"""
    f = np.float32
    q, s = np.asarray(qvec, f), np.asarray(scale, f)
    n = np.maximum(np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]), f(1e-12))
    w, x, y, z = (q[:, k] / n for k in range(4))
    tx, ty, tz = f(2) * x, f(2) * y, f(2) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = f(1)
    R = [[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, one - (txx + tyy)]]
    wk = [one / (s[:, k] * s[:, k]) for k in range(3)]
    A = {(a, b): (R[a][0] * R[b][0] * wk[0] + R[a][1] * R[b][1] * wk[1]) + R[a][2] * R[b][2] * wk[2] for a in range(3) for b in range(a, 3)}
    ok = idx >= 0
    j = np.where(ok, idx, 0)
    p, mu = np.asarray(pts, f), np.asarray(mean, f)
    dx, dy, dz = (p[:, None, k] - mu[j, k] for k in range(3))
    diag = (A[0, 0][j] * dx * dx + A[1, 1][j] * dy * dy) + A[2, 2][j] * dz * dz
    off = (A[0, 1][j] * dx * dy + A[0, 2][j] * dx * dz) + A[1, 2][j] * dy * dz
    m = diag + f(2) * off
    with np.errstate(over="ignore", under="ignore"):
        t = np.where(ok, np.asarray(opacity, f)[j] * np.exp(f(-0.5) * m), f(0))
    out = np.zeros(p.shape[0], f)
    for k in range(idx.shape[1]):
        out = out + t[:, k]
    return out


def kept(idx, K, skip):
    """columns skip .. skip + K - 1 of a K + skip search"""
    return np.ascontiguousarray(idx[:, skip:skip + K])


def load_golden():
    return dict(np.load(GOLDEN))


def check_golden_grid(grid, z):
    """a kernel grid [reso^3] on the fixture's lattice against the fixture: per-point bound, and max-abs / RMS error against the fp64
    grid at most twice the reference's own (two fp32 evaluation orders of one formula) -> (max_abs, rms) of the kernel"""
    g64 = z["grid64"].reshape(-1)
    err = np.abs(np.asarray(grid, np.float64).reshape(-1) - g64)
    worst = int(np.argmax(err - z["bound"].reshape(-1)))
    mx, rms = float(err.max()), float(np.sqrt((err ** 2).mean()))
    print(f"density golden: kernel max|err| {mx:.3e} rms {rms:.3e}; reference max|err| {float(z['ref_max_abs']):.3e} "
          f"rms {float(z['ref_rms']):.3e}; worst point err {err[worst]:.3e} bound {z['bound'].reshape(-1)[worst]:.3e}")
    assert (err <= z["bound"].reshape(-1)).all(), (worst, err[worst], z["bound"].reshape(-1)[worst])
    assert float(z["ref_max_abs"]) > 0 and float(z["ref_rms"]) > 0
    assert mx <= 2 * float(z["ref_max_abs"]) and rms <= 2 * float(z["ref_rms"]), (mx, rms)
    return mx, rms
