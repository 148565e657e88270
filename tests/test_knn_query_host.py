"""gsgen_knn_query and gsgen_density_grid (gsgen_amd/csrc/knn.hip) on the CPU SIMT emulator (oracle/emu): the query search against
an fp32 NumPy brute force -- identical dist2 bits and identical indices -- for queries near, between, far outside and on top of the
points; the fused density lattice against its own neighbour set and an fp64 restatement with a per-point rounding bound, and against
the reference's own grid (tests/golden/density)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import density_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSGEN_EUNSUPPORTED, GSGEN_EINVAL, GSGEN_EWORKSPACE = -2, -3, -4
u32, vp, sz = C.c_uint32, C.c_void_p, C.c_size_t


@pytest.fixture(scope="module")
def knn_emu(tmp_path_factory):
    """knn.hip compiled with g++ on the emulator headers, with the flags of oracle/Makefile's `emu` rule (into tmp: nothing under
    oracle/ changes)"""
    out = tmp_path_factory.mktemp("knn_query_emu") / "libknn_emu.so"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                           "-Wno-unknown-pragmas", "-DGSGEN_EMU_KNOBS=1", "-I", os.path.join(ROOT, "oracle", "emu"), "-x", "c++",
                           os.path.join(ROOT, "gsgen_amd", "csrc", "knn.hip"), "-o", str(out), "-lm"])
    lib = C.CDLL(str(out))
    lib.gsgen_knn_workspace_bytes.argtypes, lib.gsgen_knn_workspace_bytes.restype = [u32, u32], sz
    lib.gsgen_knn.argtypes, lib.gsgen_knn.restype = [vp, u32, u32, vp, vp, vp, sz, vp], C.c_int
    lib.gsgen_knn_query_workspace_bytes.argtypes, lib.gsgen_knn_query_workspace_bytes.restype = [u32, u32, u32], sz
    lib.gsgen_knn_query.argtypes, lib.gsgen_knn_query.restype = [vp, u32, vp, u32, u32, vp, vp, vp, sz, vp], C.c_int
    lib.gsgen_density_grid_workspace_bytes.argtypes, lib.gsgen_density_grid_workspace_bytes.restype = [u32, u32], sz
    lib.gsgen_density_grid.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, u32, u32, u32, u32, u32, vp, vp, sz, vp]
    lib.gsgen_density_grid.restype = C.c_int
    return lib


def run_query(lib, pts, qs, K):
    pts, qs = np.ascontiguousarray(pts, np.float32), np.ascontiguousarray(qs, np.float32)
    N, Q = pts.shape[0], qs.shape[0]
    d = np.full((Q, K), 7.0, np.float32)
    i = np.full((Q, K), -7, np.int32)
    ws = np.zeros(lib.gsgen_knn_query_workspace_bytes(N, Q, K) + 3, np.uint8)[3:]  # (an unaligned base: the carve aligns it)
    rc = lib.gsgen_knn_query(pts.ctypes.data, N, qs.ctypes.data, Q, K, d.ctypes.data, i.ctypes.data, ws.ctypes.data, ws.size, None)
    assert rc == 0, rc
    return d, i


def run_self(lib, pts, K):
    pts = np.ascontiguousarray(pts, np.float32)
    N = pts.shape[0]
    d = np.full((N, K), 7.0, np.float32)
    i = np.full((N, K), -7, np.int32)
    ws = np.zeros(lib.gsgen_knn_workspace_bytes(N, K), np.uint8)
    assert lib.gsgen_knn(pts.ctypes.data, N, K, d.ctypes.data, i.ctypes.data, ws.ctypes.data, ws.size, None) == 0
    return d, i


def run_density(lib, g, ax, ay, az, K, skip):
    mean, qvec, scale, opacity = (np.ascontiguousarray(g[k], np.float32) for k in ("mean", "qvec", "scale", "opacity"))
    ax, ay, az = (np.ascontiguousarray(a, np.float32) for a in (ax, ay, az))
    N = mean.shape[0]
    out = np.full((ax.size, ay.size, az.size), 7.0, np.float32)
    ws = np.zeros(lib.gsgen_density_grid_workspace_bytes(N, K) + 5, np.uint8)[5:]
    rc = lib.gsgen_density_grid(mean.ctypes.data, qvec.ctypes.data, scale.ctypes.data, opacity.ctypes.data, N, ax.ctypes.data,
                                ay.ctypes.data, az.ctypes.data, ax.size, ay.size, az.size, K, skip, out.ctypes.data, ws.ctypes.data,
                                ws.size, None)
    assert rc == 0, rc
    return out


def clouds():
    """the clouds of test_knn_host.clouds() that stress the index (rebuilt here: same generator, same draws)"""
    rng = np.random.default_rng(11)
    out = {}
    rng.uniform(-1, 1, (1500, 3))  # ("uniform": drawn to keep the stream in step)
    centres = rng.normal(size=(12, 3))
    out["clustered"] = centres[rng.integers(0, 12, 1800)] + 0.01 * rng.normal(size=(1800, 3))
    base = rng.uniform(-1, 1, (600, 3))
    dup = np.concatenate([base, base[rng.integers(0, 600, 400)], base[:50]])  # exact duplicates, some three times
    out["duplicates"] = dup[rng.permutation(dup.shape[0])]
    rng.uniform(-1, 1, (1500, 3))  # ("planar")
    core = rng.normal(size=(1800, 3)) * 0.5
    far = rng.normal(size=(40, 3))
    out["outliers"] = np.concatenate([core, 100.0 * far / np.linalg.norm(far, axis=1, keepdims=True)])
    nanc = rng.uniform(-1, 1, (1200, 3))
    nanc[rng.integers(0, 1200, 30), rng.integers(0, 3, 30)] = np.nan
    nanc[5, 1] = np.inf
    nanc[17] = -np.inf
    out["nan_rows"] = nanc
    out["offset"] = rng.uniform(-1, 1, (800, 3)) * 1e-3 + np.array([1000.0, -2000.0, 500.0])  # far from the origin, fine spacing
    return {k: v.astype(np.float32) for k, v in out.items()}


def queries_for(pts, seed):
    """about 1 500 queries: jittered copies of points, uniform draws in the bounding box (mostly empty space in these clouds), points
    well outside the box of the cloud's core on every side, edge and corner (26 directions x 5 distances x 3), exact copies of cloud
    points, three non-finite queries"""
    rng = np.random.default_rng(seed)
    fin = pts[np.isfinite(pts).all(1)].astype(np.float64)
    lo, hi = np.quantile(fin, 0.02, axis=0), np.quantile(fin, 0.98, axis=0)  # (the core: far outliers do not set the scale)
    ctr, ext = (lo + hi) / 2, float((hi - lo).max())
    jit = fin[rng.integers(0, fin.shape[0], 700)] + 1e-3 * ext * rng.normal(size=(700, 3))
    blo, bhi = fin.min(0), fin.max(0)
    inside = rng.uniform(blo, bhi, (400, 3))
    dirs = np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)], np.float64)
    outside = np.concatenate([ctr + dirs * ext * m * (1 + 0.1 * rng.uniform(size=(26, 3))) for m in (0.8, 1.5, 3.0, 10.0, 100.0) for _ in range(3)])
    copies = pts[rng.integers(0, pts.shape[0], 10)]
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [-np.inf, np.nan, 1]])
    q = np.concatenate([jit, inside, outside, copies, bad]).astype(np.float32)
    return q[rng.permutation(q.shape[0])]


CLOUDS = clouds()
QUERIES = {name: queries_for(p, 100 + n) for n, (name, p) in enumerate(sorted(CLOUDS.items()))}
_BRUTE = {}


def brute32(name):
    """the K = 32 brute force of a cloud's queries, computed once (its first K columns are the K search)"""
    if name not in _BRUTE:
        _BRUTE[name] = DC.brute_query(CLOUDS[name], QUERIES[name], 32)
    return _BRUTE[name]


def test_the_rebuilt_clouds_are_the_self_search_tests_clouds():
    assert sorted(CLOUDS) == ["clustered", "duplicates", "nan_rows", "offset", "outliers"]
    assert CLOUDS["outliers"].shape == (1840, 3) and np.abs(CLOUDS["outliers"][-40:]).max() > 50
    assert np.isnan(CLOUDS["nan_rows"]).any() and abs(CLOUDS["offset"][:, 1].mean() + 2000) < 1
    assert np.unique(CLOUDS["duplicates"], axis=0).shape[0] == 600
    for q in QUERIES.values():
        assert 1400 <= q.shape[0] <= 1600


@pytest.mark.parametrize("name", sorted(CLOUDS))
@pytest.mark.parametrize("K", [1, 2, 4, 8, 32])
def test_emulated_knn_query_is_the_brute_force_bit_for_bit(knn_emu, name, K):
    d, i = run_query(knn_emu, CLOUDS[name], QUERIES[name], K)
    bd, bi = brute32(name)
    np.testing.assert_array_equal(i, bi[:, :K])
    np.testing.assert_array_equal(d.view(np.uint32), np.ascontiguousarray(bd[:, :K]).view(np.uint32))
    bad = ~np.isfinite(QUERIES[name]).all(1)
    assert bad.sum() == 3 and (i[bad] == -1).all() and np.isinf(d[bad]).all()


def test_emulated_knn_query_ties_go_to_the_lower_index(knn_emu):
    pts = CLOUDS["duplicates"]
    _, inv, cnt = np.unique(pts, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    rows = np.nonzero(cnt[inv] >= 2)[0][:200]  # points that exist two or three times
    d, i = run_query(knn_emu, pts, pts[rows], 4)
    for r, row in enumerate(rows):
        same = np.nonzero(inv == inv[row])[0]  # ascending
        n = min(len(same), 4)
        assert i[r, :n].tolist() == same[:n].tolist() and (d[r, :n] == 0).all()
    small = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0], [5, 5, 5]], np.float32)
    d, i = run_query(knn_emu, small, np.array([[0, 0, 0], [0.5, 0, 0], [5, 5, 5]], np.float32), 4)
    assert i.tolist() == [[0, 2, 3, 1], [0, 1, 2, 3], [4, 1, 0, 2]] and d[1].tolist() == [0.25] * 4


def test_emulated_knn_query_pads_short_rows(knn_emu):
    pts = np.array([[0, 0, 0], [np.nan, 0, 0], [1, 1, 1], [0, np.inf, 0]], np.float32)
    d, i = run_query(knn_emu, pts, np.array([[0.1, 0, 0], [np.nan, 0, 0], [9, 9, 9]], np.float32), 3)
    assert i.tolist() == [[0, 2, -1], [-1, -1, -1], [2, 0, -1]]
    assert np.isinf(d[:, 2]).all() and np.isinf(d[1]).all()
    d, i = run_query(knn_emu, np.full((5, 3), np.nan, np.float32), np.zeros((2, 3), np.float32), 2)  # no finite point at all
    assert (i == -1).all() and np.isinf(d).all()


def test_emulated_knn_query_argument_checks(knn_emu):
    lib = knn_emu
    pts, qs = np.zeros((4, 3), np.float32), np.ones((6, 3), np.float32)
    d, i = np.full((6, 33), 7.0, np.float32), np.full((6, 33), -7, np.int32)
    ws = np.zeros(1 << 16, np.uint8)

    def call(N, Q, K, wsb=ws.size, p=pts.ctypes.data, q=qs.ctypes.data):
        return lib.gsgen_knn_query(p, N, q, Q, K, d.ctypes.data, i.ctypes.data, ws.ctypes.data, wsb, None)
    assert call(4, 6, 0) == GSGEN_EUNSUPPORTED and call(4, 6, 33) == GSGEN_EUNSUPPORTED
    assert call(4, 6, 5) == GSGEN_EINVAL  # K > n_points
    assert call(0, 6, 1) == GSGEN_EINVAL
    assert call(4, 6, 2, p=None) == GSGEN_EINVAL and call(4, 6, 2, q=None) == GSGEN_EINVAL
    assert call(4, 6, 2, wsb=16) == GSGEN_EWORKSPACE
    assert call(4, 0, 2) == 0 and (d == 7.0).all() and (i == -7).all()  # no query: success, nothing written
    assert call(4, 6, 4) == 0 and lib.gsgen_knn_query_workspace_bytes(4, 6, 4) <= ws.size
    assert lib.gsgen_knn_query_workspace_bytes(0, 6, 4) == 0 and lib.gsgen_knn_query_workspace_bytes(10, 6, 33) == 0
    mean = np.zeros((4, 3), np.float32)
    q4, s3, o1, ax, out = np.ones((4, 4), np.float32), np.ones((4, 3), np.float32), np.ones(4, np.float32), np.zeros(2, np.float32), np.full(8, 7.0, np.float32)

    def dens(N, n, K, skip, wsb=ws.size, m=mean.ctypes.data):
        return lib.gsgen_density_grid(m, q4.ctypes.data, s3.ctypes.data, o1.ctypes.data, N, ax.ctypes.data, ax.ctypes.data, ax.ctypes.data,
                                      n, n, n, K, skip, out.ctypes.data, ws.ctypes.data, wsb, None)
    assert dens(4, 2, 0, 1) == GSGEN_EUNSUPPORTED and dens(4, 2, 32, 1) == GSGEN_EUNSUPPORTED
    assert dens(4, 2, 4, 1) == GSGEN_EINVAL and dens(0, 2, 1, 0) == GSGEN_EINVAL and dens(4, 2, 2, 2) == GSGEN_EINVAL
    assert dens(4, 2, 2, 1, m=None) == GSGEN_EINVAL and dens(4, 2, 2, 1, wsb=16) == GSGEN_EWORKSPACE
    assert dens(4, 0, 2, 1) == 0 and (out == 7.0).all()
    assert dens(4, 2, 3, 1) == 0 and np.allclose(out, 3.0)  # four unit Gaussians at the lattice point: the nearest dropped


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_emulated_self_search_is_unchanged(knn_emu, name):
    """gsgen_knn after the index / query split: still the self brute force, bit for bit"""
    pts = CLOUDS[name]
    d, i = run_self(knn_emu, pts, 8)
    bd, bi = DC.brute_query(pts, pts, 8)
    np.testing.assert_array_equal(i, bi)
    np.testing.assert_array_equal(d.view(np.uint32), bd.view(np.uint32))


# ---- the density lattice ------------------------------------------------------------------------------------------------
def shell_gaussians():
    """about 1 200 Gaussians on a hollow shell and 20 far outliers; scales 0.005 .. 0.06, random rotations"""
    rng = np.random.default_rng(5)
    n, n_out = 1200, 20
    u = rng.normal(size=(n, 3))
    mean = u / np.linalg.norm(u, axis=1, keepdims=True) * (1.0 + 0.02 * rng.normal(size=(n, 1)))
    v = rng.normal(size=(n_out, 3))
    mean = np.concatenate([mean, v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(3.0, 4.0, (n_out, 1))])
    N = n + n_out
    return dict(mean=mean.astype(np.float32), qvec=rng.normal(size=(N, 4)).astype(np.float32),
                scale=rng.uniform(0.005, 0.06, (N, 3)).astype(np.float32), opacity=rng.uniform(0.05, 1.0, N).astype(np.float32))


SHELL = shell_gaussians()


def shell_axes(which):
    """9 x 6 x 21 (no dimension a multiple of the brick) at +-1.1 max|mean| ("full": the outliers set it), and the same lattice drawn
    over the shell alone ("core"), where most points have Gaussians within reach"""
    L = np.float32(1.1) * np.abs(SHELL["mean"]).max() if which == "full" else np.float32(1.15)
    return tuple(np.linspace(-L, L, n).astype(np.float32) for n in (9, 6, 21))


@pytest.mark.parametrize("which", ["full", "core"])
@pytest.mark.parametrize("K,skip", [(3, 0), (3, 1), (7, 0), (7, 1)])
def test_emulated_density_grid_against_its_neighbours_and_fp64(knn_emu, which, K, skip):
    """The fused lattice kernel: (1) its neighbour set is gsgen_knn_query's on the same lattice points (which is the brute force's):
    the output equals what those indices give; (2) every value lies within the rounding bound of the fp64 restatement
    |delta| <= sum_k t_k (1/2 c eps Mbar_k + 4 eps) + 2^-126 K with c = density_cases.C_OPS = 55 from the operation count written there
    (48 for an entry of Sigma^-1 through the rotation, 7 for the quadratic form); (3) the fp64 restatement rounded to fp32 at the
    kernel's own points of the chain stays inside the same bound, so the bound is one fp32 arithmetic can meet."""
    g = SHELL
    ax, ay, az = shell_axes(which)
    pts = DC.lattice(ax, ay, az)
    out = run_density(knn_emu, g, ax, ay, az, K, skip).reshape(-1)
    _, qi = run_query(knn_emu, g["mean"], pts, K + skip)
    _, bi = DC.brute_query(g["mean"], pts, K + skip)
    np.testing.assert_array_equal(qi, bi)
    val, bound = DC.density64(g["mean"], g["qvec"], g["scale"], g["opacity"], pts, DC.kept(qi, K, skip))
    err = np.abs(out.astype(np.float64) - val)
    chain = DC.density32_chain(g["mean"], g["qvec"], g["scale"], g["opacity"], pts, DC.kept(qi, K, skip))
    cerr = np.abs(chain.astype(np.float64) - val)
    w = int(np.argmax(err / bound))
    print(f"{which} K={K} skip={skip}: nonzero {int((val > 1e-30).sum())}/{val.size} max value {val.max():.3e}; kernel worst err/bound "
          f"{err[w] / bound[w]:.3f} (err {err[w]:.3e}); fp32 chain worst err/bound {float((cerr / bound).max()):.3f}")
    assert (val > 1e-30).sum() >= (20 if which == "full" else 150)  # (the comparison is not one of zeros)
    assert (cerr <= bound).all()
    assert (err <= bound).all(), (w, err[w], bound[w])
    if skip:  # dropping the nearest is visible: the other choice of skip is far outside the bound at most points with mass
        other, _ = DC.density64(g["mean"], g["qvec"], g["scale"], g["opacity"], pts, DC.kept(qi, K, 0))
        assert (np.abs(out - other) > bound).sum() >= 10


def test_emulated_density_grid_matches_the_reference_golden(knn_emu):
    """tests/golden/density (the reference's get_density_val_grid_from_ckpt on the CPU, reso 24, K = 3): on the fixture's lattice the
    kernel's grid lies within the per-point bound of the fp64 grid, and its max-abs and RMS error against fp64 are at most twice the
    reference's own recorded figures (two fp32 evaluation orders of one formula)"""
    z = DC.load_golden()
    ax = z["axis"]
    assert float(z["L"]) == float(np.abs(z["mean"]).max()) * 1.1  # L as the port computes it (mean.abs().max().item() * 1.1)
    out = run_density(knn_emu, z, ax, ax, ax, int(z["K"]), 1)
    DC.check_golden_grid(out, z)
