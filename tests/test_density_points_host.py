"""gsgen_density_points (gsgen_amd/csrc/knn.hip) on the CPU SIMT emulator (oracle/emu): the density field at points of the caller's
own, with its gradient and a term-weighted colour.  The fp64 restatement itself against central differences; the value bit-equal
to gsgen_density_grid on a lattice at every list width; value, gradient and colour within counted rounding bounds of the fp64
restatement on the brute-force neighbour list (tests/density_points_cases.py); the colour's fallback; outputs and arguments."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import density_cases as DC
import density_points_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSGEN_EUNSUPPORTED, GSGEN_EINVAL, GSGEN_EWORKSPACE = -2, -3, -4
u32, vp, sz = C.c_uint32, C.c_void_p, C.c_size_t
KS_LIST = (1, 2, 3, 4, 8, 9, 17, 32)  # every list length the fp64 cases below search


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """knn.hip compiled with g++ on the emulator headers, with the flags of oracle/Makefile's `emu` rule (into tmp: nothing under
    oracle/ changes)"""
    out = tmp_path_factory.mktemp("density_points_emu") / "libknn_emu.so"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                           "-Wno-unknown-pragmas", "-DGSGEN_EMU_KNOBS=1", "-I", os.path.join(ROOT, "oracle", "emu"), "-x", "c++",
                           os.path.join(ROOT, "gsgen_amd", "csrc", "knn.hip"), "-o", str(out), "-lm"])
    lib = C.CDLL(str(out))
    lib.gsgen_density_grid_workspace_bytes.argtypes, lib.gsgen_density_grid_workspace_bytes.restype = [u32, u32], sz
    lib.gsgen_density_grid.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, u32, u32, u32, u32, u32, vp, vp, sz, vp]
    lib.gsgen_density_grid.restype = C.c_int
    lib.gsgen_density_points_workspace_bytes.argtypes, lib.gsgen_density_points_workspace_bytes.restype = [u32, u32], sz
    lib.gsgen_density_points.argtypes = [vp, vp, vp, vp, vp, u32, vp, u32, u32, u32, vp, vp, vp, vp, sz, vp]
    lib.gsgen_density_points.restype = C.c_int
    return lib


SENTINEL, PAST = np.float32(7.0), 5


def run_points(lib, g, pts, K, skip, want=("density", "grad", "rgb"), color=True, shift=5):
    """-> dict of the outputs asked for, each allocated PAST rows longer than Q and filled with a sentinel (checked untouched past Q);
    the workspace base is shifted off its alignment"""
    f = {k: np.ascontiguousarray(g[k], np.float32) for k in ("mean", "qvec", "scale", "opacity", "color")}
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    N, Q = f["mean"].shape[0], pts.shape[0]
    bufs = {"density": np.full(Q + PAST, SENTINEL), "grad": np.full((Q + PAST, 3), SENTINEL), "rgb": np.full((Q + PAST, 3), SENTINEL)}
    ptr = lambda k: bufs[k].ctypes.data if k in want else None  # noqa: E731
    ws = np.zeros(lib.gsgen_density_points_workspace_bytes(N, K) + shift, np.uint8)[shift:]
    rc = lib.gsgen_density_points(f["mean"].ctypes.data, f["qvec"].ctypes.data, f["scale"].ctypes.data, f["opacity"].ctypes.data,
                                  f["color"].ctypes.data if color else None, N, pts.ctypes.data, Q, K, skip, ptr("density"), ptr("grad"),
                                  ptr("rgb"), ws.ctypes.data, ws.size, None)
    assert rc == 0, rc
    for k, b in bufs.items():
        assert (b[Q:] == SENTINEL).all(), f"{k}: written past Q"
        if k not in want:
            assert (b == SENTINEL).all(), f"{k}: written though not asked for"
    return {k: bufs[k][:Q] for k in want}


def run_grid(lib, g, ax, ay, az, K, skip):
    mean, qvec, scale, opacity = (np.ascontiguousarray(g[k], np.float32) for k in ("mean", "qvec", "scale", "opacity"))
    ax, ay, az = (np.ascontiguousarray(a, np.float32) for a in (ax, ay, az))
    N = mean.shape[0]
    out = np.full((ax.size, ay.size, az.size), 7.0, np.float32)
    ws = np.zeros(lib.gsgen_density_grid_workspace_bytes(N, K), np.uint8)
    rc = lib.gsgen_density_grid(mean.ctypes.data, qvec.ctypes.data, scale.ctypes.data, opacity.ctypes.data, N, ax.ctypes.data,
                                ay.ctypes.data, az.ctypes.data, ax.size, ay.size, az.size, K, skip, out.ctypes.data, ws.ctypes.data,
                                ws.size, None)
    assert rc == 0, rc
    return out


def clouds():
    """the clouds of test_knn_query_host.clouds() (rebuilt here: same generator, same draws) that the point kernel is run on"""
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
    return {k: v.astype(np.float32) for k, v in out.items()}


def queries_for(g, seed, n=2000):
    """n queries in a fixed random order: jittered centres, exact copies of centres (d = 0), uniform draws in 1.1 x the bounding box,
    points 3 .. 100 x the core's radius away, and two non-finite rows (1 and 300: one in each of the first two workgroups).  Drawn
    with a surplus;
    a draw whose fp64 colour denominator falls into 1e-50 .. 1e-30 for any list length of KS_LIST is dropped
    (density_points_cases.gap_free), so which branch the colour takes is a property of the inputs."""
    rng = np.random.default_rng(seed)
    pts = g["mean"]
    fin = pts[np.isfinite(pts).all(1)].astype(np.float64)
    med = np.median(fin, axis=0)
    r = float(np.quantile(np.linalg.norm(fin - med, axis=1), 0.98))  # (the core's radius: far outliers do not set it)
    s = float(np.median(g["scale"]))
    jit = fin[rng.integers(0, fin.shape[0], 900)] + s * rng.normal(size=(900, 3)) * rng.uniform(0.1, 3.0, (900, 1))
    copies = fin[rng.integers(0, fin.shape[0], 200)]
    lo, hi = fin.min(0), fin.max(0)
    uni = (lo + hi) / 2 + (rng.uniform(size=(500, 3)) * 2 - 1) * (hi - lo) / 2 * 1.1
    d = rng.normal(size=(600, 3))
    far = med + d / np.linalg.norm(d, axis=1, keepdims=True) * r * np.exp(rng.uniform(np.log(3.0), np.log(100.0), (600, 1)))
    q = np.concatenate([jit, copies, uni, far]).astype(np.float32)
    q = q[rng.permutation(q.shape[0])]
    q = q[PC.gap_free(g, q, KS_LIST)]
    assert q.shape[0] >= n, q.shape
    q = q[:n].copy()
    q[1] = (np.nan, 0.0, 0.0)
    q[min(300, n - 1)] = (0.0, -np.inf, 1.0)
    return q


CLOUDS = clouds()
FIELDS = {name: PC.fields_for(p, 40 + n) for n, (name, p) in enumerate(sorted(CLOUDS.items()))}
_QUERIES, _BRUTE = {}, {}


def queries(name):
    if name not in _QUERIES:
        _QUERIES[name] = queries_for(FIELDS[name], 300 + sorted(CLOUDS).index(name))
    return _QUERIES[name]


def brute32(name):
    """the K = 32 brute-force lists of a cloud's queries, computed once (the first Ks columns are the Ks search)"""
    if name not in _BRUTE:
        _BRUTE[name] = DC.brute_query(CLOUDS[name], queries(name), 32)[1]
    return _BRUTE[name]


def test_field64_gradient_is_the_central_difference_of_density64():
    """the restatement itself, in NumPy alone: field64's value is density64's, and its gradient is the central difference of that
    value with the neighbour list held fixed.  Step h = 1e-5 x the smallest scale: the truncation error is of relative size
    (h |g|)^2 / 6 <= 1e-8 for |d| within 30 sigma, the fp64 cancellation 2^-53 / (h |g|): both far inside the 1e-6 asked for,
    measured against sum_k t_k (gbar_ka + 1 / s_min), the size of the terms that are summed."""
    g = FIELDS["clustered"]
    rng = np.random.default_rng(3)
    pts = (g["mean"][rng.integers(0, g["mean"].shape[0], 300)] + g["scale"].mean() * rng.normal(size=(300, 3))).astype(np.float32)
    K, skip = 5, 1
    _, idx = DC.brute_query(g["mean"], pts, K + skip)
    f = PC.field64(g["mean"], g["qvec"], g["scale"], g["opacity"], g["color"], pts, idx, K, skip)
    v64, vb = DC.density64(g["mean"], g["qvec"], g["scale"], g["opacity"], pts, DC.kept(idx, K, skip))
    np.testing.assert_allclose(f["value"], v64, rtol=1e-13)
    np.testing.assert_allclose(f["value_bound"], vb, rtol=1e-13)
    assert (f["value"] > 1e-3).sum() > 100
    smin = float(g["scale"].min())
    h = 1e-5 * smin
    fd = np.zeros((300, 3))
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        up = PC.field64(g["mean"], g["qvec"], g["scale"], g["opacity"], None, pts.astype(np.float64) + e, idx, K, skip)["value"]
        dn = PC.field64(g["mean"], g["qvec"], g["scale"], g["opacity"], None, pts.astype(np.float64) - e, idx, K, skip)["value"]
        fd[:, a] = (up - dn) / (2 * h)
    A = DC.sigma_inv64(g["qvec"], g["scale"])
    j = idx[:, skip:]
    d = pts.astype(np.float64)[:, None, :] - g["mean"].astype(np.float64)[j]
    gbar = np.einsum("pkij,pkj->pki", np.abs(A[j]), np.abs(d))
    size = (f["t"][:, skip:, None] * (gbar + 1.0 / smin)).sum(1)
    err = np.abs(fd - f["grad"])
    print(f"field64 grad vs central differences: worst err / size {float((err / size).max()):.3e}")
    assert (err <= 1e-6 * size).all()
    w = f["t"] / f["den"][:, None]  # the colour is the weighted mean over ALL Ks entries: inside the hull of their colours
    c = g["color"].astype(np.float64)[idx]
    np.testing.assert_allclose(f["rgb"], (w[..., None] * c).sum(1), rtol=1e-13)
    assert (f["rgb"] >= c.min(1) - 1e-15).all() and (f["rgb"] <= c.max(1) + 1e-15).all()


@pytest.mark.parametrize("K,skip", [(1, 0), (2, 0), (2, 1), (4, 1), (8, 1), (16, 1), (31, 1)])
def test_emulated_points_equal_the_lattice_bit_for_bit(emu, K, skip):
    """the golden fields on a 6 x 5 x 7 sub-lattice of their axis: density at lattice(ax, ay, az) is gsgen_density_grid's, bit for
    bit, at every list width L (1, 2, 4, 8, 16, 32)"""
    z = DC.load_golden()
    g = dict(mean=z["mean"], qvec=z["qvec"], scale=z["scale"], opacity=z["opacity"], color=np.zeros_like(z["mean"]))
    ax, ay, az = z["axis"][9:15], z["axis"][8:13], z["axis"][7:14]
    grid = run_grid(emu, g, ax, ay, az, K, skip).reshape(-1)
    out = run_points(emu, g, DC.lattice(ax, ay, az), K, skip)
    assert grid.shape == (210,) and (grid > 1e-6).sum() >= 20  # (not a comparison of zeros)
    np.testing.assert_array_equal(out["density"].view(np.uint32), grid.view(np.uint32))


@pytest.mark.parametrize("name", sorted(CLOUDS))
@pytest.mark.parametrize("K,skip,Q", [(1, 0, 2000), (3, 1, 2000), (8, 0, 2000), (8, 1, 2000), (16, 1, 2000), (31, 1, 2000),
                                       (3, 1, 1), (3, 1, 257), (2, 0, 257), (3, 0, 257)])
def test_emulated_points_against_fp64(emu, name, K, skip, Q):
    """value, gradient and colour on the brute-force list (the kernel's own formula and tie rule: no query is ambiguous) within the
    counted bounds of density_points_cases; the colour's fallback rows bit-equal to the nearest centre's colour; both branches of
    the colour are taken"""
    assert K + skip in KS_LIST
    g, q = FIELDS[name], queries(name)[:Q]
    idx = np.ascontiguousarray(brute32(name)[:Q, :K + skip])
    out = run_points(emu, g, q, K, skip)
    low = PC.check_against_fp64(name, g, q, idx, K, skip, out["density"], out["grad"], out["rgb"])
    if Q == 2000:
        assert 400 <= low <= 1100, low
        assert (np.abs(out["grad"]).max(1) > 1e-3).sum() >= 300


def test_emulated_points_with_zero_opacity_copy_the_nearest_colour(emu):
    """opacity == 0 everywhere: every denominator is 0, the same branch as a query far from everything"""
    name = "duplicates"
    g = dict(FIELDS[name], opacity=np.zeros_like(FIELDS[name]["opacity"]))
    q = queries(name)[:300]
    out = run_points(emu, g, q, 3, 1)
    idx0 = brute32(name)[:300, 0]
    want = np.where((idx0 >= 0)[:, None], g["color"][np.where(idx0 >= 0, idx0, 0)], np.float32(0))
    assert (idx0 < 0).sum() == 1  # (query 1 is non-finite)
    np.testing.assert_array_equal(out["rgb"].view(np.uint32), want.view(np.uint32))
    assert (out["density"] == 0).all() and (out["grad"] == 0).all()


def test_emulated_points_null_outputs_leave_the_others_unchanged(emu):
    g, q = FIELDS["outliers"], queries("outliers")[:300]
    full = run_points(emu, g, q, 3, 1)
    names = ("density", "grad", "rgb")
    for n in (1, 2):
        for want in itertools.combinations(names, n):
            part = run_points(emu, g, q, 3, 1, want=want, color="rgb" in want)
            for k in want:
                assert part[k].tobytes() == full[k].tobytes(), (want, k)
    assert run_points(emu, g, q, 3, 1, want=()) == {}  # nothing asked for: success, nothing written
    with_color = run_points(emu, g, q, 3, 1, want=("density", "grad"), color=True)  # (a colour table without rgb: ignored)
    assert with_color["grad"].tobytes() == full["grad"].tobytes()
    for shift in (0, 1, 64):  # the base of the workspace: any alignment
        again = run_points(emu, g, q, 3, 1, shift=shift)
        assert all(again[k].tobytes() == full[k].tobytes() for k in names)


def test_emulated_points_argument_checks_and_edge_sizes(emu):
    lib = emu
    mean = np.zeros((4, 3), np.float32)
    q4, s3, o1, col = np.ones((4, 4), np.float32), np.ones((4, 3), np.float32), np.ones(4, np.float32), np.ones((4, 3), np.float32)
    col[:, 1] = 0.25
    pts = np.zeros((6, 3), np.float32)
    den, grad, rgb = np.full(6, 7.0, np.float32), np.full((6, 3), 7.0, np.float32), np.full((6, 3), 7.0, np.float32)
    ws = np.zeros(1 << 16, np.uint8)

    def call(N, Q, K, skip, wsb=ws.size, m=mean.ctypes.data, c=col.ctypes.data, r=rgb.ctypes.data, p=pts.ctypes.data):
        return lib.gsgen_density_points(m, q4.ctypes.data, s3.ctypes.data, o1.ctypes.data, c, N, p, Q, K, skip, den.ctypes.data,
                                        grad.ctypes.data, r, ws.ctypes.data, wsb, None)
    assert call(4, 6, 0, 1) == GSGEN_EUNSUPPORTED and call(4, 6, 32, 1) == GSGEN_EUNSUPPORTED and call(4, 6, 33, 0) == GSGEN_EUNSUPPORTED
    assert call(4, 6, 4, 1) == GSGEN_EINVAL and call(0, 6, 1, 0) == GSGEN_EINVAL and call(4, 6, 2, 2) == GSGEN_EINVAL  # Ks > N, ...
    assert call(4, 6, 2, 1, c=None) == GSGEN_EINVAL  # rgb without color
    assert call(4, 6, 2, 1, m=None) == GSGEN_EINVAL and call(4, 6, 2, 1, p=None) == GSGEN_EINVAL
    assert call(4, 6, 2, 1, wsb=16) == GSGEN_EWORKSPACE
    assert lib.gsgen_density_grid_workspace_bytes(4, 3) < lib.gsgen_density_points_workspace_bytes(4, 3) <= ws.size  # (+ the gradient's records)
    assert call(4, 6, 2, 1, wsb=lib.gsgen_density_grid_workspace_bytes(4, 2)) == GSGEN_EWORKSPACE  # (the lattice's size is too small)
    assert lib.gsgen_density_points_workspace_bytes(0, 3) == 0 and lib.gsgen_density_points_workspace_bytes(10, 33) == 0
    assert (den == 7.0).all() and (grad == 7.0).all() and (rgb == 7.0).all()  # no failed call wrote
    assert call(4, 0, 2, 1) == 0 and (den == 7.0).all() and (grad == 7.0).all() and (rgb == 7.0).all()  # Q == 0: nothing enqueued
    assert call(4, 6, 2, 1, c=None, r=None) == 0 and np.allclose(den, 2.0) and (grad == 0).all() and (rgb == 7.0).all()
    # N == Ks: four unit Gaussians at the query, the nearest dropped by the field and kept by the colour
    assert call(4, 6, 3, 1) == 0 and np.allclose(den, 3.0) and (grad == 0).all()
    assert np.allclose(rgb, [1.0, 0.25, 1.0], rtol=1e-6)
    # N = 1, K = 1: one Gaussian of scale 1 at the origin, a query at (1, 0, 0): exp(-1/2), gradient -exp(-1/2) x
    pts[:, 0] = 1.0
    assert call(1, 6, 1, 0) == 0
    e = np.exp(-0.5)
    assert np.allclose(den, e, rtol=1e-6) and np.allclose(grad, [-e, 0.0, 0.0], rtol=1e-6, atol=1e-7)
    assert np.array_equal(rgb.view(np.uint32), np.broadcast_to(col[0], (6, 3)).copy().view(np.uint32))  # (one colour: num / den = c)
