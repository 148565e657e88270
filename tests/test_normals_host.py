"""gsgen_point_normals (gsgen_amd/csrc/knn.hip) on the CPU SIMT emulator (oracle/emu): normals, curvatures and frames against the
fp64 restatement of tests/normals_cases.py on the brute-force neighbour list, at every list width (4, 8, 16, 32 and the 64 that
only this kernel has), with and without disambiguation; degenerate clouds; output subsets; arguments; and the restatement's own
sanity on an exact plane and an exact sphere."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import normals_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSGEN_EUNSUPPORTED, GSGEN_EINVAL, GSGEN_EWORKSPACE = -2, -3, -4
u32, vp, sz = C.c_uint32, C.c_void_p, C.c_size_t
SHAPES = {"normals": (3,), "curvature": (3,), "frames": (3, 3)}
SENTINEL, PAST = np.float32(7.0), 5


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """knn.hip compiled with g++ on the emulator headers, with the flags of oracle/Makefile's `emu` rule (into tmp: nothing under
    oracle/ changes)"""
    out = tmp_path_factory.mktemp("normals_emu") / "libknn_emu.so"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                           "-Wno-unknown-pragmas", "-DGSGEN_EMU_KNOBS=1", "-I", os.path.join(ROOT, "oracle", "emu"), "-x", "c++",
                           os.path.join(ROOT, "gsgen_amd", "csrc", "knn.hip"), "-o", str(out), "-lm"])
    lib = C.CDLL(str(out))
    lib.gsgen_point_normals_workspace_bytes.argtypes, lib.gsgen_point_normals_workspace_bytes.restype = [u32, u32], sz
    lib.gsgen_point_normals.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp, sz, vp]
    lib.gsgen_point_normals.restype = C.c_int
    lib.gsgen_knn_workspace_bytes.argtypes, lib.gsgen_knn_workspace_bytes.restype = [u32, u32], sz
    lib.gsgen_knn.argtypes = [vp, u32, u32, vp, vp, vp, sz, vp]
    lib.gsgen_knn.restype = C.c_int
    return lib


def run(lib, pts, K, disambiguate=True, want=tuple(SHAPES), shift=5):
    """-> dict of the outputs asked for; every buffer is PAST rows longer than N and filled with a sentinel (checked untouched past
    N, and everywhere in a buffer not asked for); the workspace base is shifted off its alignment"""
    pts = np.ascontiguousarray(pts, np.float32)
    N = pts.shape[0]
    bufs = {k: np.full((N + PAST,) + s, SENTINEL) for k, s in SHAPES.items()}
    ptr = lambda k: bufs[k].ctypes.data if k in want else None  # noqa: E731
    ws = np.zeros(lib.gsgen_point_normals_workspace_bytes(N, K) + shift, np.uint8)[shift:]
    rc = lib.gsgen_point_normals(pts.ctypes.data, N, K, int(disambiguate), ptr("normals"), ptr("curvature"), ptr("frames"),
                                 ws.ctypes.data, ws.size, None)
    assert rc == 0, rc
    for k, b in bufs.items():
        assert (b[N:] == SENTINEL).all(), f"{k}: written past N"
        if k not in want:
            assert (b == SENTINEL).all(), f"{k}: written though not asked for"
    return {k: bufs[k][:N] for k in want}


DESIGNATED = NC.designated(2000)
DEGENERATE = NC.degenerate(1500)


@pytest.mark.parametrize("K", NC.K_LIST)
@pytest.mark.parametrize("name", sorted(DESIGNATED))
def test_emulated_normals_against_fp64(emu, name, K):
    """the designated clouds: curvature, n and z within the counted bounds of normals_cases, the disambiguated sign where the fp64
    decision is robust, the caps on what is left out; disambiguation off: the same frame up to sign, the kernel's own sign rule"""
    pts = DESIGNATED[name]
    idx = NC.brute_list(name, pts, K)
    on = run(emu, pts, K, True)
    NC.check_against_fp64(name, pts, idx, K, True, on, is_designated=True)
    off = run(emu, pts, K, False)
    NC.check_against_fp64(name, pts, idx, K, False, off, is_designated=True)
    assert on["curvature"].tobytes() == off["curvature"].tobytes()
    assert np.array_equal(np.abs(on["normals"]), np.abs(off["normals"]))  # (the same direction, bit for bit, up to sign)


def test_the_neighbour_list_is_gsgen_knn_s(emu):
    """the brute force the restatement runs on is the list gsgen_knn returns (K = 32: the widest it has)"""
    pts = np.ascontiguousarray(DESIGNATED["outliers"])
    N, K = pts.shape[0], 32
    d2, idx = np.zeros((N, K), np.float32), np.zeros((N, K), np.int32)
    ws = np.zeros(emu.gsgen_knn_workspace_bytes(N, K), np.uint8)
    assert emu.gsgen_knn(pts.ctypes.data, N, K, d2.ctypes.data, idx.ctypes.data, ws.ctypes.data, ws.size, None) == 0
    np.testing.assert_array_equal(idx, NC.brute_list("outliers", pts, K))


@pytest.mark.parametrize("K", NC.K_LIST)
@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_emulated_normals_on_degenerate_clouds(emu, name, K):
    """duplicates, a line, the plane z = 0, one position, NaN / Inf rows: finite, unit length, orthonormal, zero rows exactly where
    a point is not finite or short of K finite neighbours, the same bits on a second run.  Not held to the bound, except that the
    plane's normal is +-(0, 0, 1) wherever its in-plane gap allows (and +(0, 0, 1) with disambiguation: every projection is 0)."""
    pts = DEGENERATE[name]
    idx = NC.brute_list("deg_" + name, pts, K)
    for dis in (True, False):
        out = run(emu, pts, K, dis)
        valid = NC.check_structure(name, pts, idx, K, out)
        again = run(emu, pts, K, dis, shift=0)
        assert all(out[k].tobytes() == again[k].tobytes() for k in out)
        if name == "nan_rows":
            assert 0 < (~valid).sum() < 40
        else:
            assert valid.all()
        if name == "coincident":
            assert (out["curvature"] == 0).all()
        if name == "plane":
            r = NC.frames64(pts, idx, K, dis)
            g = r["lam"][:, 1] / np.maximum(r["lam"][:, 2], 1e-300)  # (lambda0 = 0: the plane is exact)
            use = g >= NC.G_MIN
            err = NC.cross_norm(np.broadcast_to([0.0, 0.0, 1.0], (len(pts), 3)), out["normals"].astype(np.float64))
            assert (err[use] <= NC.c_dir(K, r["kappa"][use]) * NC.EPS / g[use]).all() and use.mean() > 0.9
            assert (out["normals"][use, 2] > 0).all()
            assert (np.abs(out["curvature"][:, 0]) <= NC.c_lambda(K, r["kappa"]) * NC.EPS * r["l2"]).all()


@pytest.mark.parametrize("K", (3, 8, 32, 33, 64))
def test_emulated_normals_n_equals_k_plus_1(emu, K):
    """the smallest cloud the call accepts: every neighbourhood is the whole cloud but one point"""
    pts = NC.n_eq_k_plus_1(K)
    idx = NC.brute_list(f"nk{K}", pts, K)
    for dis in (True, False):
        NC.check_against_fp64(f"N=K+1={K + 1}", pts, idx, K, dis, run(emu, pts, K, dis))


def test_emulated_normals_output_subsets_and_workspace_alignment(emu):
    pts = DESIGNATED["gauss"][:700]
    for K in (9, 50):
        full = run(emu, pts, K)
        for n in (1, 2):
            for want in itertools.combinations(SHAPES, n):
                part = run(emu, pts, K, want=want)
                for k in want:
                    assert part[k].tobytes() == full[k].tobytes(), (K, want, k)
        for shift in (0, 1, 64):
            again = run(emu, pts, K, shift=shift)
            assert all(again[k].tobytes() == full[k].tobytes() for k in SHAPES)


def test_emulated_normals_argument_checks(emu):
    lib = emu
    pts = np.random.default_rng(0).uniform(-1, 1, (80, 3)).astype(np.float32)
    out = {k: np.full((80,) + s, SENTINEL) for k, s in SHAPES.items()}
    ws = np.zeros(1 << 16, np.uint8)

    def call(N, K, p=pts.ctypes.data, n=out["normals"].ctypes.data, c=out["curvature"].ctypes.data, f=out["frames"].ctypes.data,
             w=ws.ctypes.data, wsb=ws.size):
        return lib.gsgen_point_normals(p, N, K, 1, n, c, f, w, wsb, None)
    size = lib.gsgen_point_normals_workspace_bytes
    assert [call(80, K) for K in (0, 1, 2, 65, 1000)] == [GSGEN_EUNSUPPORTED] * 5
    assert [size(80, K) for K in (0, 2, 65)] == [0, 0, 0] and size(0, 8) == 0
    assert 0 < size(80, 3) <= ws.size and 0 < size(80, 64) <= ws.size
    assert call(0, 8) == GSGEN_EINVAL and call(8, 8) == GSGEN_EINVAL and call(7, 8) == GSGEN_EINVAL  # K >= N
    assert call(0x80000000, 8) == GSGEN_EINVAL
    assert call(80, 8, p=None) == GSGEN_EINVAL and call(80, 8, w=None) == GSGEN_EINVAL
    assert call(80, 8, n=None, c=None, f=None) == GSGEN_EINVAL
    assert call(80, 8, wsb=16) == GSGEN_EWORKSPACE and call(80, 8, wsb=size(80, 8) - 1) == GSGEN_EWORKSPACE
    assert all((b == SENTINEL).all() for b in out.values())  # no failed call wrote
    assert call(9, 8) == 0 and (out["normals"][:9] != SENTINEL).all() and (out["normals"][9:] == SENTINEL).all()
    assert call(80, 64, wsb=size(80, 64)) == 0


def test_fp64_restatement_on_an_exact_plane_and_an_exact_sphere():
    """the restatement itself, in NumPy alone.  A tilted plane through points that are exact in fp32 products of small integers:
    the normal is the plane's, to 1e-12, lambda0 = 0 to 1e-12 lambda2, with and without disambiguation.  A unit sphere (fp32
    points, 2^-24 off it): the normal of a neighbourhood of chord radius r is the radial direction within 2 r -- the centroid is
    within r of the point, and the fitted plane tilts against the tangent plane there by the cap's heights (r^2 / 2 at most) over
    its spread, at most r more when the neighbourhood is lopsided; the median is far inside."""
    rng = np.random.default_rng(2)
    ab = rng.integers(-512, 513, (1200, 2)).astype(np.float64) / 256.0
    e1, e2 = np.array([1.0, 0.0, 0.5]), np.array([0.0, 1.0, -0.25])  # z = x / 2 - y / 4: exact in fp32
    pts = (ab[:, :1] * e1 + ab[:, 1:] * e2).astype(np.float32)
    assert np.array_equal(pts.astype(np.float64), ab[:, :1] * e1 + ab[:, 1:] * e2)
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm)
    for K in (4, 30, 50):
        idx = NC.brute_list("exact_plane", pts, K)
        for dis in (True, False):
            r = NC.frames64(pts, idx, K, dis)
            ok = r["g_n"] > 1e-3
            assert ok.mean() > 0.9
            assert (NC.cross_norm(np.broadcast_to(nrm, r["n"].shape), r["n"])[ok] < 1e-12).all()
            assert (np.abs(r["lam"][:, 0]) <= 1e-12 * r["lam"][:, 2]).all()
            if not dis:
                assert (r["n"][ok] @ nrm > 0).all() == (not NC.first_negative(nrm))
    sph = NC.shell(2000, 3, noise=0.0)
    rad = sph.astype(np.float64) / np.linalg.norm(sph.astype(np.float64), axis=1, keepdims=True)
    for K in (8, 30):
        r = NC.frames64(sph, NC.brute_list("exact_sphere", sph, K), K, True)
        err = NC.cross_norm(rad, r["n"])
        assert (err <= 2 * r["dmax"]).all() and np.median(err) < 0.25 * np.median(r["dmax"])
        assert np.median(r["g_n"]) > 0.2  # (a sphere's neighbourhood is a cap: thin against its width)
