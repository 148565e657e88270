"""gsgen_amd/csrc/fps.hip on the CPU SIMT emulator (oracle/emu) against the fp32 NumPy reference of tests/fps_cases.py: the whole
index array, exactly, for the brute and the bucket-pruned kernel, on the clouds that stress ties, the grid and the pruning bounds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from fps_cases import CLOUDS, NAMES, fps_reference, reference, with_rgb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSGEN_EUNSUPPORTED, GSGEN_EINVAL = -2, -3
AUTO, BRUTE, BUCKET = 0, 1, 2
METHODS = {"brute": BRUTE, "bucket": BUCKET}


@pytest.fixture(scope="module")
def fps_emu(tmp_path_factory):
    """fps.hip compiled with g++ on the emulator headers, with the flags of oracle/Makefile's `emu` rule (into tmp: nothing under
    oracle/ changes)"""
    out = tmp_path_factory.mktemp("fps_emu") / "libfps_emu.so"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                           "-Wno-unknown-pragmas", "-DGSGEN_EMU_KNOBS=1", "-I", os.path.join(ROOT, "oracle", "emu"), "-x", "c++",
                           os.path.join(ROOT, "gsgen_amd", "csrc", "fps.hip"), "-o", str(out), "-lm"])
    lib = C.CDLL(str(out))
    lib.gsgen_fps_workspace_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    lib.gsgen_fps_workspace_bytes.restype = C.c_size_t
    lib.gsgen_fps.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                              C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    lib.gsgen_fps.restype = C.c_int
    lib.gsgen_fps_emu_visits.argtypes, lib.gsgen_fps_emu_visits.restype = [C.c_void_p, C.c_uint32], C.c_uint32
    lib.gsgen_fps_emu_constants.argtypes, lib.gsgen_fps_emu_constants.restype = [C.c_void_p], None
    return lib


def run_fps(lib, pts, K, starts, method, lengths=None, shared=False):
    """pts [L, D] with shared=True (every start samples it) or [B, L, D] -> idx int32 [B, K]"""
    pts = np.ascontiguousarray(pts, np.float32)
    starts = np.ascontiguousarray(starts, np.int32)
    B = starts.shape[0]
    L, D = pts.shape[-2:]
    stride = 0 if shared else L * D
    assert shared or pts.shape[0] == B
    idx = np.full((B, K), -7, np.int32)
    lens = None if lengths is None else np.ascontiguousarray(lengths, np.int32)
    nbytes = lib.gsgen_fps_workspace_bytes(L, D, B, K, method)
    assert nbytes > 0
    ws = np.zeros(nbytes + 3, np.uint8)[3:]  # (an unaligned base: the carve aligns it)
    rc = lib.gsgen_fps(pts.ctypes.data, L, D, stride, None if lens is None else lens.ctypes.data, starts.ctypes.data, B, K,
                       idx.ctypes.data, ws.ctypes.data, ws.size, method, None)
    assert rc == 0, rc
    return idx


@pytest.mark.parametrize("method", sorted(METHODS))
@pytest.mark.parametrize("name", NAMES)
def test_emulated_fps_is_the_reference_index_for_index(fps_emu, name, method):
    pts, s0 = CLOUDS[name]
    idx = run_fps(fps_emu, pts, 64, [s0], METHODS[method], shared=True)
    np.testing.assert_array_equal(idx[0], reference(name, 64))


@pytest.mark.parametrize("name", NAMES)
def test_emulated_fps_brute_with_six_coordinates(fps_emu, name):
    pts, s0 = with_rgb(name)
    idx = run_fps(fps_emu, pts, 32, [s0], BRUTE, shared=True)
    np.testing.assert_array_equal(idx[0], reference(name, 32, 6))


@pytest.mark.parametrize("method", sorted(METHODS))
def test_emulated_fps_sample_counts(fps_emu, method):
    m = METHODS[method]
    dup = CLOUDS["duplicates"][0][:150]
    for K, s0 in ((1, 149), (150, 0), (150, 40)):  # K = 1, K = L
        np.testing.assert_array_equal(run_fps(fps_emu, dup, K, [s0], m, shared=True)[0], fps_reference(dup, K, s0))
    nanc = CLOUDS["nan_rows"][0][:100]
    got = run_fps(fps_emu, nanc, 120, [77], m, shared=True)[0]  # K > the finite points: padded with -1
    n_fin = int(np.isfinite(nanc).all(1).sum())
    assert n_fin < 100 and (got[n_fin:] == -1).all() and (got[:n_fin] >= 0).all()
    assert sorted(got[:n_fin].tolist()) == np.nonzero(np.isfinite(nanc).all(1))[0].tolist()  # (distinct points: each picked once)
    np.testing.assert_array_equal(got, fps_reference(nanc, 120, 77))
    none = np.full((40, 3), np.nan, np.float32)
    assert (run_fps(fps_emu, none, 5, [3], m, shared=True) == -1).all()


@pytest.mark.parametrize("method", sorted(METHODS))
def test_emulated_fps_start_out_of_range_is_the_lowest_finite_point(fps_emu, method):
    pts = CLOUDS["nan_rows"][0]
    want = fps_reference(pts, 16, 1)  # (index 0 is not finite)
    for s0 in (-5, 1500, 2 ** 31 - 1, 0):
        np.testing.assert_array_equal(run_fps(fps_emu, pts, 16, [s0], METHODS[method], shared=True)[0], want)


@pytest.mark.parametrize("method", sorted(METHODS))
def test_emulated_fps_lengths_shorter_than_the_cloud(fps_emu, method):
    a, b, c = CLOUDS["uniform"][0][:900], CLOUDS["clustered"][0][:900], CLOUDS["duplicates"][0][:900]
    pts = np.stack([a, b, c])
    lengths, starts = [900, 333, 0], [5, 400, 2]  # (start 400 is past its cloud's length: the lowest-index point instead)
    got = run_fps(fps_emu, pts, 40, starts, METHODS[method], lengths=lengths)
    for r in range(3):
        np.testing.assert_array_equal(got[r], fps_reference(pts[r], 40, starts[r], lengths[r]))
    assert (got[2] == -1).all() and got[1].max() < 333


@pytest.mark.parametrize("method", sorted(METHODS))
def test_emulated_fps_shared_cloud_equals_separate_calls(fps_emu, method):
    pts = CLOUDS["outliers"][0]
    starts = [11, 2000, 977]
    shared = run_fps(fps_emu, pts, 32, starts, METHODS[method], shared=True)
    copies = run_fps(fps_emu, np.stack([pts] * 3), 32, starts, METHODS[method])
    for r, s0 in enumerate(starts):
        single = run_fps(fps_emu, pts, 32, [s0], METHODS[method], shared=True)[0]
        np.testing.assert_array_equal(shared[r], single)
        np.testing.assert_array_equal(copies[r], single)
        np.testing.assert_array_equal(single, fps_reference(pts, 32, s0))


def test_emulated_fps_argument_checks(fps_emu):
    lib = fps_emu
    pts = np.zeros((50, 6), np.float32)
    idx, start = np.zeros((1, 8), np.int32), np.zeros(1, np.int32)
    ws = np.zeros(1 << 20, np.uint8)

    def call(L, D, K, method, wsb=ws.size):
        return lib.gsgen_fps(pts.ctypes.data, L, D, 0, None, start.ctypes.data, 1, K, idx.ctypes.data, ws.ctypes.data, wsb, method, None)
    assert call(50, 3, 0, BRUTE) == GSGEN_EINVAL and call(50, 3, 0, BUCKET) == GSGEN_EINVAL
    assert call(50, 5, 4, AUTO) == GSGEN_EUNSUPPORTED and call(50, 5, 4, BRUTE) == GSGEN_EUNSUPPORTED
    assert call(50, 6, 4, BUCKET) == GSGEN_EUNSUPPORTED and call(50, 3, 4, 3) == GSGEN_EUNSUPPORTED
    assert lib.gsgen_fps_workspace_bytes(50, 5, 1, 4, AUTO) == 0 and lib.gsgen_fps_workspace_bytes(50, 6, 1, 4, BUCKET) == 0
    for method in (BRUTE, BUCKET, AUTO):
        need = lib.gsgen_fps_workspace_bytes(50, 3, 1, 4, method)
        assert 0 < need <= ws.size
        assert call(50, 3, 4, method, need - 1) == GSGEN_EINVAL  # an undersized workspace
        assert call(50, 3, 4, method, need) == 0
    assert call(0, 3, 4, BRUTE) == GSGEN_EINVAL
    assert lib.gsgen_fps(None, 50, 3, 0, None, start.ctypes.data, 1, 4, idx.ctypes.data, ws.ctypes.data, ws.size, BRUTE, None) == GSGEN_EINVAL
    assert call(50, 6, 4, AUTO) == 0


def test_python_constants_are_the_kernels(fps_emu):
    from gsgen_amd import fps
    c = np.zeros(4, np.uint32)
    fps_emu.gsgen_fps_emu_constants(c.ctypes.data)
    assert c.tolist() == [fps.BRUTE_THREADS, fps.BRUTE_REG_POINTS, fps.BUCKETS_MAX, fps.AUTO_BUCKET_MIN_POINTS]
    assert fps.AUTO_BUCKET_MIN_POINTS & (fps.AUTO_BUCKET_MIN_POINTS - 1) == 0  # a power of two


def test_emulated_fps_pruning_is_real(fps_emu):
    """The bucket kernel is not a disguised full scan: a full scan visits every non-empty bucket at every pick.  On the uniform
    cloud of 3000 points at K = 64 the updates after picks 33 .. 63 (1-based; pick 64 is the last and updates nothing) visit fewer
    buckets than that, in total, and none of them visits more."""
    pts, s0 = CLOUDS["uniform"]
    assert pts.shape[0] == 3000
    idx = run_fps(fps_emu, pts, 64, [s0], BUCKET, shared=True)
    np.testing.assert_array_equal(idx[0], reference("uniform", 64))
    visits = np.zeros(64, np.uint32)
    full = fps_emu.gsgen_fps_emu_visits(visits.ctypes.data, 64)
    late = visits[32:63].astype(np.int64)
    print("non-empty buckets", full, "visits per pick", visits.tolist())
    assert full > 16 and visits[0] == full  # (the first pick lowers every m from +inf)
    assert (late <= full).all() and (late > 0).all()
    assert late.sum() < 31 * full
