"""gsgen_amd/csrc/knn.hip on the CPU SIMT emulator (oracle/emu), against an fp32 NumPy brute force: identical dist2 bits and
identical indices, on the clouds that stress the grid (clusters, duplicates, a plane, far outliers, NaN rows)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from knn_cases import brute, clouds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSGEN_EUNSUPPORTED, GSGEN_EINVAL = -2, -3


@pytest.fixture(scope="module")
def knn_emu(tmp_path_factory):
    """knn.hip compiled with g++ on the emulator headers, with the flags of oracle/Makefile's `emu` rule (into tmp: nothing under
    oracle/ changes)"""
    out = tmp_path_factory.mktemp("knn_emu") / "libknn_emu.so"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                           "-Wno-unknown-pragmas", "-DGSGEN_EMU_KNOBS=1", "-I", os.path.join(ROOT, "oracle", "emu"), "-x", "c++",
                           os.path.join(ROOT, "gsgen_amd", "csrc", "knn.hip"), "-o", str(out), "-lm"])
    lib = C.CDLL(str(out))
    lib.gsgen_knn_workspace_bytes.argtypes, lib.gsgen_knn_workspace_bytes.restype = [C.c_uint32, C.c_uint32], C.c_size_t
    lib.gsgen_knn.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.gsgen_knn.restype = C.c_int
    return lib


def run_knn(lib, pts, K):
    pts = np.ascontiguousarray(pts, np.float32)
    N = pts.shape[0]
    d = np.full((N, K), 7.0, np.float32)
    i = np.full((N, K), -7, np.int32)
    ws = np.zeros(lib.gsgen_knn_workspace_bytes(N, K) + 3, np.uint8)[3:]  # (an unaligned base: the carve aligns it)
    rc = lib.gsgen_knn(pts.ctypes.data, N, K, d.ctypes.data, i.ctypes.data, ws.ctypes.data, ws.size, None)
    assert rc == 0, rc
    return d, i


CLOUDS = clouds()


@pytest.mark.parametrize("name", sorted(CLOUDS))
@pytest.mark.parametrize("K", [1, 2, 4, 17, 32])
def test_emulated_knn_is_the_brute_force_bit_for_bit(knn_emu, name, K):
    pts = CLOUDS[name]
    d, i = run_knn(knn_emu, pts, K)
    bd, bi = brute(pts, K)
    np.testing.assert_array_equal(i, bi)
    np.testing.assert_array_equal(d.view(np.uint32), bd.view(np.uint32))


def test_emulated_knn_self_and_duplicate_order(knn_emu):
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0], [5, 5, 5]], np.float32)
    d, i = run_knn(knn_emu, pts, 4)
    assert i[0].tolist() == [0, 2, 3, 1] and i[2].tolist() == [0, 2, 3, 1]  # a lower-index duplicate comes before self
    assert d[0, 0] == 0 and d[2, 1] == 0
    assert i[4, 0] == 4 and d[4, 0] == 0.0


def test_emulated_knn_pads_short_rows(knn_emu):
    pts = np.array([[0, 0, 0], [np.nan, 0, 0], [1, 1, 1], [0, np.inf, 0]], np.float32)
    d, i = run_knn(knn_emu, pts, 3)
    assert i.tolist() == [[0, 2, -1], [-1, -1, -1], [2, 0, -1], [-1, -1, -1]]
    assert np.isinf(d[:, 2]).all() and np.isinf(d[1]).all() and np.isinf(d[3]).all()
    d, i = run_knn(knn_emu, np.full((5, 3), np.nan, np.float32), 2)  # no finite point at all
    assert (i == -1).all() and np.isinf(d).all()


def test_emulated_knn_is_deterministic(knn_emu):
    pts = CLOUDS["duplicates"]
    a = run_knn(knn_emu, pts, 8)
    b = run_knn(knn_emu, pts, 8)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_emulated_knn_argument_checks(knn_emu):
    lib = knn_emu
    pts = np.zeros((4, 3), np.float32)
    d, i = np.zeros((4, 33), np.float32), np.zeros((4, 33), np.int32)
    ws = np.zeros(1 << 16, np.uint8)
    call = lambda N, K, wsb=ws.size: lib.gsgen_knn(pts.ctypes.data, N, K, d.ctypes.data, i.ctypes.data, ws.ctypes.data, wsb, None)  # noqa: E731
    assert call(4, 0) == GSGEN_EUNSUPPORTED
    assert call(4, 33) == GSGEN_EUNSUPPORTED
    assert call(4, 5) == GSGEN_EINVAL  # K > N
    assert call(0, 1) == GSGEN_EINVAL
    assert call(4, 2, 16) == -4  # GSGEN_EWORKSPACE
    assert lib.gsgen_knn(None, 4, 2, d.ctypes.data, i.ctypes.data, ws.ctypes.data, ws.size, None) == GSGEN_EINVAL
    assert call(4, 4) == 0 and lib.gsgen_knn_workspace_bytes(4, 4) <= ws.size
    assert lib.gsgen_knn_workspace_bytes(0, 4) == 0 and lib.gsgen_knn_workspace_bytes(10, 33) == 0
