"""gsgen_mesh_sample and gsgen_remove_close_* (gsgen_amd/csrc/mesh_sample.hip) on the CPU SIMT emulator (oracle/emu) through
ctypes: the cases and checks of tests/mesh_sample_cases.py -- face choice against exact integers, points / weights / attributes /
normals against fp64 within the counted bound, the keep mask of remove_close equal to the sequential greedy -- and what only a raw
call can show: sentinel rows past the end, outputs not asked for left untouched, a workspace off its alignment, error codes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mesh_sample_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSGEN_EINVAL, GSGEN_EWORKSPACE = -3, -4
u32, vp, sz, f32c = C.c_uint32, C.c_void_p, C.c_size_t, C.c_float
SENTINEL, PAST = np.float32(7.0), 5
SHAPES = {"points": (3, np.float32), "face": (None, np.int32), "bary": (2, np.float32), "attrs": (0, np.float32),
          "normals": (3, np.float32)}
GROUP = 8


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """mesh_sample.hip compiled unchanged with g++ on the emulator headers, with the flags of oracle/Makefile's `emu` rule (into
    tmp: nothing under oracle/ changes)"""
    out = tmp_path_factory.mktemp("mesh_sample_emu") / "libmesh_sample_emu.so"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                           "-Wno-unknown-pragmas", "-DGSGEN_EMU_KNOBS=1", "-I", os.path.join(ROOT, "oracle", "emu"), "-x", "c++",
                           os.path.join(ROOT, "gsgen_amd", "csrc", "mesh_sample.hip"), "-o", str(out), "-lm"])
    lib = C.CDLL(str(out))
    lib.gsgen_mesh_sample_workspace_bytes.argtypes, lib.gsgen_mesh_sample_workspace_bytes.restype = [u32], sz
    lib.gsgen_mesh_sample.argtypes = [vp, u32, vp, u32, vp, u32, vp, u32, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.gsgen_mesh_sample.restype = C.c_int
    lib.gsgen_remove_close_workspace_bytes.argtypes, lib.gsgen_remove_close_workspace_bytes.restype = [u32], sz
    lib.gsgen_remove_close_init.argtypes = [vp, u32, f32c, vp, vp, sz, vp]
    lib.gsgen_remove_close_init.restype = C.c_int
    lib.gsgen_remove_close_rounds.argtypes = [u32, u32, f32c, vp, vp, vp, sz, vp]
    lib.gsgen_remove_close_rounds.restype = C.c_int
    return lib


def make_sample(lib, shift=5):
    def sample(verts, tris, uni, attrs=None, want=MC.WANT):
        """every buffer is PAST rows longer than M and filled with a sentinel (checked untouched past M, and everywhere in a buffer
        not asked for); the workspace base is shifted off its alignment"""
        verts, tris = np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(tris, np.int32)
        uni = np.ascontiguousarray(uni, np.float32)
        M, F, A = len(uni), len(tris), 0 if attrs is None else attrs.shape[1]
        attrs = None if attrs is None else np.ascontiguousarray(attrs, np.float32)
        bufs = {}
        for k, (w, dt) in SHAPES.items():
            w = max(A, 1) if k == "attrs" else w
            bufs[k] = np.full((M + PAST,) if w is None else (M + PAST, w), SENTINEL, dt)
        ptr = lambda k: bufs[k].ctypes.data if k in want else None  # noqa: E731
        status = np.zeros(2, np.float64)
        ws = np.full(lib.gsgen_mesh_sample_workspace_bytes(F) + shift, 0xA5, np.uint8)[shift:]
        rc = lib.gsgen_mesh_sample(verts.ctypes.data, len(verts), tris.ctypes.data, F, uni.ctypes.data, M,
                                   None if attrs is None else attrs.ctypes.data, A, ptr("points"), ptr("face"), ptr("bary"),
                                   ptr("attrs"), ptr("normals"), status.ctypes.data, ws.ctypes.data, ws.size, None)
        assert rc == 0, rc
        for k, b in bufs.items():
            assert (b[M:] == b.dtype.type(SENTINEL)).all(), f"{k}: written past M"
            if k not in want:
                assert (b == b.dtype.type(SENTINEL)).all(), f"{k}: written though not asked for"
        out = {k: bufs[k][:M] for k in want}
        ints = status[:1].view(np.uint32)
        out["status"] = (int(ints[0]), int(ints[1]), float(status[1]))
        return out
    return sample


ROUNDS = {}


def make_thin(lib, shift=3):
    def thin(points, radius):
        """gsgen_amd.mesh_sample.remove_close's loop: groups of GROUP rounds until nothing is undecided; every group must lower
        the count"""
        points = np.ascontiguousarray(points, np.float32)
        N = len(points)
        keep = np.full(N + PAST, 9, np.uint8)
        remaining = np.full(1, 0xFFFFFFFF, np.uint32)
        ws = np.full(lib.gsgen_remove_close_workspace_bytes(N) + shift, 0xA5, np.uint8)[shift:]
        args = (N, float(radius), keep.ctypes.data)
        assert lib.gsgen_remove_close_init(points.ctypes.data, *args, ws.ctypes.data, ws.size, None) == 0
        before, groups = N, 0
        while N:
            assert lib.gsgen_remove_close_rounds(GROUP, *args, remaining.ctypes.data, ws.ctypes.data, ws.size, None) == 0
            groups += 1
            left = int(remaining[0])
            if left == 0:
                break
            assert left < before, (left, before)
            before = left
        ROUNDS[(N, float(radius))] = groups
        assert (keep[N:] == 9).all() and (keep[:N] <= 1).all()
        return keep[:N].astype(bool)
    return thin


def test_emulated_face_choice_on_the_exact_grid(emu):
    MC.check_exact_grid(make_sample(emu))


@pytest.mark.parametrize("F", (1, 2, 1023, 1024, 1025, 4097))
def test_emulated_face_choice_around_the_scan_tiles(emu, F):
    MC.check_tile_edge(make_sample(emu), F)


def test_emulated_zero_weight_faces_and_bad_indices(emu):
    MC.check_zero_weight(make_sample(emu))


def test_emulated_areas_over_18_orders_of_magnitude(emu):
    MC.check_wide_areas(make_sample(emu))


@pytest.mark.parametrize("level,M", ((2, 900), (3, 6000)))
def test_emulated_icosphere_samples_against_fp64(emu, level, M):
    MC.check_icosphere(make_sample(emu), level, M, seed=level)
    print("worst error / (2^-24 max|v|):", MC.WORST)


def test_emulated_flip_edge_and_sample_counts(emu):
    MC.check_flip_edge(make_sample(emu))


def test_emulated_zero_total_area(emu):
    MC.check_zero_total(make_sample(emu))


def test_emulated_output_subsets_and_workspace_alignment(emu):
    verts, tris, uni = MC.icosphere_uniforms(2, 257, 9)
    attrs = verts[:, ::-1].copy()
    full = make_sample(emu)(verts, tris, uni, attrs, want=tuple(SHAPES))
    for k in SHAPES:
        part = make_sample(emu, shift=0)(verts, tris, uni, attrs if k == "attrs" else None, want=(k,))
        assert part[k].tobytes() == full[k].tobytes(), k
    for shift in (1, 64, 255):
        again = make_sample(emu, shift=shift)(verts, tris, uni, attrs, want=tuple(SHAPES))
        assert all(again[k].tobytes() == full[k].tobytes() for k in SHAPES)


@pytest.mark.parametrize("count", (300, 2000))
def test_emulated_remove_close_on_icosphere_samples(emu, count):
    kept = MC.check_icosphere_thin(make_sample(emu), make_thin(emu), count)
    print(f"count {count}: the greedy keeps {kept}; groups of {GROUP} rounds: {ROUNDS}")


THIN = MC.thin_cases()


@pytest.mark.parametrize("name", sorted(THIN))
def test_emulated_remove_close_cases(emu, name):
    points, radius, kept = THIN[name]
    mask = MC.check_thin(name, make_thin(emu), points, radius, kept)
    assert make_thin(emu, shift=0)(points, radius).tobytes() == mask.tobytes()  # repeatable
    if name == "line":
        assert mask[::2].all() and not mask[1::2].any()  # (how many rounds that takes depends on what a round happens to see)
    if name == "duplicates":
        assert mask[7] and mask[np.all(points == points[7], axis=1)].sum() == 1  # the first of the equal rows survives


def test_emulated_mesh_sample_argument_checks(emu):
    lib = emu
    verts, tris = MC.icosphere(1)
    uni = MC.uniforms(0, 40)
    pts = np.full((40, 3), SENTINEL)
    status = np.zeros(2, np.float64)
    need = lib.gsgen_mesh_sample_workspace_bytes(len(tris))
    ws = np.zeros(need, np.uint8)

    def call(F=len(tris), M=40, attrs=None, A=0, attr_out=None, st=status.ctypes.data, w=ws.ctypes.data, wsb=need, t=tris.ctypes.data):
        return lib.gsgen_mesh_sample(verts.ctypes.data, len(verts), t, F, uni.ctypes.data, M, attrs, A, pts.ctypes.data, None, None,
                                     attr_out, None, st, w, wsb, None)
    a = np.zeros((len(verts), 9), np.float32)
    assert lib.gsgen_mesh_sample_workspace_bytes(0) == 0 and need > 0
    assert call(attrs=a.ctypes.data, A=9, attr_out=a.ctypes.data) == GSGEN_EINVAL
    assert call(A=3) == GSGEN_EINVAL and call(attrs=a.ctypes.data) == GSGEN_EINVAL and call(attr_out=a.ctypes.data) == GSGEN_EINVAL
    assert call(st=status.ctypes.data + 4) == GSGEN_EINVAL
    assert call(t=None) == GSGEN_EINVAL and call(w=None) == GSGEN_EINVAL
    assert call(wsb=need - 1) == GSGEN_EWORKSPACE and call(wsb=16) == GSGEN_EWORKSPACE
    assert call(F=0) == 0 and call(M=0, st=None) == 0
    assert (pts == SENTINEL).all() and (status == 0).all()  # no refused or empty call wrote
    assert call(M=0) == 0 and abs(status[1] - 4 * np.pi) < 1.0 and (pts == SENTINEL).all()  # M = 0 with a status block: the area
    assert call() == 0 and np.isfinite(pts).all()


def test_emulated_remove_close_argument_checks(emu):
    lib = emu
    pts = MC.uniforms(1, 50)
    keep = np.full(50, 9, np.uint8)
    rem = np.full(1, 77, np.uint32)
    need = lib.gsgen_remove_close_workspace_bytes(50)
    ws = np.zeros(need, np.uint8)

    def init(N=50, r=0.1, wsb=need):
        return lib.gsgen_remove_close_init(pts.ctypes.data, N, r, keep.ctypes.data, ws.ctypes.data, wsb, None)

    def rounds(N=50, r=0.1, wsb=need, n=4):
        return lib.gsgen_remove_close_rounds(n, N, r, keep.ctypes.data, rem.ctypes.data, ws.ctypes.data, wsb, None)
    assert lib.gsgen_remove_close_workspace_bytes(0) == 0 and need > 0
    assert [init(r=r) for r in (-1.0, float("nan"), -0.0001)] == [GSGEN_EINVAL] * 3
    assert [rounds(r=r) for r in (-1.0, float("nan"))] == [GSGEN_EINVAL] * 2
    assert init(wsb=need - 1) == GSGEN_EWORKSPACE and rounds(wsb=16) == GSGEN_EWORKSPACE
    assert init(N=0) == 0 and rounds(N=0) == 0
    assert (keep == 9).all() and rem[0] == 77  # no refused or empty call wrote
    assert init() == 0 and (keep == 0).all()
    assert rounds(n=0) == 0 and rem[0] == 50  # before the first round every finite point is undecided
    assert rounds(n=64) == 0 and rem[0] == 0
    np.testing.assert_array_equal(keep.astype(bool), MC.greedy(pts, 0.1))
    assert rounds(n=3) == 0 and rem[0] == 0  # rounds after the end change nothing
    np.testing.assert_array_equal(keep.astype(bool), MC.greedy(pts, 0.1))


def test_the_restatements_on_cases_with_known_answers():
    """NumPy alone: the unit sphere's area, the greedy on a line, the closed ball"""
    verts, tris = MC.icosphere(3)
    w = MC.weights64(verts, tris)[0]
    assert len(tris) == 1280 and abs(w.sum() - 4 * np.pi) < 0.1 and (w > 0).all()
    line, r, _ = THIN["line"]
    assert MC.greedy(line, r).tolist() == [i % 2 == 0 for i in range(300)]
    assert MC.greedy(*THIN["closed_ball"][:2]).tolist() == [True, False]
    assert MC.greedy(*THIN["just_outside"][:2]).tolist() == [True, True]
    assert MC.choose64(np.asarray([0.0, 0.0, 1.0, 0.0, 1.0]), np.asarray([0.0, 0.5, 0.75], np.float32))[0].tolist() == [2, 2, 4]
