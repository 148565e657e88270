"""gsgen_amd/csrc/marching_cubes.hip on the CPU SIMT emulator (oracle/emu) against the goldens and invariants of
tests/mesh_cases.py, the table generator, the OBJ reader and writer, and the argument checks of gsgen_amd.mesh that need no GPU.
The file is compiled without contraction, so the emulated kernels perform the GPU's fp32 operations in the GPU's order."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSGEN_EUNSUPPORTED, GSGEN_EINVAL, GSGEN_EWORKSPACE = -2, -3, -4


@pytest.fixture(scope="module")
def mc_emu(tmp_path_factory):
    """marching_cubes.hip compiled with g++ on the emulator headers, with the flags of oracle/Makefile's `emu` rule (into tmp:
    nothing under oracle/ changes)"""
    out = tmp_path_factory.mktemp("mc_emu") / "libmc_emu.so"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                           "-Wno-unknown-pragmas", "-DGSGEN_EMU_KNOBS=1", "-I", os.path.join(ROOT, "oracle", "emu"), "-x", "c++",
                           os.path.join(ROOT, "gsgen_amd", "csrc", "marching_cubes.hip"), "-o", str(out), "-lm"])
    lib = C.CDLL(str(out))
    u32, vp, f32, i32, sz = C.c_uint32, C.c_void_p, C.c_float, C.c_int, C.c_size_t
    lib.gsgen_marching_cubes_workspace_bytes.argtypes = [u32, u32, u32]
    lib.gsgen_marching_cubes_workspace_bytes.restype = sz
    lib.gsgen_marching_cubes.argtypes = [vp, u32, u32, u32, f32, vp, u32, vp, u32, vp, vp, sz, vp]
    lib.gsgen_marching_cubes.restype = i32
    return lib


def call(lib, field, thresh, verts, tris, counts, wsb=None):
    X, Y, Z = field.shape
    if wsb is None:
        nbytes = lib.gsgen_marching_cubes_workspace_bytes(X, Y, Z)
        assert nbytes > 0
        wsb = np.full(nbytes + 3, 0xA5, np.uint8)[3:]  # (an unaligned, dirty base: the carve aligns it and nothing is assumed zero)
    return lib.gsgen_marching_cubes(field.ctypes.data, X, Y, Z, thresh, verts.ctypes.data if verts is not None else None,
                                    len(verts) if verts is not None else 0, tris.ctypes.data if tris is not None else None,
                                    len(tris) if tris is not None else 0, counts.ctypes.data, wsb.ctypes.data, wsb.size, None)


def run_mc(lib, field, thresh=0.0):
    """the counting call, then the emit call into arrays of the exact size -> (verts, tris)"""
    field = np.ascontiguousarray(field, np.float32)
    counts = np.full(3, 99, np.uint32)
    assert call(lib, field, thresh, None, None, counts) == 0
    V, F = int(counts[0]), int(counts[1])
    assert counts[2] == (1 if V or F else 0)  # (capacities of 0)
    verts, tris, again = np.full((V, 3), np.nan, np.float32), np.full((F, 3), -1, np.int32), np.full(3, 99, np.uint32)
    assert call(lib, field, thresh, verts, tris, again) == 0
    assert again.tolist() == [V, F, 0]
    return verts, tris


# --- the goldens -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC.NAMES)
def test_restatement_of_the_vertex_stage_is_bit_equal_to_the_reference(name):
    g = MC.golden(name)
    MC.check_vertices(name, MC.restate_vertices(g["field"], g["thresh"]))
    assert (g["field"] - np.float32(g["thresh"]) != 0).all() and all((n - 1) & (n - 2) == 0 for n in g["field"].shape)


@pytest.mark.parametrize("name", MC.NAMES)
def test_the_goldens_pass_their_own_checks(name):
    g = MC.golden(name)
    MC.check_all(name, g["verts"], g["faces"])


@pytest.mark.parametrize("name", MC.NAMES)
def test_emulated_marching_cubes_against_the_golden(mc_emu, name):
    g = MC.golden(name)
    verts, tris = run_mc(mc_emu, g["field"], g["thresh"])
    MC.check_all(name, verts, tris)


def test_the_issues_figures_of_the_fixtures():
    for name, (V, F, _) in MC.FIGURES.items():
        g = MC.golden(name)
        assert (len(g["verts"]), len(g["faces"])) == (V, F)
    assert any(MC.golden(n)["thresh"] != 0 for n in MC.NAMES)
    for n in MC.NAMES:
        assert os.path.getsize(os.path.join(MC.GOLDEN, n + ".npz")) < 100_000


# --- the table ---------------------------------------------------------------------------------------------------------------
def edge_crossings(field, thresh=0.0):
    ins = MC.inside(field, thresh)
    return int((ins[1:] != ins[:-1]).sum() + (ins[:, 1:] != ins[:, :-1]).sum() + (ins[:, :, 1:] != ins[:, :, :-1]).sum())


def check_closed_mesh(field, verts, tris):
    assert verts.tobytes() == MC.restate_vertices(field, 0.0).tobytes()
    assert len(verts) == edge_crossings(field)
    if len(tris) == 0:
        assert len(verts) == 0
        return
    assert sorted(set(tris.reshape(-1).tolist())) == list(range(len(verts)))  # every sign-changing edge is used
    assert (tris[:, 0] != tris[:, 1]).all() and (tris[:, 1] != tris[:, 2]).all() and (tris[:, 0] != tris[:, 2]).all()
    assert MC.is_closed(tris)
    assert MC.signed_volume(verts, tris) > 0


def test_all_256_single_cube_cases_give_a_closed_mesh(mc_emu):
    """each case alone: its 8 corners in the middle cube of a 4^3 field of -1"""
    seen = 0
    for case in range(256):
        field = np.full((4, 4, 4), -1.0, np.float32)
        for c in range(8):
            if case >> c & 1:
                field[1 + (c & 1), 1 + (c >> 1 & 1), 1 + (c >> 2 & 1)] = 1.0 + 0.125 * c  # (unequal values: no vertex at a midpoint)
        verts, tris = run_mc(mc_emu, field)
        check_closed_mesh(field, verts, tris)
        assert MC.cube_cases(field, 0.0)[0][1, 1, 1] == case
        seen += len(tris) > 0
    assert seen == 255


def test_50_random_sign_fields_are_closed(mc_emu):
    rng = np.random.default_rng(11)
    for _ in range(50):
        field = np.full((7, 7, 7), -1.0, np.float32)
        field[1:-1, 1:-1, 1:-1] = rng.choice(np.float32([-1.0, 1.0, 0.5, -0.25]), size=(5, 5, 5))
        verts, tris = run_mc(mc_emu, field)
        check_closed_mesh(field, verts, tris)


def test_committed_table_is_what_the_generator_writes():
    """tools/gen_mc_table.py derives the 256 cases, checks them and renders mc_table.inc: the committed file is its output"""
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_mc_table.py"), "--check"])


# --- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_vertices_at_scan_edges_and_odd_shapes(mc_emu):
    """lattices of 1023, 1024 and 1025 points (one tile, exactly one, one point more), the smallest one, and shapes with n - 1 not a
    power of two: vertices bit-equal to the restatement, triangles closed where the border is outside"""
    rng = np.random.default_rng(5)
    for shape in ((3, 11, 31), (4, 16, 16), (5, 5, 41), (2, 2, 2), (2, 2, 300), (13, 7, 22)):
        field = rng.standard_normal(shape).astype(np.float32)
        verts, tris = run_mc(mc_emu, field, 0.25)
        assert verts.tobytes() == MC.restate_vertices(field, 0.25).tobytes(), shape
        assert len(verts) == edge_crossings(field, 0.25)
        e = MC.directed_edges(tris)
        assert len(np.unique(e, axis=0)) == len(e) and tris.min(initial=0) >= 0 and tris.max(initial=-1) < len(verts)
        if min(shape) >= 3:
            bordered = np.full(shape, -1.0, np.float32)
            inner = tuple(slice(1, n - 1) for n in shape)
            bordered[inner] = field[inner]
            check_closed_mesh(bordered, *run_mc(mc_emu, bordered))


def test_all_outside_all_inside_and_nan(mc_emu):
    for value in (-1.0, 1.0, np.nan):
        field = np.full((5, 6, 7), value, np.float32)
        verts, tris = run_mc(mc_emu, field)
        assert verts.shape == (0, 3) and tris.shape == (0, 3)
    field = np.full((5, 6, 7), np.nan, np.float32)  # a NaN is outside
    field[2, 3, 3] = 1.0
    verts, tris = run_mc(mc_emu, field)
    assert len(verts) == 6 and len(tris) == 8 and MC.is_closed(tris)


def test_argument_checks(mc_emu):
    lib = mc_emu
    field = np.random.default_rng(0).standard_normal((6, 6, 6)).astype(np.float32)
    V, F = (len(a) for a in run_mc(lib, field))
    verts, tris, counts = np.full((V, 3), 7.0, np.float32), np.full((F, 3), 7, np.int32), np.full(3, 7, np.uint32)
    need = lib.gsgen_marching_cubes_workspace_bytes(6, 6, 6)
    wsb = np.zeros(need, np.uint8)
    p = lambda a: a.ctypes.data  # noqa: E731

    def mc(X=6, Y=6, Z=6, grid=p(field), v=p(verts), vcap=V, t=p(tris), tcap=F, cnt=p(counts), ws=p(wsb), nbytes=need):
        return lib.gsgen_marching_cubes(grid, X, Y, Z, 0.0, v, vcap, t, tcap, cnt, ws, nbytes, None)
    for dims in ((1, 6, 6), (6, 1, 6), (6, 6, 1), (0, 6, 6), (1 << 11, 1 << 10, 1 << 10), (1 << 16, 1 << 16, 2), (1 << 31, 2, 2)):
        assert mc(*dims) == GSGEN_EUNSUPPORTED, dims
        assert lib.gsgen_marching_cubes_workspace_bytes(*dims) == 0
    assert lib.gsgen_marching_cubes_workspace_bytes(1 << 10, 1 << 10, 1 << 10) >= 4 << 30  # (2^30 points are taken)
    assert mc(grid=None) == GSGEN_EINVAL and mc(cnt=None) == GSGEN_EINVAL and mc(ws=None) == GSGEN_EINVAL
    assert mc(v=None) == GSGEN_EINVAL and mc(t=None) == GSGEN_EINVAL          # a capacity without its array
    assert mc(vcap=1 << 31) == GSGEN_EINVAL and mc(tcap=1 << 31) == GSGEN_EINVAL
    assert mc(nbytes=need - 1) == GSGEN_EWORKSPACE
    assert (verts == 7.0).all() and (tris == 7).all() and (counts == 7).all()  # a refused call enqueues nothing
    assert mc(v=None, vcap=0, t=None, tcap=0) == 0 and counts.tolist() == [V, F, 1]
    assert (verts == 7.0).all() and (tris == 7).all()
    assert mc() == 0 and counts.tolist() == [V, F, 0] and np.isfinite(verts).all() and tris.max() == V - 1


def test_capacity_overflow(mc_emu):
    g = MC.golden("blobs")
    field = g["field"]
    V, F = len(g["verts"]), len(g["faces"])
    full_v, full_t = run_mc(mc_emu, field)
    for vcap, tcap in ((V - 1, F - 1), (V, F - 1), (V - 1, F), (10, 0), (0, 10), (V + 5, F + 5)):
        verts, tris, counts = np.full((V + 8, 3), 7.0, np.float32), np.full((F + 8, 3), 7, np.int32), np.zeros(3, np.uint32)
        X, Y, Z = field.shape
        need = mc_emu.gsgen_marching_cubes_workspace_bytes(X, Y, Z)
        wsb = np.full(need, 0x5A, np.uint8)
        assert mc_emu.gsgen_marching_cubes(field.ctypes.data, X, Y, Z, 0.0, verts.ctypes.data, vcap, tris.ctypes.data, tcap, counts.ctypes.data,
                                           wsb.ctypes.data, need, None) == 0
        assert counts.tolist() == [V, F, int(vcap < V or tcap < F)]
        nv, nt = min(vcap, V), min(tcap, F)
        assert verts[:nv].tobytes() == full_v[:nv].tobytes() and (verts[nv:] == 7.0).all()  # the rows that fit; nothing past them
        assert tris[:nt].tobytes() == full_t[:nt].tobytes() and (tris[nt:] == 7).all()


def test_two_runs_are_bit_identical_in_a_dirty_unaligned_workspace(mc_emu):
    g = MC.golden("noise_17x5x9")
    field = g["field"]
    X, Y, Z = field.shape
    need = mc_emu.gsgen_marching_cubes_workspace_bytes(X, Y, Z)
    outs = []
    for fill, shift in ((0x00, 0), (0xFF, 1), (0xA5, 255)):
        wsb = np.full(need + shift, fill, np.uint8)[shift:]
        verts, tris, counts = np.zeros_like(g["verts"]), np.zeros(g["faces"].shape, np.int32), np.zeros(3, np.uint32)
        assert call(mc_emu, field, g["thresh"], verts, tris, counts, wsb) == 0
        outs.append(verts.tobytes() + tris.tobytes() + counts.tobytes())
    assert outs[0] == outs[1] == outs[2]


# --- OBJ ---------------------------------------------------------------------------------------------------------------------
def test_obj_round_trip_is_bit_exact(tmp_path):
    from gsgen_amd import io as GIO
    g = MC.golden("noise_17x5x9")
    rng = np.random.default_rng(3)
    verts = np.concatenate((g["verts"], (rng.standard_normal((64, 3)) * 10.0 ** rng.integers(-30, 30, (64, 3))).astype(np.float32),
                            np.float32([[0.0, -0.0, 1e-45], [3.4028235e38, -1.1754944e-38, 1 / 3]])))
    tris = np.concatenate((g["faces"], [[len(verts) - 1, 0, len(verts) - 2]]))
    path = tmp_path / "m.obj"
    GIO.write_obj(path, verts, tris)
    v2, t2 = GIO.read_obj(path)
    assert v2.dtype == np.float32 and v2.tobytes() == verts.tobytes() and np.array_equal(t2, tris)
    lines = open(path).read().splitlines()
    assert len(lines) == len(verts) + len(tris) and all(ln.startswith("v ") for ln in lines[:len(verts)])
    a, b, c = tris[0]
    assert lines[len(verts)] == f"f {a + 1} {b + 1} {c + 1}"                      # 1-based
    assert min(int(x) for ln in lines[len(verts):] for x in ln.split()[1:]) == 1
    assert not any("/" in ln or ln.startswith("vn") for ln in lines)               # no normals
    with pytest.raises(ValueError, match="triangle indices"):
        GIO.write_obj(tmp_path / "bad.obj", verts[:3], [[0, 1, 3]])
    import torch
    GIO.write_obj(path, torch.from_numpy(verts[:5].copy()), torch.tensor([[0, 1, 2]], dtype=torch.int32))
    v3, t3 = GIO.read_obj(path)
    assert v3.tobytes() == verts[:5].tobytes() and t3.tolist() == [[0, 1, 2]]
    GIO.write_obj(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v4, t4 = GIO.read_obj(path)
    assert v4.shape == (0, 3) and t4.shape == (0, 3)


# --- gsgen_amd.mesh: the refusals, which need neither a GPU nor the library -----------------------------------------------------
def test_python_refusals():
    import torch
    from gsgen_amd import mesh as GM
    with pytest.raises(ValueError, match="no CPU implementation"):
        GM.marching_cubes(torch.zeros(4, 4, 4), 0.5)
    with pytest.raises(ValueError, match=r"\[X, Y, Z\]"):
        GM.marching_cubes(torch.zeros(4, 4), 0.5)
    with pytest.raises(ValueError, match="at least 2"):
        GM.marching_cubes(torch.zeros(4, 1, 4), 0.5)
    with pytest.raises(ValueError, match="index_dtype"):
        GM.marching_cubes(torch.zeros(4, 4, 4), 0.5, index_dtype=torch.int16)
    with pytest.raises(ValueError, match="no CPU implementation"):
        GM.marching_cubes_into(torch.zeros(4, 4, 4), 0.5, None, None, torch.zeros(3, dtype=torch.int32))
    v = GM.index_to_world(torch.tensor([[0.0, 16.0, 32.0]]), 1.5, 33)
    assert v.dtype == torch.float32 and v.tolist() == [[-1.5, 0.0, 1.5]]


def test_package_exports_the_mesh_names():
    import gsgen_amd
    from gsgen_amd import mesh as GM
    assert gsgen_amd.mesh is GM
    for name in ("marching_cubes", "marching_cubes_into", "density_mesh", "mesh_from_ckpt"):
        assert getattr(gsgen_amd, name) is getattr(GM, name)
    from gsgen_amd import _capi
    assert "gsgen_marching_cubes" in _capi.EXPORTS and "gsgen_marching_cubes_workspace_bytes" in _capi.EXPORTS
