"""gsgen_amd.mesh on the MI355X: the goldens and invariants of tests/mesh_cases.py through marching_cubes, the vertex stage
against its NumPy restatement at the scan's edges, the properties an exporter relies on (empty meshes, index types, input forms,
bit equality from run to run, a captured call, the overflow contract) and the lattice-to-mesh entry points."""
import numpy as np
import pytest
import torch

import mesh_cases as MC

pytestmark = pytest.mark.gpu

from gsgen_amd import mesh as GM  # noqa: E402

DEV = "cuda"


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(verts, tris):
    return verts.cpu().numpy(), tris.cpu().numpy()


@pytest.mark.parametrize("name", MC.NAMES)
def test_marching_cubes_against_the_golden(name):
    g = MC.golden(name)
    verts, tris = GM.marching_cubes(dev(g["field"]), g["thresh"])
    assert verts.dtype == torch.float32 and tris.dtype == torch.int32 and verts.is_cuda and tris.is_cuda
    MC.check_all(name, *host(verts, tris))


@pytest.mark.parametrize("shape", [(3, 11, 31), (4, 16, 16), (5, 5, 41), (65, 64, 65), (2, 2, 2), (2, 2, 300), (13, 7, 22)],
                         ids=lambda s: "x".join(map(str, s)))
def test_vertices_equal_the_restatement_at_the_scan_edges(shape):
    """1023, 1024 and 1025 points (the 1024-point tile), more than 256 tiles, the smallest lattice, one long row, odd sizes; with an
    outside border (where there is room for one) the mesh is closed, uses every vertex and has positive volume"""
    field = np.random.default_rng(sum(shape)).standard_normal(shape).astype(np.float32)
    if min(shape) >= 3:
        inner = tuple(slice(1, n - 1) for n in shape)
        bordered = np.full(shape, -1.0, np.float32)
        bordered[inner] = field[inner]
        field = bordered
    verts, tris = host(*GM.marching_cubes(dev(field), 0.25))
    want = MC.restate_vertices(field, 0.25)
    assert verts.shape == want.shape and verts.tobytes() == want.tobytes()
    e = MC.directed_edges(tris)
    assert len(np.unique(e, axis=0)) == len(e) and tris.min(initial=0) >= 0 and tris.max(initial=-1) < len(verts)
    if min(shape) >= 3 and len(tris):
        assert MC.is_closed(tris) and MC.signed_volume(verts, tris) > 0
        assert len(np.unique(tris)) == len(verts)


def test_all_outside_and_all_inside_are_empty():
    for value in (0.0, 1.0):
        verts, tris = GM.marching_cubes(torch.full((9, 8, 7), value, device=DEV), 0.5)
        assert verts.shape == (0, 3) and tris.shape == (0, 3) and verts.dtype == torch.float32 and tris.dtype == torch.int32


def test_index_dtype_input_forms_and_two_runs():
    g = MC.golden("noise_17x5x9")
    field = dev(g["field"])
    verts, tris = GM.marching_cubes(field, g["thresh"])
    v64, t64 = GM.marching_cubes(field, g["thresh"], index_dtype=torch.int64)
    assert t64.dtype == torch.int64 and torch.equal(t64, tris.long()) and torch.equal(v64.view(torch.int32), verts.view(torch.int32))
    again = GM.marching_cubes(field, g["thresh"])                                 # bit-identical from run to run
    assert torch.equal(again[0].view(torch.int32), verts.view(torch.int32)) and torch.equal(again[1], tris)
    strided = dev(np.ascontiguousarray(g["field"].transpose(2, 0, 1))).permute(1, 2, 0)
    assert not strided.is_contiguous() and strided.shape == field.shape
    for other in (strided, field.double()):                                       # made contiguous fp32
        v, t = GM.marching_cubes(other, g["thresh"])
        assert torch.equal(v.view(torch.int32), verts.view(torch.int32)) and torch.equal(t, tris)


def test_marching_cubes_into_replays_in_a_captured_graph():
    a, b = MC.golden("blobs"), MC.golden("noise")
    grid = dev(a["field"])
    vbuf, tbuf = torch.zeros(6000, 3, device=DEV), torch.zeros(12000, 3, device=DEV, dtype=torch.int32)
    counts = torch.zeros(3, device=DEV, dtype=torch.int32)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        GM.marching_cubes_into(grid, 0.0, vbuf, tbuf, counts)  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        GM.marching_cubes_into(grid, 0.0, vbuf, tbuf, counts)
    for g in (b, a):
        grid.copy_(dev(g["field"]))
        graph.replay()
        ev, et = GM.marching_cubes(grid, 0.0)
        torch.cuda.synchronize()
        V, F = len(g["verts"]), len(g["faces"])
        assert counts.tolist() == [V, F, 0]
        assert torch.equal(vbuf[:V].view(torch.int32), ev.view(torch.int32)) and torch.equal(tbuf[:F], et)


def test_overflow_sets_the_flag_and_writes_nothing_past_the_capacity():
    g = MC.golden("blobs")
    grid = dev(g["field"])
    V, F = len(g["verts"]), len(g["faces"])
    full_v, full_t = GM.marching_cubes(grid, g["thresh"])
    vbuf, tbuf = torch.full((V + 4, 3), 7.0, device=DEV), torch.full((F + 4, 3), 7, device=DEV, dtype=torch.int32)
    counts = torch.zeros(3, device=DEV, dtype=torch.int32)
    GM.marching_cubes_into(grid, g["thresh"], vbuf[:V - 1], tbuf[:F - 1], counts)
    assert counts.tolist() == [V, F, 1]                                           # the true counts
    assert torch.equal(vbuf[:V - 1].view(torch.int32), full_v[:V - 1].view(torch.int32)) and bool((vbuf[V - 1:] == 7.0).all())
    assert torch.equal(tbuf[:F - 1], full_t[:F - 1]) and bool((tbuf[F - 1:] == 7).all())
    GM.marching_cubes_into(grid, g["thresh"], vbuf[:V], tbuf[:F], counts)
    assert counts.tolist() == [V, F, 0]
    GM.marching_cubes_into(grid, g["thresh"], None, None, counts)                 # the counting call
    assert counts.tolist() == [V, F, 1] and bool((vbuf[V:] == 7.0).all()) and bool((tbuf[F:] == 7).all())
    with pytest.raises(ValueError, match="counts"):
        GM.marching_cubes_into(grid, 0.0, None, None, torch.zeros(3, device=DEV))
    with pytest.raises(ValueError, match="tris_buf"):
        GM.marching_cubes_into(grid, 0.0, vbuf, tbuf.long(), counts)


def test_density_mesh_and_mesh_from_ckpt_on_a_seeded_cloud(tmp_path):
    from gsgen_amd import io as GIO
    from gsgen_amd.density import density_grid
    gen = torch.Generator().manual_seed(200)
    N, L, reso = 200, 1.5, 33
    # (centres within 0.7 and scales below 0.2: the density at the lattice's border, 4 sigma and more away, is far below the
    # threshold, so the surface is closed)
    ckpt = {"mean": (torch.randn(N, 3, generator=gen) * 0.3).clamp(-0.7, 0.7), "qvec": torch.randn(N, 4, generator=gen),
            "svec": torch.log(0.1 + 0.1 * torch.rand(N, 3, generator=gen)), "alpha": torch.full((N,), 2.0)}
    ckpt = {k: v.to(DEV) for k, v in ckpt.items()}
    scale, opacity = torch.exp(ckpt["svec"]), torch.sigmoid(ckpt["alpha"])
    verts, tris = GM.density_mesh(ckpt["mean"], ckpt["qvec"], scale, opacity, L, reso)
    assert verts.shape[0] > 100 and tris.shape[0] > 100 and tris.dtype == torch.int32
    grid = density_grid(ckpt["mean"], ckpt["qvec"], scale, opacity, L, reso, 3, True)
    iv, it = GM.marching_cubes(grid, 0.5)
    assert torch.equal(it, tris) and torch.equal(GM.index_to_world(iv, L, reso).view(torch.int32), verts.view(torch.int32))
    # four fp32 roundings (the step, the product, L, the difference) of values of at most 2 L: each <= 2^-24 * 2 L
    want = iv.double().cpu() * (2.0 * L / (reso - 1)) - L
    err = float((verts.double().cpu() - want).abs().max())
    print(f"world map: max abs error {err:.3e}, bound {2.0 ** -20 * L:.3e}")
    assert err <= 2.0 ** -20 * L
    assert float(verts.abs().max()) < L and MC.is_closed(it.cpu().numpy()) and MC.signed_volume(*host(iv, it)) > 0
    cv, ct, cL = GM.mesh_from_ckpt(ckpt, reso=reso, K=3, thresh=0.5, L=L)
    assert cL == L and torch.equal(ct, tris) and torch.equal(cv.view(torch.int32), verts.view(torch.int32))
    av, at, aL = GM.mesh_from_ckpt(ckpt, reso=reso)                               # L from the cloud, the reference's default
    assert aL == ckpt["mean"].abs().max().item() * 1.1 and at.shape[0] > 100
    dv, dt = GM.density_mesh(ckpt["mean"], ckpt["qvec"], scale, opacity, aL, reso)
    assert torch.equal(dt, at) and torch.equal(dv.view(torch.int32), av.view(torch.int32))
    GIO.write_obj(tmp_path / "cloud.obj", cv, ct)                                 # a checkpoint to an .obj, nothing third-party
    rv, rt = GIO.read_obj(tmp_path / "cloud.obj")
    assert rv.tobytes() == cv.cpu().numpy().tobytes() and np.array_equal(rt, ct.cpu().numpy())
