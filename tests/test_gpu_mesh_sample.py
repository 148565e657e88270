"""gsgen_amd.mesh_sample on the MI355X: the cases and checks of tests/mesh_sample_cases.py through the Python module -- face choice
against exact integers (and one mesh of 2^20 + 5 faces, which takes the scan's third level), points / weights / attributes /
normals against fp64 within the counted bound, remove_close's mask equal to the sequential greedy -- and sample_surface_even end
to end."""
import numpy as np
import pytest
import torch

import mesh_sample_cases as MC

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEYS = {"points": "points", "face": "face", "bary": "barycentric", "attrs": "attributes", "normals": "normals"}


def sample(verts, tris, uni, attrs=None, want=MC.WANT):
    from gsgen_amd import mesh_sample as GS
    v, t = GS._mesh(torch.tensor(verts, device=DEV), torch.tensor(tris))
    a = None if attrs is None else torch.tensor(attrs, device=DEV)
    out = GS._sample_raw(v, t, torch.tensor(uni, device=DEV), a, points="points" in want, face="face" in want,
                         barycentric="bary" in want, normals="normals" in want)
    res = {k: out[KEYS[k]].cpu().numpy() for k in want}
    st = out["status"].cpu().numpy()
    ints = st[:1].view(np.uint32)
    res["status"] = (int(ints[0]), int(ints[1]), float(st[1]))
    return res


def thin(points, radius):
    from gsgen_amd.mesh_sample import remove_close
    p = torch.tensor(np.ascontiguousarray(points, np.float32), device=DEV)
    kept, mask = remove_close(p, float(radius))
    assert mask.dtype == torch.bool and torch.equal(kept, p[mask])
    return mask.cpu().numpy()


def test_face_choice_on_the_exact_grid():
    MC.check_exact_grid(sample)


@pytest.mark.parametrize("F", (1, 2, 1023, 1024, 1025, 4097, (1 << 20) + 5))
def test_face_choice_around_the_scan_tiles(F):
    MC.check_tile_edge(sample, F)


def test_zero_weight_faces_and_bad_indices():
    MC.check_zero_weight(sample)


def test_areas_over_18_orders_of_magnitude():
    MC.check_wide_areas(sample)


@pytest.mark.parametrize("level,M", ((2, 900), (3, 6000), (3, 30000)))
def test_icosphere_samples_against_fp64(level, M):
    MC.check_icosphere(sample, level, M, seed=level)
    print("worst error / (2^-24 max|v|):", MC.WORST)


def test_flip_edge_and_sample_counts():
    MC.check_flip_edge(sample)


def test_zero_total_area_and_empty_meshes():
    from gsgen_amd import mesh_sample as GS
    MC.check_zero_total(sample)
    verts = torch.tensor(MC.single_triangle()[0], device=DEV)
    flat = torch.tensor([[0, 0, 1]])
    with pytest.raises(ValueError, match="no area"):
        GS.sample_surface_even(verts, flat, 10)
    with pytest.raises(ValueError, match="no area"):
        GS.sample_surface_even(verts, torch.zeros(0, 3, dtype=torch.int64), 10)
    p, f = GS.sample_surface(verts, torch.zeros(0, 3, dtype=torch.int64), 4)
    assert bool(torch.isnan(p).all()) and f.tolist() == [-1] * 4
    p, f = GS.sample_surface(verts, torch.tensor([[0, 1, 2]]), 0)
    assert p.shape == (0, 3) and f.shape == (0,)
    assert float(GS.mesh_area(verts, flat)) == 0.0 and float(GS.mesh_area(verts, torch.zeros(0, 3, dtype=torch.int64))) == 0.0


def test_sample_surface_call_shapes():
    import gsgen_amd
    from gsgen_amd import mesh_sample as GS
    assert gsgen_amd.sample_surface_even is GS.sample_surface_even and gsgen_amd.mesh_sample is GS
    verts, tris = MC.icosphere(2)
    v, t = torch.tensor(verts, device=DEV), torch.tensor(tris.astype(np.int64), device=DEV)
    area = GS.mesh_area(v, t)
    assert area.dtype == torch.float64 and area.is_cuda and area.dim() == 0
    assert abs(float(area) - MC.weights64(verts, tris)[0].sum()) < 1e-12
    gen = torch.Generator(device=DEV).manual_seed(5)
    p, f = GS.sample_surface(v, t, 500, generator=gen)
    gen.manual_seed(5)
    uni = torch.rand(500, 3, generator=gen, device=DEV)
    p2, f2, at, nr, ba = GS.sample_surface(v, t, 500, uniforms=uni, attributes=v[:, :2], normals=True, barycentric=True)
    assert torch.equal(p, p2) and torch.equal(f, f2) and f.dtype == torch.int64 and p.dtype == torch.float32
    assert at.shape == (500, 2) and nr.shape == (500, 3) and ba.shape == (500, 2)
    assert float((at - p[:, :2]).abs().max()) <= MC.C_POINT * MC.EPS * 2  # (the points' own coordinates as attributes)
    radial = (nr * p).sum(1)
    assert float(radial.abs().min()) > 0.9 and bool((radial > 0).all() or (radial < 0).all())  # a sphere's face normals are radial
    assert GS.sample_surface(verts, tris, 10)[0].is_cuda  # NumPy arrays are uploaded
    with pytest.raises(ValueError):
        GS.sample_surface(v, t, 10, attributes=torch.zeros(len(verts), 9, device=DEV))
    with pytest.raises(ValueError):
        GS.remove_close(p, -1.0)
    with pytest.raises(ValueError):
        GS.remove_close(p, float("nan"))
    kept, mask = GS.remove_close(p[:0], 0.1)
    assert kept.shape == (0, 3) and mask.shape == (0,)


@pytest.mark.parametrize("count", (300, 2000))
def test_remove_close_on_icosphere_samples(count):
    kept = MC.check_icosphere_thin(sample, thin, count)
    print(f"count {count}: the greedy keeps {kept}")


THIN = MC.thin_cases()


@pytest.mark.parametrize("name", sorted(THIN))
def test_remove_close_cases(name):
    points, radius, kept = THIN[name]
    mask = MC.check_thin(name, thin, points, radius, kept)
    assert thin(points, radius).tobytes() == mask.tobytes()  # repeatable
    if name == "line":
        assert mask[::2].all() and not mask[1::2].any()
    if name == "duplicates":
        assert mask[7] and mask[np.all(points == points[7], axis=1)].sum() == 1  # the first of the equal rows survives


@pytest.mark.parametrize("count", (300, 2000))
def test_sample_surface_even_end_to_end(count):
    from gsgen_amd import mesh_sample as GS
    verts, tris = MC.icosphere(3)
    v, t = torch.tensor(verts, device=DEV), torch.tensor(tris, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(count)
    p, f, a = GS.sample_surface_even(v, t, count, generator=gen, attributes=v)
    assert p.shape == (count, 3) and f.shape == (count,) and a.shape == (count, 3)  # exactly count rows
    r = MC.even_radius(verts, tris, count)
    assert MC.no_pair_within(p.cpu().numpy(), r)
    # rows in ascending sample order: they are the first `count` survivors of the 3 * count samples of the same stream
    gen.manual_seed(count)
    uni = torch.rand(3 * count, 3, generator=gen, device=DEV)
    allp, allf = GS.sample_surface(v, t, 3 * count, uniforms=uni)
    keep = MC.greedy(allp.cpu().numpy(), r)
    first = np.flatnonzero(keep)[:count]
    assert torch.equal(p, allp[torch.tensor(first, device=DEV)]) and np.array_equal(f.cpu().numpy(), allf.cpu().numpy()[first])
    assert float((a - p).abs().max()) <= MC.C_POINT * MC.EPS  # the interpolated vertex positions are the points


def test_sample_surface_even_may_return_fewer_rows():
    from gsgen_amd import mesh_sample as GS
    verts, tris = MC.single_triangle()
    p, f = GS.sample_surface_even(torch.tensor(verts, device=DEV), torch.tensor(tris), 50, radius=0.3,
                                  generator=torch.Generator(device=DEV).manual_seed(1))
    assert 0 < p.shape[0] < 50 and f.shape[0] == p.shape[0] and bool((f == 0).all())
    assert MC.no_pair_within(p.cpu().numpy(), np.float32(0.3))


def test_load_mesh_as_pcd_tops_up(tmp_path):
    from gsgen_amd import io as GIO
    from gsgen_amd import mesh_sample as GS
    verts, tris = MC.icosphere(2)
    gen = torch.Generator(device=DEV).manual_seed(3)
    p, c = GS.load_mesh_as_pcd(verts, tris, num_points=777, generator=gen)
    assert p.shape == c.shape == (777, 3) and p.is_cuda and float(c.min()) >= 0 and float(c.max()) < 1
    assert float((p.norm(dim=1) - 1).abs().max()) < 0.03  # on the inscribed polyhedron
    for name, write in (("s.obj", GIO.write_obj), ("s.ply", GIO.write_ply_mesh)):
        write(tmp_path / name, verts, tris)
        q, _ = GS.load_mesh_as_pcd(tmp_path / name, num_points=100, generator=gen)
        assert q.shape == (100, 3) and float((q.norm(dim=1) - 1).abs().max()) < 0.03
    with pytest.raises(NotImplementedError):
        GS.load_mesh_as_pcd(tmp_path / "s.stl", num_points=10)
