"""gsgen_amd.io's mesh files with vertex normals and colours, on the host: write_obj with `v x y z r g b`, `vn` and `f a//a b//b c//c`
(and, with neither, the bytes it wrote before), read_obj_attributes, the unchanged read_obj on the coloured file, and the binary
little-endian PLY of write_ply_mesh / read_ply_mesh."""
import numpy as np
import pytest

from gsgen_amd import io as GIO


def mesh(seed=0, V=40, F=70):
    rng = np.random.default_rng(seed)
    verts = (rng.normal(size=(V, 3)) * rng.choice([1e-6, 1.0, 1e4], (V, 1))).astype(np.float32)
    tris = rng.integers(0, V, (F, 3)).astype(np.int32)
    n = rng.normal(size=(V, 3))
    normals = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    normals[3] = 0  # (a zero normal: a vertex whose gradient vanished)
    colors = rng.uniform(0, 1, (V, 3)).astype(np.float32)
    colors[0], colors[1] = (0.0, 1.0, 0.5), (np.float32(1 / 3), np.float32(2 / 255), np.float32(1e-8))
    return verts, tris, normals, colors


def old_obj_text(verts, tris):
    """the writer as it was before attributes: `v` lines with %.9g, then `f a b c` lines"""
    return ("".join("v %.9g %.9g %.9g\n" % (x, y, z) for x, y, z in verts.astype(np.float64).tolist())
            + "".join("f %d %d %d\n" % (a, b, c) for a, b, c in (tris.astype(np.int64) + 1).tolist()))


def test_obj_without_attributes_is_byte_identical_to_the_old_writer(tmp_path):
    verts, tris, _, _ = mesh()
    GIO.write_obj(tmp_path / "a.obj", verts, tris)
    assert (tmp_path / "a.obj").read_bytes() == old_obj_text(verts, tris).encode()
    GIO.write_obj(tmp_path / "b.obj", verts, tris, None, None)
    assert (tmp_path / "b.obj").read_bytes() == (tmp_path / "a.obj").read_bytes()
    v, t, n, c = GIO.read_obj_attributes(tmp_path / "a.obj")
    assert n is None and c is None and v.tobytes() == verts.tobytes() and np.array_equal(t, tris)


@pytest.mark.parametrize("with_normals,with_colors", [(True, True), (True, False), (False, True)])
def test_obj_round_trip_with_attributes(tmp_path, with_normals, with_colors):
    verts, tris, normals, colors = mesh(1)
    path = tmp_path / "m.obj"
    GIO.write_obj(path, verts, tris, normals if with_normals else None, colors if with_colors else None)
    v, t, n, c = GIO.read_obj_attributes(path)
    assert v.dtype == np.float32 and v.tobytes() == verts.tobytes() and t.dtype == np.int64 and np.array_equal(t, tris)
    assert (n.tobytes() == normals.tobytes()) if with_normals else n is None  # %.9g identifies a float32
    assert (c.tobytes() == colors.tobytes()) if with_colors else c is None
    ov, ot = GIO.read_obj(path)  # the plain reader keeps its return value and drops what it does not know
    assert ov.tobytes() == verts.tobytes() and np.array_equal(ot, tris)
    lines = path.read_text().splitlines()
    assert sum(ln.startswith("v ") for ln in lines) == len(verts) and sum(ln.startswith("vn ") for ln in lines) == (len(verts) if with_normals else 0)
    assert len(lines[0].split()) == (7 if with_colors else 4)
    a, b, cc = (tris[0] + 1).tolist()
    assert lines[-len(tris)] == (f"f {a}//{a} {b}//{b} {cc}//{cc}" if with_normals else f"f {a} {b} {cc}")


def test_obj_colours_are_clipped_and_sizes_are_checked(tmp_path):
    verts, tris, normals, colors = mesh(2)
    wild = colors.copy()
    wild[0], wild[1] = (-0.5, 1.5, 0.25), (2.0, -1e-9, 1.0)
    GIO.write_obj(tmp_path / "c.obj", verts, tris, None, wild)
    c = GIO.read_obj_attributes(tmp_path / "c.obj")[3]
    assert c.tobytes() == np.clip(wild, 0, 1).astype(np.float32).tobytes() and c[0].tolist() == [0.0, 1.0, 0.25]
    with pytest.raises(ValueError, match="normals"):
        GIO.write_obj(tmp_path / "bad.obj", verts, tris, normals[:-1])
    with pytest.raises(ValueError, match="colors"):
        GIO.write_ply_mesh(tmp_path / "bad.ply", verts, tris, None, colors[:-1])
    with pytest.raises(ValueError, match="triangle indices"):
        GIO.write_ply_mesh(tmp_path / "bad.ply", verts[:3], [[0, 1, 3]])
    import torch
    GIO.write_obj(tmp_path / "t.obj", torch.from_numpy(verts), torch.from_numpy(tris), torch.from_numpy(normals), torch.from_numpy(colors))
    GIO.write_obj(tmp_path / "n.obj", verts, tris, normals, colors)
    assert (tmp_path / "t.obj").read_bytes() == (tmp_path / "n.obj").read_bytes()  # tensors or arrays


@pytest.mark.parametrize("with_normals,with_colors", [(True, True), (True, False), (False, True), (False, False)])
def test_ply_mesh_round_trip(tmp_path, with_normals, with_colors):
    verts, tris, normals, colors = mesh(3)
    colors[2] = (-1.0, 2.0, 0.5)  # (clipped, then rounded: 0, 255, 128)
    path = tmp_path / "m.ply"
    GIO.write_ply_mesh(path, verts, tris, normals if with_normals else None, colors if with_colors else None)
    v, t, n, c = GIO.read_ply_mesh(path)
    assert v.dtype == np.float32 and v.tobytes() == verts.tobytes() and t.dtype == np.int64 and np.array_equal(t, tris)
    assert (n.tobytes() == normals.tobytes()) if with_normals else n is None
    if with_colors:
        want = np.rint(np.clip(colors.astype(np.float64), 0, 1) * 255).astype(np.uint8)
        assert c.dtype == np.uint8 and np.array_equal(c, want) and c[2].tolist() == [0, 255, 128] and c[0].tolist() == [0, 255, 128]
    else:
        assert c is None
    blob = path.read_bytes()
    head = blob[:blob.index(b"end_header\n")].decode().split("\n")
    props = ["property float x", "property float y", "property float z"]
    props += ["property float nx", "property float ny", "property float nz"] if with_normals else []
    props += ["property uchar red", "property uchar green", "property uchar blue"] if with_colors else []
    assert head[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {len(verts)}"]
    assert head[3:-1] == props + [f"element face {len(tris)}", "property list uchar int vertex_indices"]
    stride = 12 + (12 if with_normals else 0) + (3 if with_colors else 0)
    assert len(blob) == blob.index(b"end_header\n") + 11 + stride * len(verts) + 13 * len(tris)  # a face: uchar 3 + three int32


def test_empty_mesh_files(tmp_path):
    e3, ei = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    GIO.write_obj(tmp_path / "e.obj", e3, ei, e3, e3)
    v, t, n, c = GIO.read_obj_attributes(tmp_path / "e.obj")
    assert v.shape == (0, 3) and t.shape == (0, 3) and n is None and c is None
    GIO.write_ply_mesh(tmp_path / "e.ply", e3, ei, e3, e3)
    v, t, n, c = GIO.read_ply_mesh(tmp_path / "e.ply")
    assert v.shape == (0, 3) and t.shape == (0, 3) and n.shape == (0, 3) and c.shape == (0, 3) and c.dtype == np.uint8
