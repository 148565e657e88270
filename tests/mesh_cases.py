"""Checks shared by tests/test_mesh_host.py (marching_cubes.hip on the CPU emulator) and tests/test_gpu_mesh.py (the GPU): the
goldens of tests/golden/mesh (made by tests/golden/make_golden_mesh.py from the reference's shap_e/rendering/mc.py), a NumPy
restatement of the vertex stage, and mesh invariants.  Everything here is NumPy on the host; a mesh is (verts float32 [V,3] in
lattice index coordinates, tris integer [F,3]).

(a) check_vertices   count, order and bytes equal to the golden's
(b) check_triangles  per cube (a triangle belongs to the cube that holds its vertices' lattice edges and its centroid) the set of DIRECTED BOUNDARY SEGMENTS -- the
                     directed triangle edges whose reverse is not in the same cube -- equals the golden's, for every cube with no
                     ambiguous face (four corner signs alternating).  The set does not depend on how a cube's polygons are cut into
                     triangles; on an ambiguous face two consistent rules exist and the reference's is not pinned.
(c) check_whole      every directed edge occurs once and its reverse once (closed, consistently oriented), V - E + F as the golden's,
                     signed volume > 0 (normals from inside to outside)
(d) restate_vertices the vertex stage in NumPy fp32, for lattices where n - 1 is not a power of two (there the reference's own
                     v / (n - 1) * (n - 1) round trip moves its coordinates by up to 2 ulp); test_mesh_host.py asserts it bit-equal
                     to every golden
"""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh")
NAMES = ("sphere", "torus", "blobs", "blobs_thresh", "noise", "noise_17x5x9", "noise_3x17x2")
CLOSED = ("sphere", "torus", "blobs", "blobs_thresh", "noise", "noise_17x5x9")  # (an outside border; noise_3x17x2 has none)
# name -> (V, F, V - E + F) where the issue states them; surface cubes and those with an ambiguous face
FIGURES = {"sphere": (534, 1064, 2), "torus": (400, 800, 0), "noise": (5402, 11108, None)}
SURFACE_CUBES = {"sphere": (None, 0), "torus": (None, 0), "blobs": (None, 0), "blobs_thresh": (None, 0), "noise": (3971, 1436)}


@functools.lru_cache(maxsize=None)
def golden(name):
    """-> dict(field float32 [X,Y,Z], thresh float, verts float32 [V,3], faces int64 [F,3]); read-only arrays, loaded once"""
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        g = {"field": z["field"], "thresh": float(z["thresh"]), "verts": z["verts"], "faces": z["faces"].astype(np.int64)}
    for v in g.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return g


def inside(field, thresh):
    return (np.asarray(field, np.float32) - np.float32(thresh)) > 0


def restate_vertices(field, thresh):
    """(d): one vertex per sign-changing lattice edge, x-edges then y- then z-edges, each in the raster order of the lower point;
    t = s1 / (s1 - s2), v = t * p2 + (1 - t) * p1, every operation a separate fp32 NumPy ufunc (nothing fused)"""
    s = np.asarray(field, np.float32) - np.float32(thresh)
    ins = s > 0
    out = []
    for axis in range(3):
        lo = tuple(slice(0, -1) if a == axis else slice(None) for a in range(3))
        hi = tuple(slice(1, None) if a == axis else slice(None) for a in range(3))
        mask = ins[lo] != ins[hi]
        s1, s2 = s[lo][mask], s[hi][mask]
        p1 = np.argwhere(mask).astype(np.float32)
        p2 = p1.copy()
        p2[:, axis] += np.float32(1)
        t = (s1 / (s1 - s2))[:, None]
        out.append(t * p2 + (np.float32(1) - t) * p1)
    v = np.concatenate(out, axis=0)
    assert v.dtype == np.float32
    return v


def cube_cases(field, thresh):
    """-> (case uint8 [X-1,Y-1,Z-1] with corner bit dx + 2 dy + 4 dz, ambiguous bool of the same shape)"""
    ins = inside(field, thresh).astype(np.uint8)
    X, Y, Z = ins.shape
    corner = lambda dx, dy, dz: ins[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz]  # noqa: E731
    case = np.zeros((X - 1, Y - 1, Z - 1), np.uint8)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                case |= corner(dx, dy, dz) << (dx + 2 * dy + 4 * dz)
    amb = np.zeros(case.shape, bool)
    for axis in range(3):
        for side in (0, 1):
            ring = []
            for u, v in ((0, 0), (1, 0), (1, 1), (0, 1)):
                d = [0, 0, 0]
                d[axis], d[(axis + 1) % 3], d[(axis + 2) % 3] = side, u, v
                ring.append(corner(*d))
            amb |= (ring[0] == ring[2]) & (ring[1] == ring[3]) & (ring[0] != ring[1])
    return case, amb


def vertex_edges(field, thresh):
    """-> (lower lattice point int64 [V,3], axis int64 [V]) of the lattice edge every vertex lies on, in vertex order"""
    ins = inside(field, thresh)
    lower, axes = [], []
    for axis in range(3):
        lo = tuple(slice(0, -1) if a == axis else slice(None) for a in range(3))
        hi = tuple(slice(1, None) if a == axis else slice(None) for a in range(3))
        idx = np.argwhere(ins[lo] != ins[hi])
        lower.append(idx)
        axes.append(np.full(len(idx), axis, np.int64))
    return np.concatenate(lower, axis=0).astype(np.int64), np.concatenate(axes)


def cube_segments(field, thresh, verts, tris):
    """-> {cube (x, y, z): frozenset of directed boundary segments (a, b)}.  A triangle belongs to the cube that contains the lattice
    edges of its three vertices; where two cubes do (the edges share a face) the triangle's centroid decides.  The centroid alone
    is not enough: a field value of 1e-17 beside one of 0.1 (the torus has such) puts a vertex ON its lattice point in fp32, and a
    triangle of three such vertices has its centroid on a corner shared by eight cubes."""
    verts, tris = np.asarray(verts, np.float64), np.asarray(tris, np.int64)
    lower, axis = vertex_edges(field, thresh)
    assert len(lower) == len(verts)
    p = lower[tris]                                                   # [F,3 vertices,3 components]
    along = axis[tris][:, :, None] == np.arange(3)[None, None, :]     # component k is the vertex's edge axis
    lo, hi = np.where(along, p, p - 1).max(axis=1), p.min(axis=1)     # the cube's lower corner lies in [lo, hi] per component
    lo = np.maximum(lo, 0)
    hi = np.minimum(hi, np.asarray(field.shape) - 2)
    assert (lo <= hi).all(), "a triangle whose vertices share no cube"
    cubes = np.clip(np.floor(verts[tris].mean(axis=1)).astype(np.int64), lo, hi)
    per = {}
    for cube, (a, b, c) in zip(map(tuple, cubes.tolist()), tris.tolist()):
        per.setdefault(cube, set()).update(((a, b), (b, c), (c, a)))
    return {cube: frozenset(e for e in edges if (e[1], e[0]) not in edges) for cube, edges in per.items()}


def check_vertices(name, verts):
    g = golden(name)
    verts = np.asarray(verts)
    assert verts.dtype == np.float32 and verts.shape == g["verts"].shape, (verts.dtype, verts.shape, g["verts"].shape)
    assert verts.tobytes() == g["verts"].tobytes(), f"{name}: {int((verts != g['verts']).any(axis=1).sum())} vertices differ"


def check_triangles(name, verts, tris):
    g = golden(name)
    tris = np.asarray(tris)
    assert tris.shape == g["faces"].shape, (tris.shape, g["faces"].shape)  # (both tables triangulate a case's polygons: equal counts)
    case, amb = cube_cases(g["field"], g["thresh"])
    surface = (case != 0) & (case != 255)
    mine, ref = cube_segments(g["field"], g["thresh"], verts, tris), cube_segments(g["field"], g["thresh"], g["verts"], g["faces"])
    assert set(mine) == set(ref) == set(map(tuple, np.argwhere(surface).tolist()))
    left_out = 0
    for cube in ref:
        if amb[cube]:
            left_out += 1
            continue
        assert mine[cube] == ref[cube], (name, cube, int(case[cube]), sorted(mine[cube]), sorted(ref[cube]))
    assert left_out == int((amb & surface).sum())
    if name in SURFACE_CUBES:
        n_surface, n_left = SURFACE_CUBES[name]
        assert left_out == n_left and (n_surface is None or len(ref) == n_surface), (name, len(ref), left_out)
    print(f"{name}: {len(ref)} surface cubes, {left_out} with an ambiguous face left out")


def directed_edges(tris):
    t = np.asarray(tris, np.int64)
    return np.concatenate((t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]), axis=0)


def is_closed(tris):
    """every directed edge occurs once, and so does its reverse"""
    e = directed_edges(tris)
    if len(e) == 0:
        return True
    key = e[:, 0] * (e.max() + 1) + e[:, 1]
    rev = e[:, 1] * (e.max() + 1) + e[:, 0]
    return len(np.unique(key)) == len(key) and np.array_equal(np.sort(key), np.sort(rev))


def euler(n_verts, tris):
    e = np.sort(directed_edges(tris), axis=1)
    return n_verts - len(np.unique(e, axis=0)) + len(tris)


def signed_volume(verts, tris):
    v = np.asarray(verts, np.float64)[np.asarray(tris, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def check_whole(name, verts, tris):
    g = golden(name)
    tris = np.asarray(tris, np.int64)
    assert tris.min(initial=0) >= 0 and tris.max(initial=-1) < len(verts)
    assert (tris[:, 0] != tris[:, 1]).all() and (tris[:, 1] != tris[:, 2]).all() and (tris[:, 0] != tris[:, 2]).all()
    e = directed_edges(tris)
    assert len(np.unique(e, axis=0)) == len(e), f"{name}: a directed edge occurs twice"
    if name in CLOSED:
        assert is_closed(tris), f"{name}: not closed"
        assert signed_volume(verts, tris) > 0
    else:  # an open mesh: its border must be the golden's border
        def border(t):
            d = set(map(tuple, directed_edges(t).tolist()))
            return {x for x in d if (x[1], x[0]) not in d}
        assert border(tris) == border(g["faces"])
    assert euler(len(verts), tris) == euler(len(g["verts"]), g["faces"])
    if name in FIGURES:
        V, F, chi = FIGURES[name]
        assert (len(verts), len(tris)) == (V, F) and (chi is None or euler(len(verts), tris) == chi)


def check_all(name, verts, tris):
    check_vertices(name, verts)
    check_triangles(name, verts, tris)
    check_whole(name, verts, tris)
