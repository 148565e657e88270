"""Generates gsgen_amd/csrc/mc_table.inc, the 256-case marching cubes table of gsgen_amd/csrc/marching_cubes.hip.

    python tools/gen_mc_table.py            # rewrites the file
    python tools/gen_mc_table.py --check    # exit 1 when the committed file differs from what this script generates

Nothing is typed in: every case is derived.  Conventions (marching_cubes.hip):
  corner c = dx + 2 dy + 4 dz, bit c of the case set when the corner is inside;
  edge   e = 4 axis + a + 2 b, with (a, b) the lower corner's offsets along the two other axes in ascending axis order
             (x-edges: (dy, dz), y-edges: (dx, dz), z-edges: (dx, dy)).
Per case:
  1. every face, its corners in counter-clockwise order seen from outside the cube, gives directed segments between its
     sign-changing edges: from the edge where the walk enters an inside run to the edge where it leaves that run.  A face whose
     four corners alternate has two inside runs of one corner each, so its two segments each cut off one inside corner -- a rule
     that reads the face's four signs only, so the two cubes that share the face draw the same segments;
  2. a sign-changing edge lies in two faces that walk it in opposite directions: it ends one segment and starts another, and
     following the segments closes the boundary loops;
  3. each loop is cut into triangles along diagonals that do not lie in a face of the cube (triangulate(): a fan where that
     is allowed): a diagonal in a face could coincide with one of the neighbouring cube and put four triangles on one edge.
The direction of step 1 makes the normals point from inside to outside (signed volume of a closed surface around an inside
region > 0).  self_check() proves for all 256 cases that the triangles use exactly the sign-changing edges, repeat no vertex and
no directed edge, and that every directed edge without its reverse in the cube lies in a face of the cube, where the neighbouring
cube supplies the reverse; a case has at most 5 triangles.  Closedness and the sign of the volume of whole meshes, all 256 cases
among them, are tested in tests/test_mesh_host.py.
"""
import itertools
import os
import sys

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gsgen_amd", "csrc", "mc_table.inc")
MAX_TRIS = 5


def corner(d):
    return d[0] + 2 * d[1] + 4 * d[2]


def edge_of(c1, c2):
    lo, hi = min(c1, c2), max(c1, c2)
    axis = {1: 0, 2: 1, 4: 2}[hi - lo]
    d = [(lo >> k) & 1 for k in range(3)]
    a, b = [d[k] for k in range(3) if k != axis]
    return 4 * axis + a + 2 * b


def faces():
    """six faces, each as four corner ids counter-clockwise seen from outside"""
    out = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, 1):
            ring = []
            for cu, cv in ((0, 0), (1, 0), (1, 1), (0, 1)):  # counter-clockwise about +axis (u, v, axis is right-handed)
                d = [0, 0, 0]
                d[axis], d[u], d[v] = side, cu, cv
                ring.append(corner(d))
            out.append(ring if side == 1 else ring[::-1])
    return out


FACES = faces()


def case_triangles(case):
    inside = [(case >> c) & 1 for c in range(8)]
    nxt = {}
    for ring in FACES:
        s = [inside[c] for c in ring]
        for k in range(4):
            if s[k] and not s[(k + 1) % 4]:           # the walk leaves the inside over edge (k, k + 1)
                j = k
                while s[(j - 1) % 4]:                 # back through this inside run to where the walk entered it
                    j = (j - 1) % 4
                leave = edge_of(ring[k], ring[(k + 1) % 4])
                enter = edge_of(ring[(j - 1) % 4], ring[j])
                assert enter not in nxt
                nxt[enter] = leave
    tris, seen = [], set()
    for e0 in sorted(nxt):
        if e0 in seen:
            continue
        loop, e = [], e0
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == e0 and len(loop) >= 3
        cut = triangulate(loop)
        assert cut is not None, (case, loop)
        tris.extend(cut)
    return tris


def on_one_face(p, q):
    """do the cube edges p and q lie in one face of the cube?"""
    (dp, ap), (dq, aq) = edge_ends(p), edge_ends(q)
    return any(ap != axis and aq != axis and dp[axis] == side and dq[axis] == side for axis in range(3) for side in (0, 1))


def triangulate(poly):
    """the first triangulation of the loop (apexes tried in loop order, so a fan from the first edge when that is allowed) none of
    whose diagonals joins two edges of one cube face, or None.  Such a diagonal would lie in the face -- an ambiguous one, with four
    sign-changing edges --, where the neighbouring cube may draw the same diagonal: four triangles on one mesh edge."""
    if len(poly) < 3:
        return []
    first, last = poly[0], poly[-1]
    for k in range(1, len(poly) - 1):
        if (k > 1 and on_one_face(first, poly[k])) or (k < len(poly) - 2 and on_one_face(poly[k], last)):
            continue
        left, right = triangulate(poly[:k + 1]), triangulate(poly[k:])
        if left is not None and right is not None:
            return left + [(first, poly[k], last)] + right
    return None


def table():
    t = [case_triangles(c) for c in range(256)]
    assert max(len(x) for x in t) <= MAX_TRIS, max(len(x) for x in t)
    return t


def edge_ends(e):
    """-> (lower corner offsets, axis)"""
    axis, a, b = e >> 2, e & 1, (e >> 1) & 1
    d = [0, 0, 0]
    others = [k for k in range(3) if k != axis]
    d[others[0]], d[others[1]] = a, b
    return d, axis


def self_check(t):
    for case in range(256):
        inside = [(case >> c) & 1 for c in range(8)]
        crossing = set()
        for e in range(12):
            d, axis = edge_ends(e)
            d2 = list(d)
            d2[axis] = 1
            if inside[corner(d)] != inside[corner(d2)]:
                crossing.add(e)
        used, directed = set(), set()
        for tri in t[case]:
            assert len(set(tri)) == 3, (case, tri)
            used.update(tri)
            for k in range(3):
                de = (tri[k], tri[(k + 1) % 3])
                assert de not in directed, (case, de)
                directed.add(de)
        assert used == crossing, (case, used, crossing)
        # closed in the cube's interior: a directed edge without its reverse must run along a face, and one with it must not
        for (p, q) in directed:
            assert ((q, p) in directed) != on_one_face(p, q), (case, p, q)


def render(t):
    lines = ["// mc_table.inc -- generated by tools/gen_mc_table.py (do not edit; the script documents the conventions and checks the",
             "// table).  Row = case (bit c = corner dx + 2 dy + 4 dz inside): up to 5 triangles of 3 edge numbers (4 axis + a + 2 b),",
             "// padded with 0; byte 15 = the number of triangles.",
             "static __device__ const uint8_t kMcTable[256 * 16] = {"]
    for case, tris in enumerate(t):
        flat = list(itertools.chain.from_iterable(tris))
        row = flat + [0] * (15 - len(flat)) + [len(tris)]
        lines.append("  " + ", ".join(f"{v:2d}" for v in row) + f",  // {case}")
    lines.append("};")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    T = table()
    self_check(T)
    text = render(T)
    if "--check" in sys.argv:
        sys.exit(0 if open(OUT).read() == text else 1)
    with open(OUT, "w") as f:
        f.write(text)
    print(OUT, "max triangles", max(len(x) for x in T), "total", sum(len(x) for x in T))
