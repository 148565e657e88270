"""Cases, restatements and checks shared by tests/test_mesh_sample_host.py (the CPU emulator build of gsgen_amd/csrc/
mesh_sample.hip through ctypes) and tests/test_gpu_mesh_sample.py (the MI355X through gsgen_amd.mesh_sample).

Both hand the checks two callables:
    sample(verts, tris, uniforms, attrs=None, want=WANT) -> dict of the outputs named in `want` as NumPy arrays ("points" [M,3],
        "face" [M] int32, "bary" [M,2], "attrs" [M,A], "normals" [M,3]) and "status" = (bad_faces, zero_area_flag, total)
    thin(points, radius) -> the keep mask of remove_close, bool [N]

Restatements: weights64 / choose64 / combine64 are (a) and (b) of the kernel file's header in NumPy fp64 with a SEQUENTIAL sum;
greedy() is the sequential remove_close by brute force over all pairs with the fp32 predicate.

The rounding bound of a sample's coordinate.  With u = 2^-24 and m = the largest |coordinate| of the face's three vertices, the
kernel computes p = v0 + ((v1 - v0) r1 + (v2 - v0) r2) in fp32, r1, r2 >= 0, r1 + r2 <= 1 + u:
    e_k = fl(v_k - v0)         |e_k| <= 2 m, error <= 2 m u
    t_k = fl(e_k r_k)          inherits 2 m u r_k, adds u |e_k r_k| <= 2 m u r_k          -> 4 m u r_k
    s   = fl(t_1 + t_2)        inherits 4 m u (r1 + r2) <= 4 m u, adds u |s| <= 2 m u     -> 6 m u
    p   = fl(v0 + s)           inherits 6 m u, adds u |p| <= m u                          -> 7 m u
and one more m u covers the second-order terms and r1 + r2 up to 1 + u: C = 8.  Attributes: the same with their own values.
The normal is one rounding of an fp64 value of magnitude <= 1: 2^-24 absolute covers it and the fp64 noise.
"""
import numpy as np

EPS = 2.0 ** -24
C_POINT = 8.0
N_TOL = 2.0 ** -24
WANT = ("points", "face", "bary", "normals")
f32, f64 = np.float32, np.float64


# ---- meshes ---------------------------------------------------------------------------------------------------------------
def icosphere(level):
    """-> (verts float32 [V,3] on the unit sphere, tris int32 [F,3]), F = 20 * 4^level"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, f64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v, f64).astype(f32), np.asarray(f, np.int32)


def quad_grid(nx, ny, side=0.5, n_faces=None):
    """nx x ny squares of the given side in the plane z = 0, two right triangles each -> (verts, tris[:n_faces]); with a side that
    is a power of two every area and every partial sum of areas is exact in fp64, in any order"""
    xs, ys = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="xy")
    verts = np.stack([xs.ravel() * side, ys.ravel() * side, np.zeros(xs.size)], 1).astype(f32)
    q = (np.arange(ny)[:, None] * (nx + 1) + np.arange(nx)[None, :]).ravel()
    a, b, c, d = q, q + 1, q + nx + 1, q + nx + 2
    tris = np.stack([np.stack([a, b, c], 1), np.stack([b, d, c], 1)], 1).reshape(-1, 3).astype(np.int32)
    return verts, tris[:n_faces]


def single_triangle():
    return np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f32), np.asarray([[0, 1, 2]], np.int32)


# ---- the fp64 restatement of (a) and (b) -----------------------------------------------------------------------------------
def weights64(verts, tris):
    """-> (w [F] float64, cross [F,3], length [F], bad_faces)"""
    V = len(verts)
    ok = ((tris >= 0) & (tris < V)).all(1)
    t = np.where(ok[:, None], tris, 0)
    p = verts[t].astype(f64) if V else np.zeros((len(tris), 3, 3))
    a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    with np.errstate(all="ignore"):
        c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        ln = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    fin = np.isfinite(verts[t]).all((1, 2)) if V else np.zeros(len(tris), bool)
    w = np.where(ok & fin & (ln > 0), 0.5 * ln, 0.0)
    return w, c, ln, int((~ok).sum())


def choose64(w, u_face):
    """np.searchsorted(cumsum(w), u * total), then forward over zero-weight faces -> (face [M], pick [M], cum [F])"""
    cum = np.cumsum(w)
    pick = u_face.astype(f64) * cum[-1]
    i = np.searchsorted(cum, pick, side="left")
    nxt = np.full(len(w) + 1, len(w), np.int64)  # nxt[i] = the first j >= i with w[j] > 0
    for j in range(len(w) - 1, -1, -1):
        nxt[j] = j if w[j] > 0 else nxt[j + 1]
    return nxt[i], pick, cum


def flip32(r1, r2):
    r1, r2 = r1.astype(f32), r2.astype(f32)
    fl = (r1 + r2) > f32(1)
    return np.where(fl, f32(1) - r1, r1).astype(f32), np.where(fl, f32(1) - r2, r2).astype(f32)


def combine64(vals, tris, face, r1, r2):
    """a0 + (a1 - a0) r1 + (a2 - a0) r2 in fp64 on the given faces -> (value [M,A], m [M,A] = max |a_k|)"""
    p = vals[tris[face]].astype(f64)
    out = p[:, 0] + (p[:, 1] - p[:, 0]) * r1.astype(f64)[:, None] + (p[:, 2] - p[:, 0]) * r2.astype(f64)[:, None]
    return out, np.abs(p).max(1)


WORST = {}  # check name -> the largest observed error / (EPS * m), for the record


def check_faces(name, sample, verts, tris, uni, expect=None):
    """the kernel's face index equals the restatement's for EVERY sample (meshes whose partial sums of areas are exact in fp64, or
    uniforms aimed away from the boundaries); status as restated"""
    w, _, _, bad = weights64(verts, tris)
    face, pick, cum = choose64(w, uni[:, 0])
    out = sample(verts, tris, uni)
    nb, zero, total = out["status"]
    assert (nb, zero) == (bad, 0), (name, out["status"])
    assert abs(total - cum[-1]) <= 1e-13 * cum[-1], (name, total, cum[-1])
    np.testing.assert_array_equal(out["face"], face.astype(np.int32), err_msg=name)
    if expect is not None:
        np.testing.assert_array_equal(out["face"], np.asarray(expect, np.int32), err_msg=name)
    return out, w


def check_values(name, verts, tris, uni, out, attrs=None):
    """points, weights, attributes and normals against fp64 on the kernel's own face index, within the counted bounds"""
    face = out["face"].astype(np.int64)
    w, c, ln, _ = weights64(verts, tris)
    assert (face >= 0).all() and (face < len(tris)).all() and (w[face] > 0).all(), name
    r1, r2 = flip32(uni[:, 1], uni[:, 2])
    assert out["bary"].tobytes() == np.stack([r1, r2], 1).tobytes(), name  # (the flip is exact in fp32)
    assert (out["bary"] >= 0).all() and (out["bary"] <= 1).all() and (out["bary"].astype(f64).sum(1) <= 1 + EPS).all(), name
    p64, m = combine64(verts, tris, face, r1, r2)
    err = np.abs(out["points"].astype(f64) - p64)
    assert (err <= C_POINT * EPS * m).all(), (name, (err / np.maximum(EPS * m, 1e-300)).max())
    WORST[name] = float((err[m > 0] / (EPS * m[m > 0])).max()) if (m > 0).any() else 0.0
    n64 = c[face] / ln[face][:, None]
    if "normals" in out:
        assert (np.abs(out["normals"].astype(f64) - n64) <= N_TOL).all(), name
    v0 = verts[tris[face, 0]].astype(f64)
    dist = np.abs(((out["points"].astype(f64) - v0) * n64).sum(1))
    assert (dist <= (np.abs(n64) * C_POINT * EPS * m).sum(1)).all(), name  # (within the bound of the triangle's plane)
    if attrs is not None:
        a64, ma = combine64(attrs, tris, face, r1, r2)
        ea = np.abs(out["attrs"].astype(f64) - a64)
        assert (ea <= C_POINT * EPS * ma).all(), (name, (ea / np.maximum(EPS * ma, 1e-300)).max())


def step(x, up):
    return np.nextafter(f32(x), f32(2.0 if up else -1.0))


def uniforms(seed, M):
    return np.random.default_rng(seed).random((M, 3), dtype=f32)


# ---- face choice: exact integers -------------------------------------------------------------------------------------------
def check_exact_grid(sample):
    """128 right triangles with legs 0.5 (area 1/8, total 16): u = k / 128 gives pick = cum[k - 1] exactly -> face k - 1 (the tie
    rule: the first i with cum[i] >= pick), one fp32 step above -> k, one below -> k - 1"""
    verts, tris = quad_grid(8, 8)
    u, expect = [], []
    for k in range(128):
        u += [f32(k / 128.0), step(k / 128.0, True)]
        expect += [max(k - 1, 0), k]
        if k:
            u.append(step(k / 128.0, False))
            expect.append(k - 1)
    uni = uniforms(1, len(u))
    uni[:, 0] = u
    out, _ = check_faces("exact_grid", sample, verts, tris, uni, expect=expect)
    assert out["status"][2] == 16.0
    check_values("exact_grid", verts, tris, uni, out)


def check_tile_edge(sample, F):
    """F exact triangles: uniforms aimed at the middle of every face within 3 of a multiple of 1024 or of an end, and random ones"""
    nx = int(np.ceil(np.sqrt(F / 2.0))) + 1
    verts, tris = quad_grid(nx, nx, n_faces=F)
    assert len(tris) == F
    near = np.unique(np.clip(np.concatenate([np.arange(-3, 4) + e for e in list(range(0, F + 1024, 1024)) + [F]]), 0, F - 1))
    near = near[np.linspace(0, len(near) - 1, min(len(near), 600)).astype(int)]
    uni = uniforms(F, len(near) + 200)
    uni[:len(near), 0] = ((near + 0.5) / F).astype(f32)
    out, _ = check_faces(f"F={F}", sample, verts, tris, uni)
    np.testing.assert_array_equal(out["face"][:len(near)], near)
    assert out["status"][2] == F / 8.0
    check_values(f"F={F}", verts, tris, uni, out)


def zero_weight_mesh():
    """an 6 x 6 exact grid (72 faces) with zero-weight faces leading (3), interleaved and trailing (3): degenerate (a repeated
    vertex), a NaN vertex, an Inf vertex, indices -1 and V (bad_faces = 4)"""
    verts, tris = quad_grid(6, 6)
    V = len(verts)
    verts = np.concatenate([verts, [[np.nan, 0, 0], [np.inf, 1, 1]]]).astype(f32)
    deg, nan, inf, neg, big = [0, 0, 1], [0, 1, V], [2, V + 1, 3], [0, -1, 2], [0, 1, V + 2]
    rows = [deg, nan, neg] + list(tris[:10]) + [big, deg] + list(tris[10:11]) + [inf] + list(tris[11:40]) + [neg, nan] + \
        list(tris[40:]) + [deg, big, nan]
    return verts, np.asarray(rows, np.int32)


def check_zero_weight(sample):
    verts, tris = zero_weight_mesh()
    w = weights64(verts, tris)[0]
    cum = np.cumsum(w)
    assert (w[:3] == 0).all() and (w[-3:] == 0).all() and cum[-1] == 72 / 8.0
    u = [f32(0)] + [f32(c / cum[-1]) for c in np.unique(cum)[:-1]] + [step(c / cum[-1], True) for c in np.unique(cum)[:-1]] + \
        [step(1.0, False)]
    uni = uniforms(3, len(u) + 300)
    uni[:len(u), 0] = u
    out, _ = check_faces("zero_weight", sample, verts, tris, uni)
    assert out["face"][0] == 3 and out["status"][0] == 4  # (u = 0 skips the leading zero-weight faces)
    check_values("zero_weight", verts, tris, uni, out)


def check_wide_areas(sample):
    """31 right triangles with legs 2^(k - 30), k = 0..30, smallest first: areas 2^-61 .. 2^-1, 18 orders of magnitude.  Ascending,
    every partial sum that a small face's boundary depends on is exact; the uniforms aim at the middle of every face"""
    verts, tris = [], []
    for k in range(31):
        s = 2.0 ** (k - 30)
        verts += [[3.0, 0, 0], [3.0 + s, 0, 0], [3.0, s, 0]] if k >= 8 else [[0, 0, 0], [s, 0, 0], [0, s, 0]]
        tris.append([3 * k, 3 * k + 1, 3 * k + 2])
    verts, tris = np.asarray(verts, f32), np.asarray(tris, np.int32)
    w = weights64(verts, tris)[0]
    np.testing.assert_array_equal(w, 2.0 ** (2.0 * np.arange(31) - 61))
    cum = np.cumsum(w)
    mid = (cum - 0.5 * w) / cum[-1]
    uni = uniforms(5, 31 * 3)
    uni[:, 0] = np.repeat(mid, 3).astype(f32)
    assert uni[0, 0] > 0 and uni[0, 0] < 1e-18
    out, _ = check_faces("wide_areas", sample, verts, tris, uni, expect=np.repeat(np.arange(31), 3))
    check_values("wide_areas", verts, tris, uni, out)


def icosphere_uniforms(level, M, seed):
    """random uniforms none of whose picks lies within 1e-12 of the total of a face boundary (re-seeded otherwise)"""
    verts, tris = icosphere(level)
    w = weights64(verts, tris)[0]
    cum = np.cumsum(w)
    for s in range(seed, seed + 20):
        uni = uniforms(s, M)
        pick = uni[:, 0].astype(f64) * cum[-1]
        j = np.searchsorted(cum, pick)
        gap = np.minimum(np.abs(cum[np.minimum(j, len(cum) - 1)] - pick), np.abs(cum[np.maximum(j - 1, 0)] - pick))
        if gap.min() > 1e-12 * cum[-1]:
            return verts, tris, uni
    raise AssertionError("no seed with a safe margin")


def check_icosphere(sample, level, M, seed):
    verts, tris, uni = icosphere_uniforms(level, M, seed)
    attrs = np.random.default_rng(seed + 100).uniform(-2, 2, (len(verts), 5)).astype(f32)
    out = sample(verts, tris, uni, attrs, want=WANT + ("attrs",))
    face = choose64(weights64(verts, tris)[0], uni[:, 0])[0]
    np.testing.assert_array_equal(out["face"], face.astype(np.int32))  # (every sample: none is left out)
    assert out["status"][:2] == (0, 0) and abs(out["status"][2] - 4 * np.pi) < 0.6  # (inscribed: a little under the sphere)
    check_values(f"icosphere{level}_{M}", verts, tris, uni, out, attrs)
    return verts, tris, uni, out


def check_flip_edge(sample):
    """r1 + r2 exactly 1 (no flip) and one fp32 step above (flip), on a triangle with awkward coordinates; M = 1, 63, 65, 257"""
    verts = np.asarray([[0.1, -0.7, 0.3], [1.3, 0.2, -0.9], [-0.4, 1.1, 0.6], [0.2, 0.2, 2.0]], f32)
    tris = np.asarray([[0, 1, 2], [1, 3, 2]], np.int32)
    for M in (1, 63, 65, 257):
        uni = uniforms(M, M)
        uni[0, 1] = f32(0.625)
        r1 = uni[:, 1].copy()
        uni[::3, 2] = f32(1) - r1[::3]
        up = f32(1) - r1[1::3]
        while ((r1[1::3] + up) <= f32(1)).any():  # the smallest r2 whose fp32 sum with r1 exceeds 1
            up = np.where((r1[1::3] + up) <= f32(1), np.nextafter(up, f32(2)), up)
        uni[1::3, 2] = up
        ok = (uni[:, 1] + uni[:, 2] == f32(1))[::3]
        out = sample(verts, tris, uni, verts[:, :2].copy(), want=WANT + ("attrs",))
        r1f, r2f = flip32(uni[:, 1], uni[:, 2])
        assert ok[0] and (r2f[::3][ok] == uni[::3, 2][ok]).all()  # the fp32 sum is exactly 1: not flipped
        fl = (uni[:, 1] + uni[:, 2]) > f32(1)
        assert fl[1::3].all() and (r2f[fl] == f32(1) - uni[fl, 2]).all()  # one step above: flipped
        check_values(f"flip_M={M}", verts, tris, uni, out, verts[:, :2].copy())
        assert out["points"].shape == (M, 3)


def check_zero_total(sample):
    """a mesh of degenerate and bad faces only: NaN everywhere, face -1, the flag set"""
    verts = single_triangle()[0]
    tris = np.asarray([[0, 0, 1], [1, 1, 1], [0, 1, 7]], np.int32)
    out = sample(verts, tris, uniforms(0, 70), verts.copy(), want=WANT + ("attrs",))
    assert out["status"] == (1, 1, 0.0)
    assert (out["face"] == -1).all() and all(np.isnan(out[k]).all() for k in ("points", "bary", "normals", "attrs"))


# ---- remove_close ----------------------------------------------------------------------------------------------------------
def greedy(points, radius, chunk=512):
    """the sequential loop: keep i iff finite and no kept j < i with (dx dx + dy dy) + dz dz <= r r, all in fp32"""
    p = np.ascontiguousarray(points, f32)
    N = len(p)
    with np.errstate(over="ignore"):
        r2 = f32(radius) * f32(radius)
    fin = np.isfinite(p).all(1)
    lower = []
    with np.errstate(all="ignore"):
        for a in range(0, N, chunk):
            q = p[a:a + chunk]
            dx, dy, dz = (q[:, None, k] - p[None, :a + chunk, k] for k in range(3))
            near = ((dx * dx + dy * dy) + dz * dz) <= r2
            near &= fin[None, :a + chunk] & fin[a:a + chunk, None]
            near &= np.arange(a + chunk)[None, :near.shape[1]] < (a + np.arange(len(q)))[:, None]
            lower += [np.flatnonzero(row) for row in near]
    keep = np.zeros(N, bool)
    for i in range(N):
        keep[i] = fin[i] and not keep[lower[i]].any()
    return keep


def no_pair_within(points, radius):
    p = np.ascontiguousarray(points, f32)
    r2 = f32(radius) * f32(radius)
    for a in range(0, len(p), 512):
        dx, dy, dz = (p[a:a + 512, None, k] - p[None, :, k] for k in range(3))
        near = ((dx * dx + dy * dy) + dz * dz) <= r2
        near[np.arange(len(dx)), a + np.arange(len(dx))] = False
        if near.any():
            return False
    return True


def check_thin(name, thin, points, radius, expect_kept=None):
    points = np.ascontiguousarray(points, f32)
    want = greedy(points, radius)
    got = thin(points, radius)
    assert got.dtype == bool and got.shape == want.shape, name
    np.testing.assert_array_equal(got, want, err_msg=name)
    if expect_kept is not None:
        assert int(got.sum()) == expect_kept, (name, int(got.sum()))
    return got


def even_radius(verts, tris, count):
    return f32(np.sqrt(weights64(verts, tris)[0].sum() / (3 * count)))


def thin_cases():
    """name -> (points, radius, kept or None)"""
    rng = np.random.default_rng(11)
    cases = {}
    r = f32(0.37)
    line = np.zeros((300, 3), f32)
    line[:, 0] = (np.arange(300) * (0.9 * float(r))).astype(f32)
    line += f32(5.0)
    cases["line"] = (line, r, 150)  # every point depends on its predecessor: 300 rounds; the even indices survive
    cases["line_shuffled"] = (line[rng.permutation(300)], r, None)  # priority is the index, not the position
    cases["closed_ball"] = (np.asarray([[0, 0, 0], [0.75, 1, 0]], f32), f32(1.25), 1)  # d2 = 1.5625 = r r exactly
    cases["just_outside"] = (np.asarray([[0, 0, 0], [0.75, np.nextafter(f32(1), f32(2)), 0]], f32), f32(1.25), 2)
    cloud = rng.uniform(-1, 1, (1200, 3)).astype(f32)
    dup = cloud.copy()
    dup[8 + rng.choice(1192, 500, replace=False)] = dup[7]  # (501 equal rows, row 7 the first)
    cases["duplicates"] = (dup, f32(0.05), None)
    cases["single_cell"] = (rng.uniform(0, 1, (700, 3)).astype(f32), f32(2.0), 1)  # the ball holds the whole box
    cases["single_cell_sparse"] = (rng.uniform(0, 0.6, (700, 3)).astype(f32), f32(0.55), None)
    # 2 000 points in a box 10^6 radii long and 100 wide, pinned by two corner points: the budget of 2 000 cells binds, and the
    # smallest side that fits it is the length / 2 000 = 500 radii, with cell borders at x = k / 2 (DESIGN.md "Mesh sampling": the
    # side grows, no cell is dropped).  600 pairs 0.73 radii apart are planted across the borders k = 1 .. 600
    rr = f32(1e-3)
    k = np.arange(1, 601)[:, None] * 0.5
    yz = rng.uniform(0.01, 0.09, (600, 2))
    lo_side = np.concatenate([k - 0.3 * float(rr), yz], 1)
    hi_side = np.concatenate([k + 0.3 * float(rr), yz + np.asarray([0.3, -0.3]) * float(rr)], 1)
    rest = rng.uniform(0, 1, (798, 3)) * np.asarray([1000.0, 0.1, 0.1])
    box = np.concatenate([[[0, 0, 0], [1000.0, 0.1, 0.1]], np.concatenate([lo_side, hi_side, rest])[rng.permutation(1998)]]).astype(f32)
    assert (box[:, 0] >= 0).all() and (box[:, 0] <= 1000).all() and len(box) == 2000
    cases["sparse_box"] = (box, rr, None)
    bad = cloud[:900].copy()
    bad[::7, 0] = np.nan
    bad[3::11, 2] = np.inf
    bad[5::13] = -np.inf
    cases["non_finite"] = (bad, f32(0.12), None)
    cases["r=0"] = (dup, f32(0.0), 700)  # only exact duplicates go, and the first of them survives
    cases["N=1"] = (cloud[:1], f32(0.5), 1)
    cases["N=1_nan"] = (np.full((1, 3), np.nan, f32), f32(0.5), 0)
    tiny = cloud[:300] * f32(1e-10)
    cases["tiny_r"] = (np.concatenate([tiny, tiny[:100]]), f32(1e-25), 300)  # r r underflows to 0: exact duplicates only
    cases["huge_r"] = (cloud[:300] * f32(1e20), f32(3e19), None)  # r r overflows to +inf: every pair is within
    return cases


def check_icosphere_thin(sample, thin, count):
    """3 * count surface samples of the level-3 icosphere, thinned at sqrt(area / (3 count)) on the kernel's own fp32 points: the
    mask equals the greedy's, and at least `count` survive (so sample_surface_even returns exactly count rows)"""
    verts, tris = icosphere(3)
    uni = uniforms(40 + count, 3 * count)
    pts = sample(verts, tris, uni, want=("points", "face"))["points"]
    r = even_radius(verts, tris, count)
    keep = check_thin(f"icosphere_{count}", thin, pts, r)
    assert keep.sum() >= count and no_pair_within(pts[keep], r)
    np.testing.assert_array_equal(thin(pts, r), keep)  # repeatable
    return int(keep.sum())
