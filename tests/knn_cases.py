"""Shared set-up of the kNN tests.  For the model tests (tests/test_knn_model_host.py on the CPU, tests/test_gpu_knn.py on the GPU):
this repo's GaussianSplattingRenderer in the state tests/golden/make_golden_knn.py put the reference's into, and the comparisons.
For the search tests (tests/test_knn_host.py, tests/test_knn_edges_host.py on the CPU emulator, tests/test_gpu_knn_edges.py on the
GPU): the clouds that stress the index, the degenerate ones, queries that are not points of a cloud, the K values that reach every
list length, and the fp32 brute force in the kernel's formula and tie rule."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn")
FIELDS = ("mean", "qvec", "svec", "color", "alpha")
ATTR = {"mean": "mean", "qvec": "qvec", "svec": "svec_before_activation", "color": "color_before_activation",
        "alpha": "alpha_before_activation"}
PENALTIES = {  # name -> the cfg.penalty node it configures alone
    "alpha_center_weighted": {"alpha": {"type": "center_weighted", "value": 100.0}},
    "alpha_uniform_l2": {"alpha": {"type": "uniform_l2", "value": [0, 2.0, 4.0, 10]}},
    "mean_uniform_l2": {"mean": {"type": "uniform_l2", "value": 0.5}},
    "scale": {"scale": {"value": 3.0}},
    "NN": {"NN": {"value": 2.0}},
    "compat_l1": {"compat": {"type": "l1", "value": 10.0}},
    "compat_l2": {"compat": {"type": "l2", "value": [0, 1.0, 20.0, 20, "sqrt"]}},
}
PENALTY_STEP = 5
LR = dict(mean=0.005, qvec=0.003, svec=0.003, color=0.01, alpha=0.003, bg=0.003)


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def cfg(device, penalty=None, densify=None):
    return dict(device=device, svec_act="exp", alpha_act="sigmoid", color_act="sigmoid", tile_size=16, T_thresh=1e-4,
                depth_detach=True, background=dict(type="fixed", color=[0.1, 0.2, 0.3]),
                densify=densify or dict(enabled=True), prune=dict(enabled=False), penalty=penalty or {})


def model_from_raw(raw, device, penalty=None, densify=None):
    from gsgen_amd.model import GaussianSplattingRenderer
    t = {k: torch.tensor(np.ascontiguousarray(raw[k]), device=device) for k in FIELDS}
    t["raw"] = True
    return GaussianSplattingRenderer(cfg(device, penalty, densify), t)


def model_with_adam(z, device, densify=None):
    """the golden 'before' state: raw fields + one Adam step's state in every group (bg included)"""
    m = model_from_raw({k: z["before_" + k] for k in FIELDS}, device, densify=densify)
    m.setup_lr(LR)
    m.set_optimizer(dict(type="Adam", opt_args=dict(eps=1e-15)))
    params = {"bg": m.bg.bg_color, **{k: getattr(m, ATTR[k]) for k in FIELDS}}
    for name, p in params.items():
        m.optimizer.state[p] = {"step": torch.tensor(z[f"before_adam_{name}_step"]),  # (torch keeps Adam's step on the CPU)
                                **{key: torch.tensor(z[f"before_adam_{name}_{key}"], device=device) for key in ("exp_avg", "exp_avg_sq")}}
    return m


def check_after(m, z, bitwise, ref_bg=None):
    """raw fields and Adam state of the model against the golden 'after' record"""
    def eq(got, want, what):
        got = got.detach().cpu().numpy()
        assert got.shape == want.shape, (what, got.shape, want.shape)
        if bitwise:
            np.testing.assert_array_equal(got, want, err_msg=what)
        else:
            np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-6, err_msg=what)
    for k in FIELDS:
        eq(getattr(m, ATTR[k]), z["after_" + k], k)
    groups = {g["name"]: g["params"][0] for g in m.optimizer.param_groups}
    for k in FIELDS:
        assert groups[k] is getattr(m, ATTR[k]), f"optimiser group {k} does not hold the new parameter"
    for name in ("bg",) + FIELDS:
        st = m.optimizer.state[groups[name]]
        for key in ("exp_avg", "exp_avg_sq", "step"):
            eq(st[key], z[f"after_adam_{name}_{key}"], f"adam {name} {key}")


# ---- the search tests: clouds, queries, brute force -----------------------------------------------------------------------
# every list length L of knn.hip's dispatch (1, 2, 4, 8, 16, 32) and, under each L > 1, one K below it (3, 5, 9, 17, 31)
K_MATRIX = (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32)
DEGENERATE = ("same", "line", "one", "n_eq_k", "tiny")


def brute(pts, K):
    """fp32, d = p_j - p_i, dx*dx + dy*dy + dz*dz left to right; order (dist2, j); non-finite points are nobody's neighbour"""
    pts = np.asarray(pts, np.float32)
    N = pts.shape[0]
    fin = np.isfinite(pts).all(1)
    d = np.full((N, K), np.inf, np.float32)
    idx = np.full((N, K), -1, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = pts[None, :, 0] - pts[:, None, 0]
        dy = pts[None, :, 1] - pts[:, None, 1]
        dz = pts[None, :, 2] - pts[:, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(N, dtype=np.uint64)[None, :]
    key[:, ~fin] = np.iinfo(np.uint64).max
    for r in np.nonzero(fin)[0]:
        k = np.sort(key[r])[:K]
        ok = k != np.iinfo(np.uint64).max
        n = int(ok.sum())
        idx[r, :n] = (k[:n] & np.uint64(0xFFFFFFFF)).astype(np.int32)
        d[r, :n] = (k[:n] >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return d, idx


def brute_rows(pts, rows, K, chunk=32):
    """brute() for the rows `rows` of a cloud too large for an N x N table (every point finite) -> (dist2, idx) [len(rows), K]"""
    pts = np.asarray(pts, np.float32)
    j = np.arange(pts.shape[0], dtype=np.uint64)[None, :]
    out_d, out_i = [], []
    for a in range(0, len(rows), chunk):
        q = pts[rows[a:a + chunk]]
        dx = pts[None, :, 0] - q[:, None, 0]
        dy = pts[None, :, 1] - q[:, None, 1]
        dz = pts[None, :, 2] - q[:, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j
        k = np.sort(np.partition(key, K - 1, axis=1)[:, :K], axis=1)
        out_i.append((k & np.uint64(0xFFFFFFFF)).astype(np.int32))
        out_d.append((k >> np.uint64(32)).astype(np.uint32).view(np.float32))
    return np.concatenate(out_d), np.concatenate(out_i)


def n_eq_k(K, seed=23):
    """a cloud of exactly K points: every row lists the whole cloud"""
    return np.random.default_rng(seed + K).uniform(-1, 1, (K, 3)).astype(np.float32)


def clouds():
    rng = np.random.default_rng(11)
    out = {}
    out["uniform"] = rng.uniform(-1, 1, (1500, 3))
    centres = rng.normal(size=(12, 3))
    out["clustered"] = centres[rng.integers(0, 12, 1800)] + 0.01 * rng.normal(size=(1800, 3))
    base = rng.uniform(-1, 1, (600, 3))
    dup = np.concatenate([base, base[rng.integers(0, 600, 400)], base[:50]])  # exact duplicates, some three times
    out["duplicates"] = dup[rng.permutation(dup.shape[0])]
    flat = rng.uniform(-1, 1, (1500, 3))
    flat[:, 2] = 0.25
    out["planar"] = flat
    core = rng.normal(size=(1800, 3)) * 0.5
    far = rng.normal(size=(40, 3))
    out["outliers"] = np.concatenate([core, 100.0 * far / np.linalg.norm(far, axis=1, keepdims=True)])
    nanc = rng.uniform(-1, 1, (1200, 3))
    nanc[rng.integers(0, 1200, 30), rng.integers(0, 3, 30)] = np.nan
    nanc[5, 1] = np.inf
    nanc[17] = -np.inf
    out["nan_rows"] = nanc
    out["offset"] = rng.uniform(-1, 1, (800, 3)) * 1e-3 + np.array([1000.0, -2000.0, 500.0])  # far from the origin, fine spacing
    return {k: v.astype(np.float32) for k, v in out.items()}


def edge_clouds():
    """the degenerate extents (a generator of their own: clouds() keeps its draws) and the cloud of few distinct positions"""
    rng = np.random.default_rng(29)
    out = {}
    out["same"] = np.tile(np.array([[0.3, -1.7, 2.5]]), (40, 1))  # emax == 0: one cell
    line = np.zeros((300, 3))
    line[:, 0] = rng.uniform(-2, 3, 300)  # two zero extents: the kMaxDim clamp on the third
    out["line"] = line
    out["one"] = np.array([[0.5, 0.25, -4.0]])
    out["n_eq_k"] = n_eq_k(4)
    out["tiny"] = rng.uniform(-1, 1, (37, 3))  # N < 64: less than a wavefront, 18 cells
    pos = rng.uniform(-1, 1, (50, 3))
    out["few_distinct"] = pos[np.concatenate([np.arange(50), rng.integers(0, 50, 1950)])][rng.permutation(2000)]
    return {k: v.astype(np.float32) for k, v in out.items()}


def scan_cloud(N, seed=31):
    """a uniform cloud for the scan boundaries: with K = 2 the index has N / 2 cells and scans N / 2 + 3 entries"""
    return np.random.default_rng(seed + N).uniform(-1, 1, (N, 3)).astype(np.float32)


SCAN_SMALL = (2042, 2044)          # cap + 3 = 1024 (one full scan tile) and 1025 (a second tile of one entry)
SCAN_LARGE = 2 * 262144 + 40       # cap + 3 = 262 167: T = 257 scan tiles, k_knn_scan_sums' second chunk of 256


def queries_for(pts, n=512, seed=0):
    """n queries that are not points of the cloud: half jittered points (1e-3 of the radius), a quarter uniform in 1.1 x the
    bounding box, a quarter at 3 .. 100 x the radius in random directions (the radius: the 98 % quantile of the distance to the
    median, so far outliers do not set it; 1 where the cloud has no extent) -> [n, 3] float32, shuffled"""
    rng = np.random.default_rng(1000 + seed)
    fin = np.asarray(pts, np.float32)
    fin = fin[np.isfinite(fin).all(1)].astype(np.float64)
    med = np.median(fin, axis=0)
    r = float(np.quantile(np.linalg.norm(fin - med, axis=1), 0.98))
    r = r if r > 0 else 1.0
    jit = fin[rng.integers(0, fin.shape[0], n // 2)] + 1e-3 * r * rng.normal(size=(n // 2, 3))
    lo, hi = fin.min(0), fin.max(0)
    uni = (lo + hi) / 2 + rng.uniform(-1, 1, (n // 4, 3)) * (hi - lo) / 2 * 1.1
    d = rng.normal(size=(n - n // 2 - n // 4, 3))
    far = med + d / np.linalg.norm(d, axis=1, keepdims=True) * r * np.exp(rng.uniform(np.log(3.0), np.log(100.0), (d.shape[0], 1)))
    q = np.concatenate([jit, uni, far]).astype(np.float32)
    return q[rng.permutation(q.shape[0])]


CLOUDS = {**clouds(), **edge_clouds()}
QUERIES = {name: queries_for(p, seed=n) for n, (name, p) in enumerate(sorted(CLOUDS.items()))}
_BRUTE = {}


def brute_self(name):
    """the brute force of a cloud's self search at K = min(32, N), computed once (its first K columns are the K search)"""
    if ("self", name) not in _BRUTE:
        _BRUTE["self", name] = brute(CLOUDS[name], min(32, CLOUDS[name].shape[0]))
    return _BRUTE["self", name]


def brute_queries(name):
    """the same for the cloud's queries (density_cases.brute_query: d = p_j - q)"""
    if ("query", name) not in _BRUTE:
        import density_cases as DC
        _BRUTE["query", name] = DC.brute_query(CLOUDS[name], QUERIES[name], min(32, CLOUDS[name].shape[0]))
    return _BRUTE["query", name]


def same_bits(d, i, bd, bi, what):
    """identical indices and identical dist2 bits"""
    np.testing.assert_array_equal(i, bi, err_msg=f"{what}: idx")
    np.testing.assert_array_equal(np.ascontiguousarray(d).view(np.uint32), np.ascontiguousarray(bd).view(np.uint32), err_msg=f"{what}: dist2")


def no_exact_duplicates(pts):
    """True when no two rows of pts [N,3] float32 are equal (the (x, y) bit pairs first: they are almost always distinct already)"""
    b = np.ascontiguousarray(pts, np.float32).view(np.uint32).astype(np.uint64)
    if np.unique((b[:, 0] << np.uint64(32)) | b[:, 1]).size == b.shape[0]:
        return True
    return np.unique(pts, axis=0).shape[0] == pts.shape[0]


def check_whole_array(pts, d, i):
    """what must hold in every row of a self search on a finite cloud without exact duplicates: indices in [0, N), the point
    itself first, distances ascending"""
    N = pts.shape[0]
    assert i.min() >= 0 and i.max() < N
    np.testing.assert_array_equal(i[:, 0], np.arange(N, dtype=i.dtype))
    assert (d[:, 0] == 0).all() and (np.diff(d, axis=1) >= 0).all()


# ---- the density lattice at every list length ---------------------------------------------------------------------------
# (K, skip_nearest): K + skip = 1, 2, 2, 9, 16, 17, 32, 32 -> k_density_grid<1>, <2>, <2>, <16>, <16>, <32>, <32>, <32>
DENSITY_KS = ((1, 0), (1, 1), (2, 0), (9, 0), (15, 1), (16, 1), (31, 1), (32, 0))
DENSITY_SHAPES = ((5, 6, 7), (1, 1, 1), (4, 4, 9))  # no multiple of the 4 x 4 x 4 brick but one axis of the last; a single point


def density_axes(g, shape, seed=41):
    """three different axes for a lattice of `shape` on the Gaussians g (density_cases.load_golden()): coordinate k of axis a is
    that of a Gaussian n_k (one list n for the three axes) moved by a tenth of its smallest scale, and n is drawn from the Gaussians
    at whose centre the nearest OTHER Gaussian has a density above 0.05: lattice point (k, k, k) has mass with the nearest dropped
    and without, and the other points are wherever the product puts them (most in empty space) -> (ax, ay, az)"""
    import density_cases as DC
    rng = np.random.default_rng(seed + sum(shape))
    _, nn = DC.brute_query(g["mean"], g["mean"], 2)
    at_centre, _ = DC.density64(g["mean"], g["qvec"], g["scale"], g["opacity"], g["mean"], nn[:, 1:2])
    n = rng.choice(np.nonzero(at_centre > 0.05)[0], max(shape), replace=False)
    off = g["scale"][n].min(1)[:, None] / 10 * rng.choice([-1.0, 1.0], (max(shape), 3))
    p = (g["mean"][n] + off).astype(np.float32)
    return tuple(np.ascontiguousarray(p[:shape[a], a]) for a in range(3))
