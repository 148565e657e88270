"""The clouds and the fp32 NumPy reference of the farthest point sampling tests (tests/test_fps_host.py, tests/test_gpu_fps.py).

The rule (gsgen_amd/csrc/fps.hip): idx[0] = s0 (the lowest-index finite point when s0 is out of range or not finite); m = +inf;
after pick s, m[p] = min(m[p], d2(p, s)), d2 = the sum over the coordinates of (p_c - s_c)^2, left to right in fp32; the next pick
maximises the key float_bits(m) << 32 | (0xFFFFFFFF - index).  Non-finite rows and rows past `length` are never picked; entries
past the number of pickable points are -1."""
import functools

import numpy as np


def fps_reference(points, K, s0, length=None):
    pts = np.asarray(points, np.float32)
    L, D = pts.shape
    n = L if length is None else max(0, min(int(length), L))
    ok = np.isfinite(pts).all(1)
    ok[n:] = False
    idx = np.full(K, -1, np.int32)
    if not ok.any():
        return idx
    if not (0 <= s0 < n and ok[s0]):
        s0 = int(np.nonzero(ok)[0][0])
    low = (np.uint64(0xFFFFFFFF) - np.arange(L, dtype=np.uint64))
    m = np.full(L, np.inf, np.float32)
    npick = min(K, int(ok.sum()))
    cur = int(s0)
    for k in range(npick):
        idx[k] = cur
        if k + 1 == npick:
            break
        with np.errstate(invalid="ignore", over="ignore"):
            d = pts - pts[cur]
            d2 = d[:, 0] * d[:, 0]
            for c in range(1, D):
                d2 = d2 + d[:, c] * d[:, c]
            m = np.minimum(m, d2)
        assert m.dtype == np.float32
        key = (m.view(np.uint32).astype(np.uint64) << np.uint64(32)) | low
        key[~ok] = 0
        cur = int(np.argmax(key))
    return idx


def _clouds():
    rng = np.random.default_rng(23)
    out = {}
    out["uniform"] = (rng.uniform(-1, 1, (3000, 3)), 1234)
    centres = rng.normal(size=(12, 3))
    out["clustered"] = (centres[rng.integers(0, 12, 2500)] + 0.01 * rng.normal(size=(2500, 3)), 7)
    flat = rng.uniform(-1, 1, (2000, 3))
    flat[:, 2] = 0.25
    out["planar"] = (flat, 1999)
    out["identical"] = (np.tile(np.array([[0.3, -1.7, 2.5]]), (700, 1)), 350)
    base = rng.uniform(-1, 1, (600, 3))
    dup = np.concatenate([base, base[rng.integers(0, 600, 400)], base[:50]])  # exact duplicates, some three times
    out["duplicates"] = (dup[rng.permutation(dup.shape[0])], 3)
    g = np.arange(12, dtype=np.float64)
    out["lattice"] = (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3), 5 * 144 + 6 * 12 + 5)  # massive exact ties
    core = centres[rng.integers(0, 12, 2400)] + 0.01 * rng.normal(size=(2400, 3))
    far = rng.normal(size=(24, 3))
    radius = np.linalg.norm(core, axis=1).max()
    both = np.concatenate([core, 100.0 * radius * far / np.linalg.norm(far, axis=1, keepdims=True)])  # 1 % outliers at 100 x radius
    out["outliers"] = (both[rng.permutation(both.shape[0])], 11)
    nanc = rng.uniform(-1, 1, (1500, 3))
    nanc[rng.integers(2, 1500, 40), rng.integers(0, 3, 40)] = np.nan
    nanc[0, 2] = np.nan      # index 0 ...
    nanc[77] = -np.inf       # ... and the given start are not finite: the start falls back to index 1
    nanc[5, 1] = np.inf
    nanc[1] = [0.1, 0.2, 0.3]
    out["nan_rows"] = (nanc, 77)
    out["offset"] = (rng.uniform(-1, 1, (1200, 3)) * 1e-3 + np.array([1000.0, -2000.0, 500.0]), 600)  # exercises the pruning margins
    huge = rng.uniform(-1, 1, (600, 3))
    huge[::2] *= 1e20        # d2 overflows to +inf; no NaN may appear
    out["huge"] = (huge, 2)
    return {k: (np.ascontiguousarray(v, np.float32), s) for k, (v, s) in out.items()}


CLOUDS = _clouds()
NAMES = sorted(CLOUDS)


def with_rgb(name):
    """the cloud as [L, 6]: xyz + a colour per point (forward_image samples xyz + rgb)"""
    pts, s0 = CLOUDS[name]
    rng = np.random.default_rng(len(name) + pts.shape[0])
    rgb = rng.uniform(0, 1, (pts.shape[0], 3)).astype(np.float32)
    if name == "nan_rows":
        rgb[9, 1] = np.nan
    if name in ("identical", "lattice"):
        rgb[:] = 0.5  # (keep the exact ties)
    return np.ascontiguousarray(np.concatenate([pts, rgb], 1)), s0


@functools.lru_cache(maxsize=None)
def reference(name, K, dim=3):
    """computed once per (cloud, K, dim) and shared; callers must not write to it"""
    pts, s0 = CLOUDS[name] if dim == 3 else with_rgb(name)
    r = fps_reference(pts, K, s0)
    r.setflags(write=False)
    return r
