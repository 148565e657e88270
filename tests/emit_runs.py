"""Shared cases of tests/test_emit_runs_host.py (CPU emulator) and tests/test_gpu_emit_runs.py (MI355X): the emit pass of the push
binning groups a 2 048-Gaussian chunk's keys by tile in LDS and stores them in runs (gsgen_amd/csrc/binning.hip, bin_push_body).
Every case compares gaussian_ids, start, end and total of gsgen_frame_geometry and gsgen_frame_geometry_batch with the oracle's,
bit for bit.  A backend says where the arrays live (numpy for the emulator, torch on the GPU)."""
import numpy as np

import scenes

CHUNK = 2048
SIZES = [1, 511, 512, 513, 2047, 2048, 2049, 4097]         # the workgroup stride (512 threads) and the chunk (2 048 Gaussians)
IMAGES = [(16, 16), (17, 33), (40, 24), (200, 120)]        # one tile; partial edge tiles; 3 x 2; 13 x 8 tiles


class HostBackend:
    """the emulator works on host memory"""
    stream = None

    def __init__(self, lib):
        self.lib = lib

    def put(self, a):
        return np.ascontiguousarray(a).copy()

    def full(self, shape, dtype, value):
        return np.full(shape, value, dtype)

    def ptr(self, a):
        return a.ctypes.data

    def get(self, a):
        return a

    def sync(self):
        pass


class GpuBackend:
    def __init__(self, lib):
        import torch
        self.lib, self.torch, self.dev = lib, torch, torch.device("cuda:0")
        self.stream = torch.cuda.current_stream().cuda_stream

    def put(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def full(self, shape, dtype, value):
        return self.put(np.full(shape, value, dtype))

    def ptr(self, a):
        return a.data_ptr()

    def get(self, a):
        return a.cpu().numpy()

    def sync(self):
        self.torch.cuda.synchronize()


# ---- scenes with rectangles under control ------------------------------------------------------------------------------------
def front_camera(W, H):
    return scenes.Camera(W, H, fx=float(max(W, H)))


def splats_at(cam, uv, depth, svec, seed=0):
    """Gaussians whose centres project to the pixels `uv` [n, 2] at camera depth `depth` [n], isotropic scale `svec` [n]"""
    uv, depth, svec = np.asarray(uv, np.float64), np.asarray(depth, np.float64), np.asarray(svec, np.float64)
    n = uv.shape[0]
    x, y, z, pos = (cam.c2w[:, k].astype(np.float64) for k in range(4))
    mean = (pos[None] + z[None] * depth[:, None] + x[None] * ((uv[:, 0] - cam.cx) / cam.fx * depth)[:, None]
            + y[None] * ((uv[:, 1] - cam.cy) / cam.fy * depth)[:, None])
    sc = scenes.random_scene(n, seed=seed)
    sc["mean"] = mean.astype(np.float32)
    sc["qvec"] = np.tile(np.array([1.0, 0, 0, 0], np.float32), (n, 1))
    sc["svec"] = np.repeat(svec.astype(np.float32)[:, None], 3, 1)
    return sc


def tile_centres(cam, tiles):
    nth, ntw = cam.tiles
    tiles = np.asarray(tiles)
    u = np.minimum((tiles % ntw) * 16 + 8, ((tiles % ntw) * 16 + cam.w) / 2.0)   # (inside the image also in a partial edge tile)
    v = np.minimum((tiles // ntw) * 16 + 8, ((tiles // ntw) * 16 + cam.h) / 2.0)
    return np.stack([u, v], 1)


BIG, SMALL = 40.0, 2e-4   # a splat over the whole image / inside one tile (checked against the oracle's rectangles by the callers)


def cover_scene(cam, n_big, small_tiles, seed=0):
    """n_big splats that cover every tile, then one one-tile splat per entry of small_tiles; depths all different, in no order"""
    n = n_big + len(small_tiles)
    rng = np.random.default_rng(seed)
    uv = np.concatenate([np.tile([[cam.w / 2.0, cam.h / 2.0]], (n_big, 1)), tile_centres(cam, small_tiles).reshape(-1, 2)])
    depth = rng.permutation(n) / max(n, 1) * 0.5 + 2.25
    svec = np.concatenate([np.full(n_big, BIG), np.full(len(small_tiles), SMALL)])
    order = rng.permutation(n)       # big and small ones interleaved: both walks of a workgroup stage into the same runs
    sc = splats_at(cam, uv[order], depth[order], svec[order], seed)
    return sc


def chunk_key_counts(g, N):
    """keys per 2 048-Gaussian chunk, from the oracle's rectangles (all Gaussians visible: chunk = index // 2 048)"""
    assert g["mask"].all()
    per = (g["br"] - g["tl"] + 1).clip(min=0).prod(-1)
    return [int(per[c:c + CHUNK].sum()) for c in range(0, N, CHUNK)]


def expected_staged_keys(g, N, cam, capacity):
    """how many keys of one frame go through the staging array: per chunk, the leading tiles whose keys fit (the cumulative
    count over the tiles stays within the capacity), from the oracle's rectangles (all Gaussians visible)"""
    assert g["mask"].all()
    nth, ntw = cam.tiles
    total = 0
    for c in range(0, N, CHUNK):
        cnt = np.zeros((nth, ntw), np.int64)
        for (x0, y0), (x1, y1) in zip(g["tl"][c:c + CHUNK], g["br"][c:c + CHUNK]):
            cnt[max(y0, 0):min(y1, nth - 1) + 1, max(x0, 0):min(x1, ntw - 1) + 1] += 1
        ends = np.cumsum(cnt.ravel())
        fit = ends[ends <= capacity]
        total += int(fit[-1]) if len(fit) else 0
    return total


# ---- running the two entry points -------------------------------------------------------------------------------------------
def _al(n):
    return (n + 255) // 256 * 256


def keys_region(N, cap, T):
    """byte range of the binning keys inside a gsgen_frame_workspace_bytes workspace (binning.hip: carve)"""
    nchunks = max((N + CHUNK - 1) // CHUNK, 1)
    b = _al(4 * (T + 4)) + _al(4 * (T + 1)) + _al(4 * max(T, 1)) + _al(4 * nchunks * T) + _al(4 * nchunks * 4 * T)
    return b, b + 8 * max(cap, 1)


def _buffers(be, N, T, cap):
    r = dict(m2=be.full((N, 2), np.float32, 0), c2=be.full((N, 4), np.float32, 0), dep=be.full(N, np.float32, 0),
             mask=be.full(N, np.uint8, 0), ids=be.full(max(cap, 1), np.int32, -7), st=be.full(T, np.int32, 0),
             en=be.full(T, np.int32, 0), tot=be.full(1, np.uint32, 0),
             ws=be.full(be.lib.frame_workspace_bytes(N, cap, T), np.uint8, 0xAB))
    r["cap"] = cap
    return r


def _check(be, r, g, N, T, what):
    cap, D = r["cap"], g["D"]
    assert int(be.get(r["tot"])[0]) == D, what
    st, en, ids = be.get(r["st"]).ravel(), be.get(r["en"]).ravel(), be.get(r["ids"])
    if cap >= D:
        full = np.nonzero(g["mask"])[0]
        assert np.array_equal(st, g["start"]) and np.array_equal(en, g["end"]), what
        assert np.array_equal(ids[:D], full[g["ids"]]), what
        assert (ids[D:] == -7).all(), what
        b, e = keys_region(N, cap, T)   # ... and the keys lie where keys_region() says: every one of the D written
        assert (np.ascontiguousarray(be.get(r["ws"])[b:b + 8 * D]).view(np.uint64) != 0xABABABABABABABAB).all(), what
    else:   # overflow: reported, every tile marked GSGEN_LIST_OVERFLOW, and NOTHING written: neither a list entry nor a key
        assert (st == -2).all() and (en == -2).all(), what
        assert (ids == -7).all(), what
        b, e = keys_region(N, cap, T)
        assert (be.get(r["ws"])[b:e] == 0xAB).all(), what


def run_single(be, sc, cam, g, cap=None):
    from gsgen_amd import renderer as R
    lib, p = be.lib, be.ptr
    N = sc["mean"].shape[0]
    nth, ntw = cam.tiles
    T = nth * ntw
    mean, qvec, svec = be.put(sc["mean"]), be.put(sc["qvec"]), be.put(sc["svec"])
    camv = be.put(R.CameraInfo(*cam.intr).pack(cam.c2w))
    r = _buffers(be, N, T, g["D"] + 3 if cap is None else cap)
    lib.frame_geometry(N, p(mean), p(qvec), p(svec), p(camv), cam.w, cam.h, r["cap"], p(r["m2"]), p(r["c2"]), p(r["dep"]),
                       p(r["mask"]), p(r["ids"]), p(r["st"]), p(r["en"]), p(r["tot"]), p(r["ws"]), r["ws"].shape[0], be.stream)
    be.sync()
    _check(be, r, g, N, T, "frame_geometry")


def run_batch(be, sc, cams, gs_, caps=None):
    """cams / gs_: the views of the batch (the same camera may appear several times, with its one oracle result)"""
    from gsgen_amd import renderer as R
    from gsgen_amd._capi import GeometryView
    lib, p = be.lib, be.ptr
    N, B = sc["mean"].shape[0], len(cams)
    nth, ntw = cams[0].tiles
    T = nth * ntw
    mean, qvec, svec = be.put(sc["mean"]), be.put(sc["qvec"]), be.put(sc["svec"])
    camv = [be.put(R.CameraInfo(*c.intr).pack(c.c2w)) for c in cams]
    caps = caps or [g["D"] + 3 for g in gs_]
    rs = [_buffers(be, N, T, cap) for cap in caps]
    arr = (GeometryView * B)()
    for a, cv, r in zip(arr, camv, rs):
        a.cam, a.mean2d, a.cov2d, a.depth, a.mask = p(cv), p(r["m2"]), p(r["c2"]), p(r["dep"]), p(r["mask"])
        a.gaussian_ids, a.start, a.end, a.total = p(r["ids"]), p(r["st"]), p(r["en"]), p(r["tot"])
        a.workspace, a.workspace_bytes, a.D_cap = p(r["ws"]), r["ws"].shape[0], r["cap"]
    bws = be.full(lib.frame_batch_workspace_bytes(B), np.uint8, 0)
    lib.frame_geometry_batch(B, arr, N, p(mean), p(qvec), p(svec), cams[0].w, cams[0].h, p(bws), be.stream)
    be.sync()
    for v, (r, g) in enumerate(zip(rs, gs_)):
        _check(be, r, g, N, T, f"frame_geometry_batch view {v} of {B}")


def three_cameras(W, H):
    f = float(max(W, H))
    return [scenes.Camera(W, H, fx=f * (1.0 + 0.1 * i), c2w=scenes.orbit(2.3 + 0.1 * i, 25 - 12 * i, 40.0 + 100 * i)) for i in range(3)]


def views_for_push(cams, gs_, N, min_workgroups):
    """the three cameras repeated until (chunks x views) reaches the batched push form's threshold"""
    nchunks = max((N + CHUNK - 1) // CHUNK, 1)
    B = max(len(cams), -(-min_workgroups // nchunks))
    idx = [i % len(cams) for i in range(B)]
    return [cams[i] for i in idx], [gs_[i] for i in idx]


# ---- the cases (min_workgroups: 1 on the emulator, where the test sets the knob; 32 on the GPU: the library's own threshold) --
def case_sizes(be, W, H, N, min_workgroups):
    sc = scenes.random_scene(N, seed=N + W, svec=0.05, spread=0.6)
    cams = three_cameras(W, H)
    gs_ = [scenes.oracle_geometry(sc, c) for c in cams]
    assert sum(g["D"] for g in gs_) > 0
    run_single(be, sc, cams[0], gs_[0])
    run_batch(be, sc, *views_for_push(cams, gs_, N, min_workgroups))


def case_mixed(be, min_workgroups):
    """one splat over every tile among hundreds of one-tile splats: the per-thread walk and the wave-cooperative walk of a big
    rectangle stage into the same runs"""
    cam = front_camera(200, 120)
    T = cam.tiles[0] * cam.tiles[1]
    rng = np.random.default_rng(5)
    sc = cover_scene(cam, 1, rng.integers(0, T, 700), seed=5)
    N = 701
    g = scenes.oracle_geometry(sc, cam)
    per = (g["br"] - g["tl"] + 1).clip(min=0).prod(-1)
    assert g["mask"].all() and (per == T).sum() == 1 and (per == 1).sum() == 700 and g["D"] == T + 700
    run_single(be, sc, cam, g)
    run_batch(be, sc, *views_for_push([cam], [g], N, min_workgroups))


def capacity_scene(cam, K):
    """one chunk of K keys on the 8 x 8 tiles of a 128 x 128 image: K // 64 image-sized splats and K % 64 one-tile ones (tiles
    5, 6, ...: the chunk's layout runs past the capacity in the middle of the tile range)"""
    T = 64
    return cover_scene(cam, K // T, (np.arange(K % T) + 5) % T, seed=K)


def case_capacity(be, K, min_workgroups, which=("single", "batch")):
    cam = front_camera(128, 128)
    assert cam.tiles == (8, 8)
    sc = capacity_scene(cam, K)
    N = sc["mean"].shape[0]
    assert N <= CHUNK
    g = scenes.oracle_geometry(sc, cam)
    assert chunk_key_counts(g, N) == [K] and g["D"] == K
    if "single" in which:
        run_single(be, sc, cam, g)
    if "batch" in which:
        run_batch(be, sc, *views_for_push([cam], [g], N, min_workgroups))


def case_empty_view(be, N):
    """a batch of three different cameras, the middle one looking away from the scene: no visible Gaussian, every list empty"""
    W, H = 40, 24
    sc = scenes.random_scene(N, seed=3, svec=0.02, spread=0.5)
    cams = three_cameras(W, H)
    cams[1] = scenes.Camera(W, H, fx=40.0, c2w=scenes.look_at((2.5, 0.0, 0.0), at=(9.0, 0.0, 0.0)))
    gs_ = [scenes.oracle_geometry(sc, c) for c in cams]
    assert gs_[1]["D"] == 0 and not gs_[1]["mask"].any() and gs_[0]["D"] > 0 and gs_[2]["D"] > 0
    run_batch(be, sc, cams, gs_)


def case_single_view(be, N, single):
    """B = 1, and (single) the per-camera entry point in its push form"""
    cam = three_cameras(200, 120)[0]
    sc = scenes.random_scene(N, seed=8, svec=0.004, spread=0.6)
    g = scenes.oracle_geometry(sc, cam)
    assert g["D"] > N // 4
    run_batch(be, sc, [cam], [g])
    if single:
        run_single(be, sc, cam, g)


def case_overflow(be, N, min_workgroups):
    """a frame whose pairs do not fit D_cap reports its count and writes nothing; its neighbours in the batch are binned"""
    W, H = 40, 24
    sc = scenes.random_scene(N, seed=21, svec=0.05, spread=0.6)
    cams = three_cameras(W, H)
    gs_ = [scenes.oracle_geometry(sc, c) for c in cams]
    assert min(g["D"] for g in gs_) > 10
    run_single(be, sc, cams[0], gs_[0], cap=gs_[0]["D"] - 1)
    vc, vg = views_for_push(cams, gs_, N, min_workgroups)
    caps = [g["D"] + 3 for g in vg]
    caps[1] = vg[1]["D"] - 1
    caps[-1] = 1
    run_batch(be, sc, vc, vg, caps)
