"""Milliseconds of gsgen_amd.mesh_sample.sample_surface_even (gsgen_amd/csrc/mesh_sample.hip) and of its parts, on the mesh
density_mesh makes from the bench cloud and on a subdivided icosphere of 81 920 faces; prints ONE JSON line.

    python tools/bench_mesh_sample.py [--count 100000] [--iters 10] [--warmup 2] [--reso 128] [--time-limit 300]

Per mesh, with 3 * count samples and radius = sqrt(area / (3 count)), each between two events on one stream in a window of
at least 0.2 s, allocations included:
"ms_sample" (gsgen_mesh_sample: weights, scan, samples), "ms_grid" (gsgen_remove_close_init: box, grid, counting sort, state),
"ms_rounds" (the rounds in groups of 8 with a host read of the undecided count after each group, as remove_close runs them;
"rounds": how many a run with a read after EVERY round needed), "ms_total" (sample_surface_even itself, the host read of the area
included), "kept" (rows that survive; the call returns min(kept, count)).  "ms_ckdtree": trimesh's remove_close loop on scipy's
cKDTree on the host over the same points (copy from the device included), when scipy imports; "mask_differs": entries where its
fp64 mask and the device's fp32 one differ.  The process ends itself after --time-limit seconds.  The figures go into DESIGN.md
("Mesh sampling").
"""
import argparse
import json
import math
import os
import signal
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


MIN_WINDOW_MS = 200.0  # a timed window shorter than this measures the clock and the scheduler as much as the kernels


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def timed(fn, iters, warmup):
    """ms per call: warm-up, then one window of at least `iters` calls and at least MIN_WINDOW_MS (sized from a first window)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    first = window(fn, iters)
    return window(fn, max(iters, int(MIN_WINDOW_MS / max(first, 1e-3)) + 1))


def ckdtree_remove_close(points, radius):
    """trimesh.points.remove_close, restated"""
    from scipy.spatial import cKDTree
    tree = cKDTree(points)
    consumed, unique = np.zeros(len(points), bool), np.zeros(len(points), bool)
    for i, nbrs in enumerate(tree.query_ball_point(points, radius)):
        if consumed[i]:
            continue
        unique[i] = True
        consumed[nbrs] = True
    return unique


def bench_mesh(name, verts, tris, count, iters, warmup):
    from gsgen_amd import _capi
    from gsgen_amd import mesh_sample as GS
    lib = _capi.load()
    dev = verts.device
    verts, tris = GS._mesh(verts, tris)
    N = 3 * count
    uni = torch.rand(N, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    area = float(GS.mesh_area(verts, tris))
    radius = math.sqrt(area / N)
    pts = GS._sample_raw(verts, tris, uni)["points"]
    stream = torch.cuda.current_stream(dev).cuda_stream
    nbytes = lib.remove_close_workspace_bytes(N)
    st = {}

    def grid():
        st["keep"] = torch.empty(N, device=dev, dtype=torch.uint8)
        st["ws"] = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        st["left"] = torch.empty(1, device=dev, dtype=torch.int32)
        lib.remove_close_init(pts.data_ptr(), N, radius, st["keep"].data_ptr(), st["ws"].data_ptr(), nbytes, stream)

    def rounds(group):
        n = 0
        while True:
            lib.remove_close_rounds(group, N, radius, st["keep"].data_ptr(), st["left"].data_ptr(), st["ws"].data_ptr(), nbytes, stream)
            n += group
            if int(st["left"].item()) == 0:
                return n

    def grid_and_rounds():
        grid()
        rounds(GS.ROUND_GROUP)
    grid()
    n_rounds = rounds(1)  # (the round after which nothing was undecided, counted from 1)
    keep = st["keep"].bool()
    res = {"mesh": name, "V": int(verts.shape[0]), "F": int(tris.shape[0]), "count": count, "samples": N, "area": round(area, 6),
           "radius": radius, "rounds": n_rounds, "kept": int(keep.sum())}
    res["ms_sample"] = round(timed(lambda: GS._sample_raw(verts, tris, uni), iters, warmup), 4)
    res["ms_grid"] = round(timed(grid, iters, warmup), 4)
    res["ms_grid_and_rounds"] = round(timed(grid_and_rounds, iters, warmup), 4)
    res["ms_rounds"] = round(res["ms_grid_and_rounds"] - res["ms_grid"], 4)
    gen = torch.Generator(device=dev).manual_seed(2)
    res["ms_total"] = round(timed(lambda: GS.sample_surface_even(verts, tris, count, generator=gen), iters, warmup), 4)
    try:
        import scipy  # noqa: F401
        t0 = time.perf_counter()
        host = ckdtree_remove_close(pts.cpu().numpy().astype(np.float64), radius)
        res["ms_ckdtree"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["mask_differs"] = int((host != keep.cpu().numpy()).sum())
    except ImportError:
        res["ms_ckdtree"] = None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=100000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reso", type=int, default=128)
    ap.add_argument("--time-limit", type=int, default=300)
    args = ap.parse_args()
    signal.alarm(args.time_limit)  # (SIGALRM's default action ends the process)
    assert torch.cuda.is_available(), "bench_mesh_sample needs a GPU"
    import bench
    import mesh_sample_cases as MC
    from gsgen_amd import _capi
    from gsgen_amd.mesh import density_mesh
    dev = torch.device("cuda")
    sc, _, _ = bench.make_workload("cfg2")
    mean, qvec, scale = (torch.tensor(sc[k], device=dev, dtype=torch.float32) for k in ("mean", "qvec", "svec"))
    opacity = torch.full((mean.shape[0],), 0.5, device=dev)
    L = mean.abs().max().item() * 1.1
    cloud_mesh = density_mesh(mean, qvec, scale, opacity, L, args.reso, 3, 0.5, True)
    iv, it = MC.icosphere(6)
    meshes = [("bench_cloud_reso%d" % args.reso, *cloud_mesh), ("icosphere6", torch.tensor(iv, device=dev), torch.tensor(it, device=dev))]
    res = {"tool": "bench_mesh_sample", "iters": args.iters, "warmup": args.warmup, "lib": _capi.load().path,
           "device": torch.cuda.get_device_name(0),
           "meshes": [bench_mesh(n, v, t, args.count, args.iters, args.warmup) for n, v, t in meshes]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
