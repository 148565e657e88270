"""Milliseconds per marching cubes call (gsgen_amd/csrc/marching_cubes.hip) on the density lattice of the bench cloud; prints ONE
JSON line.

    python tools/bench_mesh.py [--iters 20] [--warmup 3] [--resos 128,256,512] [--thresh 0.5]

Per resolution: the density lattice of bench's cfg2 cloud (gsgen_amd.density.density_grid, K = 3, opacity 0.5 -- the lattice of
tools/bench_knn.py) is made once; then gsgen_amd.mesh.marching_cubes_into is timed between two events on one stream, into buffers
of the exact size ("emit": count + scans + emit, what marching_cubes runs second) and with no buffers ("count": what it runs
first).  Beside the times: V, F, the bytes the call must move at least -- read the lattice once, write the vertices and triangles:
4 X Y Z + 12 V + 12 F -- and the rate that floor is of the emit time.  The rate is end to end: it includes the five launches and
the workspace allocation, and the kernels move more than the floor (a classification reads each of the four lattice rows a tile's
cubes touch, and 4 bytes per point of offsets go through the workspace in tiles that have a vertex).  No threshold is fixed here; the figures go into
DESIGN.md ("Marching cubes").
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--resos", default="128,256,512")
    ap.add_argument("--thresh", type=float, default=0.5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mesh needs a GPU"
    import bench
    from gsgen_amd import _capi
    from gsgen_amd.density import density_grid
    from gsgen_amd.mesh import marching_cubes, marching_cubes_into
    dev = torch.device("cuda")
    sc, _, _ = bench.make_workload("cfg2")
    mean, qvec, scale = (torch.tensor(sc[k], device=dev, dtype=torch.float32) for k in ("mean", "qvec", "svec"))
    opacity = torch.full((mean.shape[0],), 0.5, device=dev)
    L = mean.abs().max().item() * 1.1
    res = {"tool": "bench_mesh", "iters": args.iters, "warmup": args.warmup, "thresh": args.thresh, "lib": _capi.load().path,
           "n_gaussians": int(mean.shape[0]), "resos": {}}
    for reso in (int(r) for r in args.resos.split(",")):
        grid = density_grid(mean, qvec, scale, opacity, L, reso, 3)
        verts, tris = marching_cubes(grid, args.thresh)
        V, F = verts.shape[0], tris.shape[0]
        counts = torch.zeros(3, device=dev, dtype=torch.int32)
        ms_emit = timed(lambda: marching_cubes_into(grid, args.thresh, verts, tris, counts), args.iters, args.warmup)
        assert counts.tolist() == [V, F, 0]
        ms_count = timed(lambda: marching_cubes_into(grid, args.thresh, None, None, counts), args.iters, args.warmup)
        floor = 4 * reso ** 3 + 12 * V + 12 * F
        res["resos"][str(reso)] = {"V": V, "F": F, "ms_emit": round(ms_emit, 4), "ms_count": round(ms_count, 4), "bytes_floor": floor,
                                   "emit_GBps_of_floor": round(floor / (ms_emit * 1e-3) / 1e9, 1)}
        del grid, verts, tris
        torch.cuda.empty_cache()
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
