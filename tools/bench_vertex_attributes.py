"""Milliseconds per gsgen_amd.mesh.vertex_attributes call (k_density_points, gsgen_amd/csrc/knn.hip) on the reso-128 mesh of the
bench cloud, against the route to the same numbers without the fused kernel; prints ONE JSON line.

    python tools/bench_vertex_attributes.py [--iters 20] [--warmup 3] [--reso 128] [--K 3] [--time-limit 240]

The mesh: bench's cfg2 cloud, opacity 0.5 (the lattice of tools/bench_mesh.py), density_mesh at K (the nearest dropped, the
reference's field), colours uniform in [0, 1].  "fused": vertex_attributes -- k_density_prep, the index, one k_density_points
launch, the normalisation in torch.  "torch": gsgen_amd.knn.knn_raw(mean, K + 1, query=verts) -- the same index and search, writing
the [V, K + 1] index and distance arrays -- then torch gathers and the closed-form expressions (Sigma^-1 from the quaternions, the
quadratic form, the weighted sums, the same normalisation).  Both between two events on one stream, allocations included.  The two
results are compared (max abs difference of normals and colours) so that the comparison is of equal work.  The process ends itself
after --time-limit seconds.  The figures go into DESIGN.md ("Vertex normals and colours").
"""
import argparse
import json
import os
import signal
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


def unit(grad):
    big = grad.abs().amax(dim=1, keepdim=True)
    ok = torch.isfinite(big) & (big > 0)
    g = grad / torch.where(ok, big, torch.ones_like(big))
    return torch.where(ok, -g / g.norm(dim=1, keepdim=True), torch.zeros_like(grad))


def torch_route(verts, mean, qvec, scale, opacity, color, K, skip):
    from gsgen_amd.knn import knn_raw
    _, idx = knn_raw(mean, K + skip, query=verts)
    idx = idx.long()
    q = qvec / qvec.norm(dim=1, keepdim=True).clamp_min(1e-12)
    w, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    A = (R * (1.0 / (scale * scale))[:, None, :]) @ R.transpose(1, 2)
    d = verts[:, None, :] - mean[idx]
    g = (A[idx] @ d[..., None]).squeeze(-1)
    t = opacity[idx] * torch.exp(-0.5 * (d * g).sum(-1))
    grad = -(t[:, skip:, None] * g[:, skip:]).sum(1)
    rgb = (t[..., None] * color[idx]).sum(1) / t.sum(1, keepdim=True)
    return unit(grad), rgb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reso", type=int, default=128)
    ap.add_argument("--K", type=int, default=3)
    ap.add_argument("--thresh", type=float, default=0.5)
    ap.add_argument("--time-limit", type=int, default=240)
    args = ap.parse_args()
    signal.alarm(args.time_limit)  # (SIGALRM's default action ends the process)
    assert torch.cuda.is_available(), "bench_vertex_attributes needs a GPU"
    import bench
    from gsgen_amd import _capi
    from gsgen_amd.mesh import density_mesh, vertex_attributes
    dev = torch.device("cuda")
    sc, _, _ = bench.make_workload("cfg2")
    mean, qvec, scale = (torch.tensor(sc[k], device=dev, dtype=torch.float32) for k in ("mean", "qvec", "svec"))
    opacity = torch.full((mean.shape[0],), 0.5, device=dev)
    color = torch.rand(mean.shape[0], 3, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    L = mean.abs().max().item() * 1.1
    verts, tris = density_mesh(mean, qvec, scale, opacity, L, args.reso, args.K, args.thresh, True)
    fused = lambda: vertex_attributes(verts, mean, qvec, scale, opacity, color, args.K, True)  # noqa: E731
    route = lambda: torch_route(verts, mean, qvec, scale, opacity, color, args.K, 1)  # noqa: E731
    (fn, fc), (tn, tc) = fused(), route()
    both = torch.isfinite(tc).all(1)  # (the fused colour falls back to the nearest centre where the torch quotient is 0 / 0)
    res = {"tool": "bench_vertex_attributes", "iters": args.iters, "warmup": args.warmup, "lib": _capi.load().path,
           "n_gaussians": int(mean.shape[0]), "reso": args.reso, "K": args.K, "V": int(verts.shape[0]), "F": int(tris.shape[0]),
           "max_abs_diff_normals": float((fn - tn)[both].abs().max()), "max_abs_diff_colors": float((fc - tc)[both].abs().max()),
           "rows_compared": int(both.sum())}
    res["ms_fused"] = round(timed(fused, args.iters, args.warmup), 4)
    res["ms_torch"] = round(timed(route, args.iters, args.warmup), 4)
    res["ms_fused_again"] = round(timed(fused, args.iters, args.warmup), 4)  # (order effects: the first measurement repeated)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
