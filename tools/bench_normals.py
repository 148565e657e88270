"""Milliseconds per gsgen_amd.normals.estimate_normal call (k_point_normals, gsgen_amd/csrc/knn.hip); prints ONE JSON line.

    python tools/bench_normals.py [--iters 20] [--warmup 3] [--time-limit 400]

Rows, each the mean of `iters` calls between two events on one stream after `warmup` calls, allocations included:
  estimate_normal on bench.py's cfg2 (100 k, Point-E init) and cfg3 (500 k) Gaussian centres at K = 30 (conf/renderer/
    normal_as_rgb.yaml) and K = 50 (pytorch3d's default; the 64-entry list);
  knn_raw on the same clouds at K = 30, the search alone with its [N, K] outputs written (K = 50 is beyond its lists);
  "torch", K = 30: the composition available without the fused kernel -- knn_raw, a gather of [N, K, 3], centred covariances in
    torch, torch.linalg.eigh (no disambiguation: the fused call does more).  Where eigh fails on this GPU build the row is the
    kNN + gather + covariance part alone and "eigh" says why.  The two normals are compared up to sign (max |n x n'| over the
    points whose eigenvalue gap is above 1e-2), so that the comparison is of equal work;
  one forward of the model class with cfg.normal_as_rgb at 4 x 512^2 on cfg2, beside the plain forward of the same model.
The process ends itself after --time-limit seconds.  The figures go into DESIGN.md ("Point-cloud normals").
"""
import argparse
import json
import os
import signal
import sys

import numpy as np
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


def covariances(p, K):
    from gsgen_amd.knn import knn_raw
    _, idx = knn_raw(p, K)
    d = p[idx.long()] - p[:, None, :]
    c = d - d.mean(1, keepdim=True)
    return c.transpose(1, 2) @ c / K


def torch_route(p, K):
    lam, V = torch.linalg.eigh(covariances(p, K))
    return lam, V[:, :, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--time-limit", type=int, default=400)
    args = ap.parse_args()
    signal.alarm(args.time_limit)  # (SIGALRM's default action ends the process)
    assert torch.cuda.is_available(), "bench_normals needs a GPU"
    import bench
    from gsgen_amd import _capi
    from gsgen_amd.knn import knn_raw
    from gsgen_amd.model import GaussianSplattingRenderer
    from gsgen_amd.normals import estimate_normal
    from gsgen_amd.renderer import CameraInfo
    dev = torch.device("cuda")
    res = {"tool": "bench_normals", "iters": args.iters, "warmup": args.warmup, "lib": _capi.load().path, "ms": {}}
    ms = res["ms"]
    scenes = {}
    for cfg in ("cfg2", "cfg3"):
        scenes[cfg], _, _ = bench.make_workload(cfg)
        p = torch.tensor(scenes[cfg]["mean"], device=dev, dtype=torch.float32)
        res["n_" + cfg] = int(p.shape[0])
        for K in (30, 50):
            ms[f"{cfg}_estimate_normal_K{K}"] = round(timed(lambda: estimate_normal(p, K), args.iters, args.warmup), 4)
        ms[f"{cfg}_knn_raw_K30"] = round(timed(lambda: knn_raw(p, 30), args.iters, args.warmup), 4)
        try:
            lam, n_t = torch_route(p, 30)
            torch.cuda.synchronize()
            n_f = estimate_normal(p, 30)
            ok = (lam[:, 1] - lam[:, 0]) > 1e-2 * lam[:, 2]
            res[f"{cfg}_max_cross_vs_torch"] = float(torch.linalg.cross(n_f, n_t).norm(dim=1)[ok].max())
            res[f"{cfg}_rows_compared"] = int(ok.sum())
            ms[f"{cfg}_torch_K30"] = round(timed(lambda: torch_route(p, 30), max(args.iters // 4, 2), 1), 4)
        except RuntimeError as e:  # (no eigh on this build: say so, time the part that runs)
            res["eigh"] = f"unavailable: {str(e).splitlines()[0][:200]}"
        ms[f"{cfg}_torch_K30_without_eigh"] = round(timed(lambda: covariances(p, 30), max(args.iters // 4, 2), 1), 4)
        ms[f"{cfg}_estimate_normal_K30_again"] = round(timed(lambda: estimate_normal(p, 30), args.iters, args.warmup), 4)
    # the view itself: 4 cameras of 512^2 on cfg2
    sc = scenes["cfg2"]
    n = sc["mean"].shape[0]
    cams = bench.camera_poses(4, 0, 512, 512)
    batch = {"c2w": torch.tensor(np.stack([c.c2w for c in cams])), "camera_info": [CameraInfo(*c.intr) for c in cams]}
    rng = np.random.default_rng(1)
    init = dict(mean=sc["mean"], qvec=sc["qvec"], svec=sc["svec"], color=rng.uniform(0.1, 0.9, (n, 3)).astype(np.float32),
                alpha=rng.uniform(0.2, 0.9, n).astype(np.float32))
    for name, extra in (("plain", {}), ("normal_as_rgb", dict(normal_as_rgb=True, normal=dict(neighborhood_size=30, disambiguate_directions=True)))):
        cfg = dict(device="cuda", svec_act="exp", alpha_act="sigmoid", color_act="sigmoid", tile_size=16, T_thresh=1e-4, depth_detach=True,
                   background=dict(type="fixed", color=[0.1, 0.2, 0.3]), densify=dict(enabled=False), prune=dict(enabled=False), **extra)
        m = GaussianSplattingRenderer(cfg, {k: torch.tensor(np.ascontiguousarray(v), device=dev, dtype=torch.float32) for k, v in init.items()})
        with torch.no_grad():
            ms[f"cfg2_forward_4x512_{name}"] = round(timed(lambda: m(batch), args.iters, args.warmup), 4)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
