"""Milliseconds per call of farthest point sampling (gsgen_amd/csrc/fps.hip); prints ONE JSON line.

    python tools/bench_fps.py [--iters 20] [--warmup 3] [--K 1024] [--no-torch] [--no-sweep]

Clouds: bench.py's cfg2 (100 k, Point-E init) and cfg3 (500 k) Gaussian centres, and a clustered cloud of 100 k points (12 tight
clusters + 1 % outliers at 100 x the radius).  K = 1024 picks, B = 1 start and B = 4 starts on the shared cloud (the Point-E
guidance's shape), methods brute, bucket and auto, beside a plain torch loop of the same rule (torch.minimum + argmax per pick).
The sweep times brute and bucket at B = 4 on the first 2^k points of a shuffled cfg2 and clustered cloud: the crossover of the auto
routing (AUTO_BUCKET_MIN_POINTS) is read from it.  Every time is the mean of `iters` calls between two events after `warmup`
calls.  No threshold is fixed here: the numbers go into DESIGN.md.
"""
import argparse
import json
import os
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


def clustered_cloud(n, seed=0):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(12, 3))
    n_far = n // 100
    core = centres[rng.integers(0, 12, n - n_far)] + 0.01 * rng.normal(size=(n - n_far, 3))
    far = rng.normal(size=(n_far, 3))
    radius = np.linalg.norm(core, axis=1).max()
    pts = np.concatenate([core, 100.0 * radius * far / np.linalg.norm(far, axis=1, keepdims=True)])
    return pts[rng.permutation(n)].astype(np.float32)


def torch_loop(p, K, starts):
    """the same rule in torch ops, one cloud per start (argmax returns the first maximum: the lowest index)"""
    out = torch.empty(starts.shape[0], K, dtype=torch.int64, device=p.device)
    for b in range(starts.shape[0]):
        m = torch.full((p.shape[0],), float("inf"), device=p.device)
        cur = starts[b].long()
        for k in range(K):
            out[b, k] = cur
            d = p - p[cur]
            m = torch.minimum(m, (d * d).sum(1))
            cur = torch.argmax(m)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--K", type=int, default=1024)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch loop")
    ap.add_argument("--no-sweep", action="store_true", help="skip the crossover sweep")
    ap.add_argument("--no-cfg3", action="store_true", help="skip the 500 k cloud")
    args = ap.parse_args()
    import bench
    from gsgen_amd.fps import AUTO_BUCKET_MIN_POINTS, fps_raw
    dev = torch.device("cuda")
    K = args.K
    res = {"tool": "bench_fps", "iters": args.iters, "K": K, "auto_bucket_min_points": AUTO_BUCKET_MIN_POINTS, "ms": {}, "sweep_ms_B4": {}}
    clouds = {}
    for cfg in ("cfg2",) if args.no_cfg3 else ("cfg2", "cfg3"):
        sc, _, _ = bench.make_workload(cfg)
        clouds[cfg] = torch.tensor(sc["mean"], device=dev, dtype=torch.float32)
    clouds["clustered100k"] = torch.tensor(clustered_cloud(100_000), device=dev)
    g = torch.Generator().manual_seed(0)
    for name, p in clouds.items():
        for B in (1, 4):
            starts = torch.randint(p.shape[0], (B,), generator=g).to(device=dev, dtype=torch.int32)
            for method in ("brute", "bucket", "auto"):
                res["ms"][f"{name}_B{B}_{method}"] = round(timed(lambda: fps_raw(p, K, starts, method=method, shared=True), args.iters,
                                                                 args.warmup), 4)
            if not args.no_torch:
                res["ms"][f"{name}_B{B}_torch_loop"] = round(timed(lambda: torch_loop(p, K, starts), 2, 1), 2)
    if not args.no_sweep:
        for name in ("cfg2", "clustered100k"):
            p = clouds[name][torch.randperm(clouds[name].shape[0], generator=g).to(dev)]
            for e in range(10, 17):
                q = p[:1 << e].contiguous()
                starts = torch.randint(q.shape[0], (4,), generator=g).to(device=dev, dtype=torch.int32)
                Kq = min(K, q.shape[0])
                for method in ("brute", "bucket"):
                    res["sweep_ms_B4"][f"{name}_L{1 << e}_{method}"] = round(
                        timed(lambda: fps_raw(q, Kq, starts, method=method, shared=True), max(args.iters // 2, 3), 2), 4)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
