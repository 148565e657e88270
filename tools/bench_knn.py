"""Milliseconds per call of the kNN kernel (gsgen_amd/csrc/knn.hip) and of what is built on it; prints ONE JSON line.

    python tools/bench_knn.py [--iters 20] [--warmup 3]

Rows: bench.py's cfg2 (100 k, Point-E init) and cfg3 (500 k) Gaussian centres, clean and with 1 % of the points moved to 100x the
cloud's radius, at K = 2, 4, 8, 16, 32; cfg2 with 2 % and 5 % so moved, at K = 4 and 32 (where the grid box stops
excluding the outliers); a torch brute force on the same GPU and cloud (chunked pairwise distances + topk); the model's
densify_by_compatness(3) end to end and auxiliary_loss with NN + compat configured (cfg2).  Every time is the mean of `iters`
calls between two events, after `warmup` calls.

The query search (gsgen_knn_query): Q = N jittered copies of the cloud's points in bucket-coherent order (the order of a coarse
cell sort of the cloud) and the same queries shuffled, K = 2, 4, 8, 32.  The density lattice (gsgen_density_grid): 128^3, K = 3, on
cfg2, beside a torch brute force shaped like the reference's loop (chunks of --lattice-chunk lattice points: cdist, topk of K + 1,
gather, bmm).  --lattice-only runs the lattice alone (for a kernel trace).
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


def brute_topk(p, K, chunk=4096):
    out = []
    for a in range(0, p.shape[0], chunk):
        d2 = torch.cdist(p[a:a + chunk], p).square_()
        out.append(torch.topk(d2, K, dim=1, largest=False, sorted=True).indices)
    return torch.cat(out)


def coherent_queries(p, seed=0):
    """jittered copies of the points in the order of a coarse cell sort (neighbours in the array are neighbours in space), and the
    same queries shuffled"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    lo, hi = p.min(0).values, p.max(0).values
    c = ((p - lo) / (hi - lo).clamp_min(1e-12) * 32).long().clamp_(0, 31)
    order = torch.argsort((c[:, 2] * 32 + c[:, 1]) * 32 + c[:, 0])
    r = float((hi - lo).max())
    q = p[order] + 1e-3 * r * torch.randn(p.shape[0], 3, generator=g).to(p.device)
    return q, q[torch.randperm(q.shape[0], generator=g).to(p.device)]


def brute_lattice(mean, qvec, scale, opacity, L, reso, K, chunk):
    """the reference's loop (utils/export.py:66-120) with torch's own search: per chunk cdist + topk(K + 1), column 0 dropped"""
    from gsgen_amd.densify import rotmat_of_qvec
    R = rotmat_of_qvec(qvec)
    cov_inv = torch.inverse((R * scale[:, None, :] ** 2) @ R.transpose(1, 2))
    ax = torch.linspace(-L, L, reso, device=mean.device)
    grid = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    out = torch.empty(grid.shape[0], device=mean.device)
    for a in range(0, grid.shape[0], chunk):
        pos = grid[a:a + chunk]
        idx = torch.topk(torch.cdist(pos, mean), K + 1, dim=1, largest=False, sorted=True).indices[:, 1:].reshape(-1)
        d = pos.repeat_interleave(K, 0) - mean[idx]
        m = torch.bmm(torch.bmm(d[:, None, :], cov_inv[idx]), d[:, :, None]).reshape(-1)
        out[a:a + chunk] = (opacity[idx] * torch.exp(-0.5 * m)).reshape(-1, K).sum(1)
    return out.reshape(reso, reso, reso)


def lattice_rows(res, args, dev):
    import bench
    from gsgen_amd.density import density_grid
    sc, _, _ = bench.make_workload("cfg2")
    mean, qvec, scale = (torch.tensor(sc[k], device=dev, dtype=torch.float32) for k in ("mean", "qvec", "svec"))
    opacity = torch.full((mean.shape[0],), 0.5, device=dev)
    L = mean.abs().max().item() * 1.1
    res["ms"]["cfg2_density_grid_128_K3"] = round(timed(lambda: density_grid(mean, qvec, scale, opacity, L, 128, 3), args.iters, args.warmup), 3)
    res["ms"]["cfg2_density_grid_64_K3"] = round(timed(lambda: density_grid(mean, qvec, scale, opacity, L, 64, 3), args.iters, args.warmup), 3)
    if not args.lattice_only:
        res["lattice_chunk"] = args.lattice_chunk
        res["ms"]["cfg2_density_grid_128_K3_torch_brute"] = round(
            timed(lambda: brute_lattice(mean, qvec, scale, opacity, L, 128, 3, args.lattice_chunk), 1, 0), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--brute-iters", type=int, default=2)
    ap.add_argument("--kernel-only", action="store_true", help="only the kNN rows (no brute force, no model rows)")
    ap.add_argument("--lattice-only", action="store_true", help="only the density lattice (no brute force)")
    ap.add_argument("--lattice-chunk", type=int, default=8192, help="lattice points per chunk of the torch brute force")
    args = ap.parse_args()
    import bench
    import knn_cases as KC
    from test_gpu_knn import with_outliers
    from gsgen_amd.knn import knn_raw
    dev = torch.device("cuda")
    res = {"tool": "bench_knn", "iters": args.iters, "ms": {}}
    if args.lattice_only:
        lattice_rows(res, args, dev)
        res["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(res))
        return
    clouds = {}
    for cfg in ("cfg2", "cfg3"):
        sc, _, _ = bench.make_workload(cfg)
        p = torch.tensor(sc["mean"], device=dev, dtype=torch.float32)
        clouds[cfg] = p
        clouds[cfg + "_outliers1pct"] = with_outliers(p)
        for pct in ((2, 5) if cfg == "cfg2" else ()):
            q = with_outliers(p, pct / 100.0)
            for K in (4, 32):
                res["ms"][f"{cfg}_outliers{pct}pct_K{K}"] = round(timed(lambda: knn_raw(q, K), 3, 1), 4)
    for name, p in clouds.items():
        for K in (2, 4, 8, 16, 32):
            res["ms"][f"{name}_K{K}"] = round(timed(lambda: knn_raw(p, K), args.iters, args.warmup), 4)
        if args.kernel_only:
            continue
        res["ms"][f"{name}_torch_brute_K4"] = round(timed(lambda: brute_topk(p, 4), args.brute_iters, 1), 3)
        res["ms"][f"{name}_torch_brute_K32"] = round(timed(lambda: brute_topk(p, 32), args.brute_iters, 1), 3)
    for cfg in ("cfg2", "cfg3"):  # the query search: Q = N, ordered and shuffled
        p = clouds[cfg]
        q_ord, q_shuf = coherent_queries(p)
        for K in (2, 4, 8, 32):
            res["ms"][f"{cfg}_query_ordered_K{K}"] = round(timed(lambda: knn_raw(p, K, query=q_ord), args.iters, args.warmup), 4)
            res["ms"][f"{cfg}_query_shuffled_K{K}"] = round(timed(lambda: knn_raw(p, K, query=q_shuf), args.iters, args.warmup), 4)
    if args.kernel_only:
        res["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(res))
        return
    lattice_rows(res, args, dev)
    # model features on cfg2's cloud
    sc, _, _ = bench.make_workload("cfg2")
    n = sc["mean"].shape[0]
    raw = {"mean": sc["mean"], "qvec": sc["qvec"], "svec": torch.log(torch.tensor(sc["svec"])).numpy(),
           "color": torch.zeros(n, 3).numpy(), "alpha": torch.zeros(n).numpy()}

    def densify():
        m = KC.model_from_raw(raw, dev)
        m.densify_by_compatness(3)
    res["ms"]["cfg2_densify_by_compatness3_incl_model_setup"] = round(timed(densify, max(args.iters // 4, 2), 1), 3)
    m = KC.model_from_raw(raw, dev)
    res["ms"]["cfg2_model_setup_only"] = round(timed(lambda: KC.model_from_raw(raw, dev), max(args.iters // 4, 2), 1), 3)
    m = KC.model_from_raw(raw, dev, penalty={"NN": {"value": 1.0}, "compat": {"type": "l1", "value": 1.0}})
    res["ms"]["cfg2_auxiliary_loss_NN_compat_fwd"] = round(timed(lambda: m.auxiliary_loss(1), args.iters, args.warmup), 4)
    res["ms"]["cfg2_auxiliary_loss_NN_compat_fwd_bwd"] = round(timed(lambda: m.auxiliary_loss(1).backward(), args.iters,
                                                                     args.warmup), 4)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
