"""Milliseconds per call of the kNN kernel (gsgen_amd/csrc/knn.hip) and of what is built on it; prints ONE JSON line.

    python tools/bench_knn.py [--iters 20] [--warmup 3]

Rows: bench.py's cfg2 (100 k, Point-E init) and cfg3 (500 k) Gaussian centres, clean and with 1 % of the points moved to 100x the
cloud's radius, at K = 2, 4, 8, 16, 32; cfg2 with 2 % and 5 % so moved, at K = 4 and 32 (where the grid box stops
excluding the outliers); a torch brute force on the same GPU and cloud (chunked pairwise distances + topk); the model's
densify_by_compatness(3) end to end and auxiliary_loss with NN + compat configured (cfg2).  Every time is the mean of `iters`
calls between two events, after `warmup` calls.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--brute-iters", type=int, default=2)
    ap.add_argument("--kernel-only", action="store_true", help="only the kNN rows (no brute force, no model rows)")
    args = ap.parse_args()
    import bench
    import knn_cases as KC
    from test_gpu_knn import with_outliers
    from gsgen_amd.knn import knn_raw
    dev = torch.device("cuda")
    res = {"tool": "bench_knn", "iters": args.iters, "ms": {}}
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
    if args.kernel_only:
        res["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(res))
        return
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
