"""Milliseconds per forward + backward of the three map regularisers (gsgen_amd/csrc/map_loss.hip) beside the torch composition the
trainer runs without it (trainer.py:345-382); prints ONE JSON line.

    python tools/bench_map_loss.py [--iters 300] [--warmup 50] [--repeats 5] [--sizes 4x512x512,8x800x800] [--no-launch-count]

Legs, forward + backward through autograd with the gradients going to opacity and z_var: "fused" = gsgen_amd.loss.map_loss with the three
weights; "torch" = the reference's three expressions as torch ops; "fused_fwd" = the fused forward alone under no_grad.  The maps are
rendered-like (a soft disc, z_var on its rim), not zeros.  A leg is warmed up and then timed between two events on one stream; the legs
alternate within the process, `repeats` times, the odd rounds in the reverse order; the median of a leg's repeats and their spread are
reported.  The results of the two are compared at the timed size first.  No speed ratio is fixed.  Beside the times: the device kernels
one forward + backward of each leg launches (torch.profiler, in a pass of its own after the timing; "not measured" if the profiler is
not available), and the bytes the fused kernels must move (forward: two maps; backward: the two again and two gradients = 24 bytes a
pixel) with the rate that is of the fused time -- an end-to-end figure including launches and autograd, not a kernel's share of peak.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
W = (1e-3, 1e-3, 1e-3)


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


def loss_torch(opacity, z_var):
    """trainer.py:345-382 with utils/ops.py:51-55, as the trainer writes them (the clamp evaluated once per term that uses it)"""
    sparsity = (opacity ** 2 + 0.01).sqrt().mean()
    c = opacity.clamp(1e-3, 1.0 - 1e-3)
    opague = -(c * torch.log(c) + (1 - c) * torch.log(1 - c)).mean()
    c = opacity.clamp(1e-3, 1.0 - 1e-3)
    z = (z_var / c * (c > 0.5)).mean()
    return W[0] * sparsity + W[1] * opague + W[2] * z


def count_kernels(fn):
    """device kernels of one call of fn, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception as e:  # noqa: BLE001
        print(f"bench_map_loss: launch count not measured ({type(e).__name__}: {e})", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="4x512x512,8x800x800", help="comma-separated BxHxW")
    ap.add_argument("--no-launch-count", action="store_true", help="skip the torch.profiler pass")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_map_loss needs a GPU"
    from gsgen_amd import _capi
    from gsgen_amd.loss import map_loss
    dev = torch.device("cuda")
    res = {"tool": "bench_map_loss", "iters": args.iters, "warmup": args.warmup, "repeats": args.repeats, "weights": W,
           "lib": _capi.load().path, "sizes": {}}
    for size in args.sizes.split(","):
        B, H, W_ = (int(v) for v in size.split("x"))
        gen = torch.Generator(dev).manual_seed(B * H + W_)
        yy, xx = torch.meshgrid(torch.linspace(-1, 1, H, device=dev), torch.linspace(-1, 1, W_, device=dev), indexing="ij")
        r = torch.sqrt(xx * xx + yy * yy)[None] / (0.5 + 0.3 * torch.rand(B, 1, 1, device=dev, generator=gen))
        u = torch.rand(B, H, W_, device=dev, generator=gen)
        opacity = torch.sigmoid((1 - r) * 12)
        opacity = torch.where(opacity < 1e-3, torch.zeros_like(opacity), opacity)[..., None].contiguous().requires_grad_(True)
        z_var = (1e-2 * torch.exp(-((r - 1) / 0.15) ** 2) * (0.5 + u))[..., None].contiguous().requires_grad_(True)

        def fused(o, z):
            return map_loss(o, z, *W)

        def leg(fn):
            def run():
                opacity.grad = z_var.grad = None
                fn(opacity, z_var).backward()
            return run

        def fused_fwd():
            with torch.no_grad():
                map_loss(opacity, z_var, *W)

        legs = {"fused": leg(fused), "torch": leg(loss_torch), "fused_fwd": fused_fwd}
        entry = {}
        for name, fn in (("fused", fused), ("torch", loss_torch)):  # the two agree before they are timed
            legs[name]()
            entry["loss_" + name] = float(fn(opacity, z_var).detach())
            if name == "fused":
                g_f = (opacity.grad.clone(), z_var.grad.clone())
            else:
                entry["grad_max_abs_diff_over_max_torch_vs_fused"] = [float((g.grad - f).abs().max() / f.abs().max())
                                                                      for g, f in zip((opacity, z_var), g_f)]
        order = list(legs)
        rounds = []
        for k in range(args.repeats):
            rounds.append({name: timed(legs[name], args.iters, args.warmup) for name in (order if k % 2 == 0 else order[::-1])})
        entry["ms_rounds"] = {name: [round(r_[name], 4) for r_ in rounds] for name in order}
        entry["ms"] = {name: round(statistics.median(r_[name] for r_ in rounds), 4) for name in order}
        entry["torch_over_fused"] = round(entry["ms"]["torch"] / entry["ms"]["fused"], 2)
        nbytes = B * H * W_ * 24
        entry["kernel_bytes_floor"] = nbytes
        entry["fused_end_to_end_GBps"] = round(nbytes / (entry["ms"]["fused"] * 1e-3) / 1e9, 1)
        if not args.no_launch_count:
            entry["device_kernels_fwd_bwd"] = {name: count_kernels(legs[name]) or "not measured" for name in ("fused", "torch")}
        res["sizes"][size] = entry
        del opacity, z_var
        torch.cuda.empty_cache()
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
