"""Milliseconds per forward + backward of the fused image loss (gsgen_amd/csrc/loss.hip) beside the torch composition a user has
without it; prints ONE JSON line.

    python tools/bench_loss.py [--iters 100] [--warmup 20] [--sizes 8x800x800,4x512x512] [--no-torch]

Legs: "fused" = gsgen_amd.loss.image_loss(out, gt, 0.2, "l2") + backward; "torch" = the restatement of tests/loss_cases.py
(reflect F.pad + five grouped conv2d + the elementwise SSIM map, fp32 on the device) + backward; "fused_fwd" = the forward alone
under no_grad.  Images are random, not zeros.  Each leg is warmed up and then timed between two events on one stream; the legs
alternate within the process and a second pass runs them in the reverse order; both passes and their mean are reported.  The
condition is only that the fused leg is the faster one: the ratio goes into DESIGN.md, no threshold is fixed here.
Beside the times: the bytes the two kernels must move (forward: read both images, write three maps; backward: read three maps and
both images, write the gradient = 11 image passes) and the rate that is of the fused time -- an end-to-end figure (it includes the
launches and torch's autograd), not a kernel's share of peak.  The two legs' results are compared at the timed size first.
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
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="8x800x800,4x512x512", help="comma-separated BxHxW (3 channels)")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch composition (an A/B of two builds of the kernel)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_loss needs a GPU"
    import loss_cases as LC
    from gsgen_amd import _capi
    from gsgen_amd.loss import image_loss
    dev = torch.device("cuda")
    res = {"tool": "bench_loss", "iters": args.iters, "warmup": args.warmup, "lib": _capi.load().path, "sizes": {}}
    for size in args.sizes.split(","):
        B, H, W = (int(v) for v in size.split("x"))
        gen = torch.Generator(dev).manual_seed(B * H + W)
        gt = torch.rand(B, H, W, 3, device=dev, generator=gen)
        out = (gt + 0.1 * torch.randn(B, H, W, 3, device=dev, generator=gen)).clamp(0, 1).requires_grad_(True)

        def fused():
            out.grad = None
            image_loss(out, gt, 0.2, "l2", 11).backward()

        def composed():
            out.grad = None
            LC.image_loss_torch(out, gt, 0.2, "l2", 11).backward()

        def fused_fwd():
            with torch.no_grad():
                image_loss(out, gt, 0.2, "l2", 11)

        entry = {}
        legs = {"fused": fused, "fused_fwd": fused_fwd}
        if not args.no_torch:
            legs["torch"] = composed
            composed()
            g_t, L_t = out.grad.clone(), float(LC.image_loss_torch(out, gt, 0.2, "l2", 11))
            fused()
            L_f = float(image_loss(out, gt, 0.2, "l2", 11))
            entry["loss_fused"], entry["loss_torch"] = L_f, L_t
            entry["grad_max_abs_diff_over_max"] = float((out.grad - g_t).abs().max() / g_t.abs().max())
            del g_t
        order = list(legs)
        passes = []
        for p in (order, order[::-1]):
            passes.append({name: round(timed(legs[name], args.iters, args.warmup), 4) for name in p})
        entry["ms_pass1"], entry["ms_pass2_reversed"] = passes
        entry["ms"] = {name: round(0.5 * (passes[0][name] + passes[1][name]), 4) for name in order}
        if "torch" in legs:
            entry["torch_over_fused"] = round(entry["ms"]["torch"] / entry["ms"]["fused"], 2)
        image_bytes = 4 * B * H * W * 3
        entry["kernel_bytes_floor"] = 11 * image_bytes
        entry["fused_end_to_end_GBps"] = round(11 * image_bytes / (entry["ms"]["fused"] * 1e-3) / 1e9, 1)
        res["sizes"][size] = entry
        del out, gt
        torch.cuda.empty_cache()
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
