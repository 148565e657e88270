"""Milliseconds per forward + backward of the fused MLP background composite (gsgen_amd/csrc/background.hip) beside the same
computation composed from torch ops on the same GPU in the same process; prints ONE JSON line.

    python tools/bench_background.py [--iters 20] [--repeats 7] [--warmup 5] [--sizes 4x512x512,8x800x800]

Legs, each a forward + backward through autograd with gradients to the 768 parameters, to rgb and to opacity:
"fused" = gsgen_amd.background.mlp_background_over (rays from the camera blocks, SH encoding, 16 x 2 ReLU MLP, sigmoid, nan_to_num and
rgb + (1 - opacity) bg in one launch; the backward recomputes it and sums the weight gradient on the fp32 MFMA); "torch" = DESIGN.md's
definition ("MLP background") in torch ops, rays included; "torch_given_dirs" = the same with the ray directions precomputed, the
form that favours torch most (the fused leg has no such shortcut: it always derives them).  "fused_fwd" is the forward alone under
no_grad.  The torch composition is the yardstick, not the code under test; the three legs' results are compared at the timed size
first.  Inputs are random (rotated cameras, uniform rgb and opacity, a normal upstream gradient), not zeros.  Every leg is warmed up;
a sample is `iters` calls between two device events on one stream; the legs alternate and `repeats` samples of each are taken; the
median, the smallest and the largest sample are reported.  Beside the times: the bytes the fused kernels must move per pixel
(forward: rgb 12 + opacity 4 in, 12 out; backward: gradient 12 + opacity 4 in, grad_opacity 4 out = 48) and the rate that is of the
fused time -- an end-to-end figure including launches and autograd, not a kernel's share of peak.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def rays(c2w, intr, H, W):
    dev = c2w.device
    x, y = torch.arange(W, dtype=torch.float32, device=dev), torch.arange(H, dtype=torch.float32, device=dev)
    qx, qy = (x[None] - intr[:, 2:3]) / intr[:, 0:1], (y[None] - intr[:, 3:4]) / intr[:, 1:2]
    B = c2w.shape[0]
    cam = torch.stack((qx[:, None, :].expand(B, H, W), qy[:, :, None].expand(B, H, W), torch.ones(B, H, W, device=dev)), -1)
    return torch.einsum("bij,bhwj->bhwi", c2w[:, :, :3], cam)


def background_torch(params, d):
    e = 2 * d - 1
    x, y, z = e[..., 0], e[..., 1], e[..., 2]
    one = torch.ones_like(x)
    u = torch.stack((0.28209479177387814 * one, -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
                     1.0925484305920792 * x * y, -1.0925484305920792 * y * z, 0.94617469575755997 * z * z - 0.31539156525251999,
                     -1.0925484305920792 * x * z, 0.54627421529603959 * x * x - 0.54627421529603959 * y * y,
                     one, one, one, one, one, one, one), -1)
    W0, W1, W2 = params[:256].view(16, 16), params[256:512].view(16, 16), params[512:560].view(3, 16)
    return torch.nan_to_num(torch.sigmoid(torch.relu(torch.relu(u @ W0.T) @ W1.T) @ W2.T))


def sample(fn, iters):
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
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="4x512x512,8x800x800", help="comma-separated BxHxW")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_background needs a GPU"
    from gsgen_amd import _capi
    from gsgen_amd.background import INIT_BOUND, camera_blocks, mlp_background_over
    dev = torch.device("cuda")
    res = {"tool": "bench_background", "iters": args.iters, "repeats": args.repeats, "warmup": args.warmup, "lib": _capi.load().path, "sizes": {}}
    for size in args.sizes.split(","):
        B, H, W = (int(v) for v in size.split("x"))
        gen = torch.Generator().manual_seed(B * H + W)
        q, _ = torch.linalg.qr(torch.randn(B, 3, 3, generator=gen))
        c2w = torch.cat((q, torch.randn(B, 3, 1, generator=gen)), 2).to(dev)
        intr = torch.cat((W * (0.9 + 0.2 * torch.rand(B, 2, generator=gen)), torch.tensor([[W / 2.0, H / 2.0]]).expand(B, 2)
                          + torch.rand(B, 2, generator=gen) * 8), 1).to(dev)
        cams = camera_blocks(c2w, intr)
        params = ((torch.rand(768, generator=gen) * 2 - 1) * INIT_BOUND).to(dev).requires_grad_(True)
        rgb = torch.rand(B, H, W, 3, generator=gen).to(dev).requires_grad_(True)
        opacity = torch.rand(B, H, W, 1, generator=gen).to(dev).requires_grad_(True)
        grad = torch.randn(B, H, W, 3, generator=gen).to(dev)
        dirs = rays(c2w, intr, H, W)
        leaves = (params, rgb, opacity)

        def leg(fn):
            def run():
                for t in leaves:
                    t.grad = None
                fn().backward(grad)
            return run

        def fused_fwd():
            with torch.no_grad():
                mlp_background_over(params, rgb, opacity, cams)

        forms = {"fused": lambda: mlp_background_over(params, rgb, opacity, cams),
                 "torch": lambda: rgb + (1 - opacity) * background_torch(params, rays(c2w, intr, H, W)),
                 "torch_given_dirs": lambda: rgb + (1 - opacity) * background_torch(params, dirs)}
        legs = {name: leg(fn) for name, fn in forms.items()}
        legs["fused_fwd"] = fused_fwd
        entry = {}
        legs["fused"]()
        out_f, gp_f, go_f = forms["fused"]().detach(), params.grad.clone(), opacity.grad.clone()
        legs["torch"]()  # the two agree before they are timed
        entry["out_max_abs_diff_torch_vs_fused"] = float((forms["torch"]().detach() - out_f).abs().max())
        entry["grad_params_max_abs_diff_over_max_torch_vs_fused"] = float((params.grad - gp_f).abs().max() / gp_f.abs().max())
        entry["grad_opacity_max_abs_diff_over_max_torch_vs_fused"] = float((opacity.grad - go_f).abs().max() / go_f.abs().max())
        order = list(legs)
        for name in order:
            for _ in range(args.warmup):
                legs[name]()
        torch.cuda.synchronize()
        samples = {name: [] for name in order}
        for r in range(args.repeats):
            for name in (order if r % 2 == 0 else order[::-1]):
                samples[name].append(sample(legs[name], args.iters))
        entry["ms"] = {name: round(statistics.median(v), 4) for name, v in samples.items()}
        entry["ms_min"] = {name: round(min(v), 4) for name, v in samples.items()}
        entry["ms_max"] = {name: round(max(v), 4) for name, v in samples.items()}
        entry["torch_over_fused"] = round(entry["ms"]["torch"] / entry["ms"]["fused"], 2)
        entry["torch_given_dirs_over_fused"] = round(entry["ms"]["torch_given_dirs"] / entry["ms"]["fused"], 2)
        entry["fused_not_slower_than_torch"] = bool(entry["ms"]["fused"] <= min(entry["ms"]["torch"], entry["ms"]["torch_given_dirs"]))
        nbytes = B * H * W * 48
        entry["kernel_bytes_floor"] = nbytes
        entry["fused_end_to_end_GBps"] = round(nbytes / (entry["ms"]["fused"] * 1e-3) / 1e9, 1)
        entry["fused_end_to_end_fp32_TFLOPs"] = round(B * H * W * 2 * (3 * 560 + 304) / (entry["ms"]["fused"] * 1e-3) / 1e12, 2)
        res["sizes"][size] = entry
        del dirs, rgb, opacity, grad, out_f, go_f
        torch.cuda.empty_cache()
    assert math.isfinite(sum(e["ms"]["fused"] for e in res["sizes"].values()))
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
