"""Milliseconds per forward + backward of the guidance seam (gsgen_amd/csrc/guidance_seam.hip through gsgen_amd.guidance) beside the
torch sequences of the reference it replaces; prints ONE JSON line.

    python tools/bench_guidance.py [--seconds 1.0] [--repeats 5] [--warmup 20] [--no-launch-count]

Guidance input, B = 4, square renders 512 -> 512, 800 -> 512, 256 -> 512 and 512 -> 64:
    "torch" = rgb.permute(0, 3, 1, 2) -> F.interpolate(.., bilinear, align_corners=False) -> * 2.0 -> - 1.0 -> .to(fp16)
              (guidance/stable_diffusion.py:274-284 with encode_images at :143-149),
    "fused" = gsgen_amd.guidance.vae_input,
each followed by .backward(g) with a fixed fp16 upstream gradient, the image gradient landing in rgb.grad.
SDS loss, [4, 4, 64, 64]:
    "torch" = nan_to_num -> clamp -> latents - grad -> mse_loss(sum) -> * 0.5 / bs, with loss_sds_each and grad.norm()
              (stable_diffusion.py:298-312),
    "fused" = gsgen_amd.guidance.sds_loss,
each followed by loss.backward().
The two variants run in one process and alternate: every shape is warmed, then each repeat times first one variant and then the
other between two device events around enough calls to fill `--seconds`, the order swapping from repeat to repeat.  Reported per
shape and variant: the median milliseconds per call, the repeats themselves, and their spread (max - min); beside them the device
kernels one forward + backward launches (torch.profiler, in a pass of its own after the timing; "not measured" without it).  The
results of the two variants are compared before they are timed.  There is no fallback: without a GPU the tool fails.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

INPUT_SHAPES = [(4, 512, 512), (4, 800, 512), (4, 256, 512), (4, 512, 64)]  # (B, render side, guidance side)
SDS_SHAPE = (4, 4, 64, 64)
CLIP = 1.0


def events_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


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
        print(f"bench_guidance: launch count not measured ({type(e).__name__}: {e})", file=sys.stderr)
        return None


def torch_input(rgb, side):
    return (F.interpolate(rgb.permute(0, 3, 1, 2), (side, side), mode="bilinear", align_corners=False) * 2.0 - 1.0).to(torch.float16)


def torch_sds(latents, grad, clip):
    bs = latents.shape[0]
    grad = torch.nan_to_num(grad)
    grad = grad.clamp(-clip, clip)
    target = (latents - grad).detach()
    loss = 0.5 * F.mse_loss(latents, target, reduction="sum") / bs
    each = 0.5 * F.mse_loss(latents, target, reduction="none").sum(dim=[1, 2, 3])
    return loss, each, grad.norm()


def measure(legs, seconds, repeats, warmup, launch_count):
    """legs: {"torch": fn, "fused": fn} -> the entry of one shape"""
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    calls = {name: max(10, int(seconds * 1e3 / max(events_ms(fn, 20), 1e-4))) for name, fn in legs.items()}
    runs = {name: [] for name in legs}
    for r in range(repeats):
        for name in (list(legs) if r % 2 == 0 else list(legs)[::-1]):
            runs[name].append(events_ms(legs[name], calls[name]))
    entry = {"calls_per_repeat": calls}
    for name, ms in runs.items():
        entry[name] = {"ms": round(statistics.median(ms), 5), "repeats_ms": [round(v, 5) for v in ms], "spread_ms": round(max(ms) - min(ms), 5)}
    entry["torch_over_fused"] = round(entry["torch"]["ms"] / entry["fused"]["ms"], 3)
    entry["fused_minus_torch_ms"] = round(entry["fused"]["ms"] - entry["torch"]["ms"], 5)
    entry["fused_not_slower_beyond_spread"] = bool(entry["fused"]["ms"] - entry["torch"]["ms"] <= max(entry["fused"]["spread_ms"], entry["torch"]["spread_ms"]))
    if launch_count:
        entry["device_kernels_fwd_bwd"] = {name: count_kernels(fn) or "not measured" for name, fn in legs.items()}
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="device time one timed repeat of one variant should fill")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-launch-count", action="store_true", help="skip the torch.profiler pass")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_guidance needs a GPU"
    from gsgen_amd import _capi
    from gsgen_amd import guidance as GG
    dev = torch.device("cuda")
    res = {"tool": "bench_guidance", "seconds": args.seconds, "repeats": args.repeats, "warmup": args.warmup, "lib": _capi.load().path,
           "guidance_input": {}, "sds_loss": {}}
    for B, side_in, side_out in INPUT_SHAPES:
        gen = torch.Generator(dev).manual_seed(side_in + side_out)
        rgb = torch.rand(B, side_in, side_in, 3, device=dev, generator=gen).requires_grad_(True)
        g = torch.randn(B, 3, side_out, side_out, device=dev, generator=gen).half()

        def leg(fn, rgb=rgb, g=g, side=side_out):
            def run():
                rgb.grad = None
                fn(rgb, side).backward(g)
            return run
        legs = {"torch": leg(torch_input), "fused": leg(lambda t, side: GG.vae_input(t, side))}
        legs["torch"]()
        g_t, o_t = rgb.grad.clone(), torch_input(rgb, side_out).detach().float()
        legs["fused"]()
        entry = {"out_max_abs_diff": float((GG.vae_input(rgb, side_out).detach().float() - o_t).abs().max()),
                 "grad_max_abs_diff_over_max": float((rgb.grad - g_t).abs().max() / g_t.abs().max())}
        entry.update(measure(legs, args.seconds, args.repeats, args.warmup, not args.no_launch_count))
        res["guidance_input"][f"{B}x{side_in}x{side_in}->{side_out}x{side_out}"] = entry
        del rgb, g, legs
        torch.cuda.empty_cache()
    gen = torch.Generator(dev).manual_seed(5)
    latents = torch.randn(SDS_SHAPE, device=dev, generator=gen).requires_grad_(True)
    grad = 1.5 * torch.randn(SDS_SHAPE, device=dev, generator=gen)

    def sds_leg(fn):
        def run():
            latents.grad = None
            loss, each, norm = fn(latents, grad, CLIP)
            loss.backward()
            return loss, each, norm
        return run
    legs = {"torch": sds_leg(torch_sds), "fused": sds_leg(GG.sds_loss)}
    lt = [float(v.detach().sum()) for v in legs["torch"]()]
    g_t = latents.grad.clone()
    lf = [float(v.detach().sum()) for v in legs["fused"]()]
    entry = {"loss_each_norm_torch": lt, "loss_each_norm_fused": lf, "grad_max_abs_diff_over_max": float((latents.grad - g_t).abs().max() / g_t.abs().max())}
    entry.update(measure(legs, args.seconds, args.repeats, args.warmup, not args.no_launch_count))
    res["sds_loss"]["x".join(map(str, SDS_SHAPE))] = entry
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
