"""Milliseconds per forward + backward of the Pearson depth loss (gsgen_amd/csrc/depth_loss.hip) beside the two torch forms a user has
without it; prints ONE JSON line.

    python tools/bench_depth_loss.py [--iters 200] [--warmup 30] [--sizes 4x512x512] [--no-launch-count]

Legs, each with and without a 70 % mask, forward + backward through autograd with the gradient going to the predicted depth:
"fused" = gsgen_amd.loss.pearson_depth_loss; "loop" = the reference's form (utils/loss.py:50-66: a Python loop over the batch, a
boolean-mask gather per image -- a host synchronisation -- and the centred Pearson formula that torchmetrics evaluates); "where" =
a synchronisation-free torch composition of the same (torch.where and row sums over [B, P]); "fused_fwd" = the forward alone under
no_grad.  Depth maps are random and depth-like, not zeros.  Each leg is warmed up and then timed between two events on one stream;
the legs alternate within the process and a second pass runs them in the reverse order; both passes and their mean are reported.
No speed ratio is fixed: what is checked elsewhere (tests/test_gpu_depth_loss.py) is that the fused leg can be captured, which "loop"
cannot.  Beside the times: the device kernels one forward + backward of each leg launches (torch.profiler, in a pass of its own after
the timing; "not measured" if the profiler is not available) and the bytes the three fused kernels must move (forward: pred, gt
and mask once; backward: the same again and one gradient = 22 bytes a pixel with a mask, 20 without), with the rate that is of the
fused time -- an end-to-end figure including launches and autograd, not a kernel's share of peak.  The three legs' results are
compared at the timed size first.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


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


def loss_loop(pred, gt, mask):
    """the reference's loop; torchmetrics' PearsonCorrCoef on a fresh state is the centred formula"""
    if mask is None:
        mask = torch.ones_like(gt[..., 0], dtype=torch.bool)
    loss = 0
    for p, g, m in zip(pred, gt, mask):
        x, y = torch.nan_to_num(p)[m].reshape(-1), g[m].reshape(-1)
        dx, dy = x - x.mean(), y - y.mean()
        loss = loss + 1 - (dx * dy).sum() / torch.sqrt((dx * dx).sum() * (dy * dy).sum())
    return loss / pred.shape[0]


def loss_where(pred, gt, mask):
    """the same without a gather: no host synchronisation, fixed shapes"""
    x, y = torch.nan_to_num(pred).flatten(1), gt.flatten(1)
    if mask is None:
        dx, dy = x - x.mean(1, keepdim=True), y - y.mean(1, keepdim=True)
    else:
        m = mask.flatten(1)
        n = m.sum(1, keepdim=True)
        dx = torch.where(m, x - torch.where(m, x, 0.0).sum(1, keepdim=True) / n, 0.0)
        dy = torch.where(m, y - torch.where(m, y, 0.0).sum(1, keepdim=True) / n, 0.0)
    r = (dx * dy).sum(1) / torch.sqrt((dx * dx).sum(1) * (dy * dy).sum(1))
    return (1 - r.clamp(-1, 1)).mean()


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
        print(f"bench_depth_loss: launch count not measured ({type(e).__name__}: {e})", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--sizes", default="4x512x512", help="comma-separated BxHxW")
    ap.add_argument("--no-launch-count", action="store_true", help="skip the torch.profiler pass")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_depth_loss needs a GPU"
    from gsgen_amd import _capi
    from gsgen_amd.loss import pearson_depth_loss
    dev = torch.device("cuda")
    res = {"tool": "bench_depth_loss", "iters": args.iters, "warmup": args.warmup, "lib": _capi.load().path, "sizes": {}}
    for size in args.sizes.split(","):
        B, H, W = (int(v) for v in size.split("x"))
        gen = torch.Generator(dev).manual_seed(B * H + W)
        yy, xx = torch.meshgrid(torch.linspace(0, 3, H, device=dev), torch.linspace(0, 3, W, device=dev), indexing="ij")
        gt = (3.0 + torch.sin(2 * xx + yy)[None] + 0.3 * torch.rand(B, H, W, device=dev, generator=gen))[..., None]
        pred = (0.5 * gt + 1.0 + 0.15 * torch.randn(B, H, W, 1, device=dev, generator=gen)).requires_grad_(True)
        mask70 = torch.rand(B, H, W, device=dev, generator=gen) < 0.7
        for tag, mask in (("mask70", mask70), ("nomask", None)):
            def leg(fn, mask=mask):
                def run():
                    pred.grad = None
                    fn(pred, gt, mask).backward()
                return run

            def fused_fwd(mask=mask):
                with torch.no_grad():
                    pearson_depth_loss(pred, gt, mask)

            legs = {"fused": leg(pearson_depth_loss), "fused_fwd": fused_fwd, "loop": leg(loss_loop), "where": leg(loss_where)}
            entry = {}
            for name in ("fused", "loop", "where"):  # the three agree before they are timed
                legs[name]()
                entry["loss_" + name] = float({"fused": pearson_depth_loss, "loop": loss_loop, "where": loss_where}[name](pred, gt, mask).detach())
                if name == "fused":
                    g_f = pred.grad.clone()
                else:
                    entry[f"grad_max_abs_diff_over_max_{name}_vs_fused"] = float((pred.grad - g_f).abs().max() / g_f.abs().max())
            order = list(legs)
            passes = []
            for p in (order, order[::-1]):
                passes.append({name: round(timed(legs[name], args.iters, args.warmup), 4) for name in p})
            entry["ms_pass1"], entry["ms_pass2_reversed"] = passes
            entry["ms"] = {name: round(0.5 * (passes[0][name] + passes[1][name]), 4) for name in order}
            entry["loop_over_fused"] = round(entry["ms"]["loop"] / entry["ms"]["fused"], 2)
            entry["where_over_fused"] = round(entry["ms"]["where"] / entry["ms"]["fused"], 2)
            nbytes = B * H * W * (22 if mask is not None else 20)
            entry["kernel_bytes_floor"] = nbytes
            entry["fused_end_to_end_GBps"] = round(nbytes / (entry["ms"]["fused"] * 1e-3) / 1e9, 1)
            if not args.no_launch_count:
                entry["device_kernels_fwd_bwd"] = {name: count_kernels(legs[name]) or "not measured" for name in ("fused", "loop", "where")}
            res["sizes"][f"{size}-{tag}"] = entry
        del pred, gt, mask70
        torch.cuda.empty_cache()
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
