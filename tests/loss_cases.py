"""The image loss of gsgen_amd.loss restated in torch ops, and the cases its tests share (tests/test_loss_host.py on the CPU
emulator, tests/test_gpu_loss.py on the GPU).

`reference_image_loss` is the oracle: kornia 0.6.0's `ssim_loss(out, gt, ws, reduction="mean")` mixed with the mse / l1 loss as
the reference's utils/loss.py:7-47 mixes them, written with `F.pad(mode="reflect")` and a grouped `F.conv2d`; torch autograd
supplies the gradient.  It shares no code with the kernel (gsgen_amd/csrc/loss.hip).  Run in fp64 it is the truth, run in fp32
it is what a user composes from torch ops, and its fp32 error sets the kernel's accuracy bound (`check_bound`): no fixed tolerance.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F


def gauss1d(ws, dtype, device="cpu"):
    x = torch.arange(ws, dtype=dtype, device=device) - ws // 2
    g = torch.exp(-x.pow(2) / (2 * 1.5 ** 2))
    return g / g.sum()


def filt(x, ws):
    """x [B,C,H,W] -> the per-channel correlation of reflect-padded x with the 2-D Gaussian window, same size"""
    g = gauss1d(ws, x.dtype, x.device)
    C, p = x.shape[1], (ws - 1) // 2
    xp = F.pad(x, (p, p, p, p), mode="reflect")
    return F.conv2d(xp, torch.outer(g, g).expand(C, 1, ws, ws).contiguous(), groups=C)


def ssim_map(a, b, ws):
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    mu1, mu2 = filt(a, ws), filt(b, ws)
    s1 = filt(a * a, ws) - mu1 * mu1
    s2 = filt(b * b, ws) - mu2 * mu2
    s12 = filt(a * b, ws) - mu1 * mu2
    return (2 * mu1 * mu2 + C1) * (2 * s12 + C2) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2) + 1e-12)


def image_loss_torch(out, gt, w=0.2, kind="l1", ws=11):
    """out, gt [B,H,W,C] tensors of one dtype and device -> the 0-dim loss (autograd reaches out)"""
    s = ssim_map(out.moveaxis(-1, 1), gt.moveaxis(-1, 1), ws)
    ssim = torch.clamp((1 - s) / 2, 0, 1).mean()
    base = F.mse_loss(out, gt) if kind == "l2" else F.l1_loss(out, gt)
    return w * ssim + (1 - w) * base


def reference_image_loss(out, gt, w, kind, ws, dtype):
    """out, gt: [B,H,W,C] float32 arrays / tensors (their values are converted to `dtype` exactly) -> (loss as a Python float,
    d loss / d out as a float64 array), on the CPU"""
    o = torch.as_tensor(np.asarray(out)).to(dtype).requires_grad_(True)
    g = torch.as_tensor(np.asarray(gt)).to(dtype)
    L = image_loss_torch(o, g, w, kind, ws)
    L.backward()
    return float(L.item()), o.grad.double().numpy()


# (B, H, W, C, ws): the smallest sizes at which each mechanism can break
SHAPES = [
    (1, 6, 6, 3, 11),      # every pixel's window reflects on all four sides
    (2, 16, 16, 3, 11),
    (2, 37, 53, 3, 11),    # not a multiple of any tile
    (1, 7, 19, 3, 3),
    (2, 23, 40, 3, 7),
    (1, 64, 64, 3, 11),
    (1, 128, 96, 3, 11),
    (1, 6, 300, 3, 11),    # one-tile-thin strips
    (1, 300, 6, 3, 11),
    (3, 70, 70, 1, 11),
]
KINDS = ("noise", "smooth", "wide", "constant", "constant2", "same")
SSIM_WEIGHT = 0.2


def make_images(kind, B, H, W, C, seed):
    """-> (out, gt) float32 [B,H,W,C]"""
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand(B, H, W, C, generator=gen, dtype=torch.float64)
    n = torch.randn(B, H, W, C, generator=gen, dtype=torch.float64)
    colour = torch.tensor([1.0, 0.7, 0.4], dtype=torch.float64)[:C]
    if kind in ("noise", "same"):
        gt = u
        out = gt.clone() if kind == "same" else (gt + 0.1 * n).clamp(0, 1)
    elif kind == "smooth":  # (has the sigma = E[x^2] - mu^2 cancellation)
        yy, xx = torch.meshgrid(torch.linspace(0, 3, H, dtype=torch.float64), torch.linspace(0, 3, W, dtype=torch.float64), indexing="ij")
        gt = (0.5 + 0.4 * torch.sin(3 * xx + 2 * yy))[None, :, :, None] * colour + 0.05 * u
        out = (gt + 0.1 * n).clamp(0, 1)
    elif kind == "wide":  # (the renderer does not clamp)
        gt = -0.2 + 1.5 * u
        out = (gt + 0.1 * n).clamp(-0.2, 1.3)
    elif kind == "constant":  # both images the one colour
        gt = (0.9 * colour).expand(B, H, W, C).clone()
        out = gt.clone()
    elif kind == "constant2":  # each image one colour of its own
        gt = (0.9 * colour).expand(B, H, W, C).clone()
        out = (0.25 + 0.5 * colour).expand(B, H, W, C).clone()
    else:
        raise ValueError(kind)
    return out.float().numpy(), gt.float().numpy()


def _cases():
    cases = {}
    for i, (B, H, W, C, ws) in enumerate(SHAPES):
        for j, kind in enumerate(("noise", "smooth")):
            base = ("l2", "l1")[(i + j) % 2]
            cases[f"{kind}-{B}x{H}x{W}x{C}-ws{ws}-{base}"] = (kind, B, H, W, C, ws, base, 100 + 2 * i + j)
    for i, (B, H, W, C, ws) in enumerate([SHAPES[0], SHAPES[2], SHAPES[4], SHAPES[9]]):
        for j, kind in enumerate(("wide", "constant", "constant2", "same")):
            for base in ("l2", "l1") if i == 1 else (("l2", "l1")[(i + j) % 2],):
                cases[f"{kind}-{B}x{H}x{W}x{C}-ws{ws}-{base}"] = (kind, B, H, W, C, ws, base, 200 + 4 * i + j)
    return cases


CASES = _cases()
NAMES = sorted(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(out, gt, ws, base, w, L64, g64, L32, g32): the images (float32 arrays, not to be written to) and the restatement's
    results in fp64 (the truth) and fp32 (its own error is the yardstick), computed once per process"""
    kind, B, H, W, C, ws, base, seed = CASES[name]
    out, gt = make_images(kind, B, H, W, C, seed)
    L64, g64 = reference_image_loss(out, gt, SSIM_WEIGHT, base, ws, torch.float64)
    L32, g32 = reference_image_loss(out, gt, SSIM_WEIGHT, base, ws, torch.float32)
    for arr in (out, gt, g64, g32):
        arr.setflags(write=False)
    return dict(kind=kind, out=out, gt=gt, ws=ws, base=base, w=SSIM_WEIGHT, L64=L64, g64=g64, L32=L32, g32=g32)


def noise_twin(name):
    """the noise case of the same shape and base kind as `name` (made on demand: not every shape has one in CASES)"""
    kind, B, H, W, C, ws, base, seed = CASES[name]
    out, gt = make_images("noise", B, H, W, C, seed)
    return reference_image_loss(out, gt, SSIM_WEIGHT, base, ws, torch.float64)


def bound_report(name, L, g):
    """-> (gradient error, its bound, loss error, its bound, a line for the log).  The bound: 4 x the fp32 restatement's own error
    against fp64, floored at 2^-22 of the largest gradient entry / of the loss (four ulps at the scale of the largest term); the
    4 covers the kernel summing 2 x ws taps separably where conv2d sums ws^2 in another order."""
    c = case(name)
    g = np.asarray(g, np.float64).reshape(c["g64"].shape)
    gmax = np.abs(c["g64"]).max()
    eg, eg32 = np.abs(g - c["g64"]).max(), np.abs(c["g32"] - c["g64"]).max()
    bg = 4 * max(eg32, 2.0 ** -22 * gmax)
    eL, eL32 = abs(float(L) - c["L64"]), abs(c["L32"] - c["L64"])
    bL = 4 * max(eL32, 2.0 ** -22 * abs(c["L64"]))
    line = (f"{name}: L64 {c['L64']:.7f} |L-L64| {eL:.2e} (fp32 torch {eL32:.2e}, bound {bL:.2e}, ratio to bound/4 {eL / (bL / 4):.2f}) "
            f"max|g64| {gmax:.3e} max|g-g64| {eg:.2e} (fp32 torch {eg32:.2e}, bound {bg:.2e}, ratio to bound/4 {eg / (bg / 4) if bg else 0:.2f})")
    return eg, bg, eL, bL, line


def check_bound(name, L, g):
    eg, bg, eL, bL, line = bound_report(name, L, g)
    print(line)
    assert np.isfinite(np.asarray(g)).all() and np.isfinite(L), line
    assert eg <= bg, line
    assert eL <= bL, line


def check_same(name, L, g):
    """out == gt: the loss is 0 up to the 1e-12 of the definition's denominator and the gradient vanishes"""
    _, gn = noise_twin(name)
    gmax = np.abs(np.asarray(g, np.float64)).max()
    print(f"{name}: L {float(L):.3e}, max|g| {gmax:.3e}, 1e-6 of the noise case's {1e-6 * np.abs(gn).max():.3e}")
    assert 0.0 <= float(L) <= 1e-7
    assert np.isfinite(np.asarray(g)).all() and gmax <= 1e-6 * np.abs(gn).max()
