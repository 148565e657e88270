"""The guidance seam of gsgen_amd.guidance restated in torch ops, and the cases its tests share (tests/test_guidance_host.py on the CPU
emulator, tests/test_gpu_guidance.py on the GPU).

`resize_torch` is torch's upsample_bilinear2d map with align_corners=False and no antialiasing written out per axis
    src = max(in / out * (o + 0.5) - 0.5, 0),  i0 = min(int(src), in - 1),  i1 = min(i0 + 1, in - 1),  l1 = src - i0,  l0 = 1 - l1,
    out = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11),  then scale * out + shift
as gathers, with autograd for the gradient; `sds_torch` is the reference's chain (guidance/stable_diffusion.py:298-312).  Neither
shares code with the kernels (gsgen_amd/csrc/guidance_seam.hip).  Run in fp64 they are the truth, run in fp32 they are what a user
composes from torch ops, and their fp32 error sets the kernels' accuracy bound: the rule of tests/depth_loss_cases.py::bound_report,
    error against fp64 <= 4 x max(the fp32 restatement's own error against fp64, 2^-22 of the tensor's largest entry),
plus, for an fp16 output, the rounding fp16 itself imposes: 2^-11 |value|, 2^-25 below 2^-14.  The yardstick is not one number: on
130 x 70 -> 32 x 48 it is some 4e-6, because the source coordinate is rounded in fp32, and 1e-7 elsewhere.
"""
import functools

import numpy as np
import torch

FLOOR = 2.0 ** -22
KPIX, KCHUNK = 4, 1024  # guidance_seam.hip: kPix, kChunk (tests/test_guidance_host.py checks them against the compiled file)


# ---- the resize ---------------------------------------------------------------------------------------------------------------
def axis_torch(n_in, n_out, dtype):
    """-> (i0, i1 int64 [n_out], l0, l1 [n_out] in dtype)"""
    o = torch.arange(n_out, dtype=dtype)
    rs = torch.tensor(float(n_in), dtype=dtype) / torch.tensor(float(n_out), dtype=dtype)
    src = torch.clamp(rs * (o + 0.5) - 0.5, min=0)
    i0 = torch.clamp(src.long(), max=n_in - 1)
    i1 = torch.clamp(i0 + 1, max=n_in - 1)
    l1 = src - i0.to(dtype)
    return i0, i1, 1 - l1, l1


def resize_torch(x, OH, OW, scale=1.0, shift=0.0):
    """x [B,H,W,C] -> [B,OH,OW,C] in x's dtype"""
    _, H, W, _ = x.shape
    y0, y1, ly0, ly1 = axis_torch(H, OH, x.dtype)
    x0, x1, lx0, lx1 = axis_torch(W, OW, x.dtype)
    r0, r1 = x[:, y0], x[:, y1]
    lx0, lx1, ly0, ly1 = lx0[None, None, :, None], lx1[None, None, :, None], ly0[None, :, None, None], ly1[None, :, None, None]
    out = ly0 * (lx0 * r0[:, :, x0] + lx1 * r0[:, :, x1]) + ly1 * (lx0 * r1[:, :, x0] + lx1 * r1[:, :, x1])
    return scale * out + shift


def reference_resize(x, OH, OW, scale, shift, grads, dtype):
    """x [B,H,W,C] float32 array, grads: upstream gradients [B,OH,OW,C] float32 arrays -> (out float64 [B,OH,OW,C], [d / d x for each
    upstream] float64 [B,H,W,C]) computed on the CPU in `dtype`"""
    xt = torch.as_tensor(np.asarray(x)).to(dtype).requires_grad_(True)
    out = resize_torch(xt, OH, OW, scale, shift)
    gx = []
    for g in grads:
        (gi,) = torch.autograd.grad(out, xt, torch.as_tensor(np.asarray(g)).to(dtype), retain_graph=True)
        gx.append(gi.double().numpy())
    return out.detach().double().numpy(), gx


# (H, W, OH, OW): the smallest shapes at which each mechanism can fail
SHAPES = [
    (16, 16, 16, 16),    # identity: every l1 = 0
    (5, 7, 16, 12),      # upsampling, several outputs per input and axis
    (8, 8, 16, 16),
    (25, 19, 16, 12),    # downsampling, every input touched
    (67, 67, 8, 8),      # 51 of 67 input rows untouched
    (23, 7, 7, 13),      # 10 of 23 rows untouched; 7 x 13 = 91 elements per plane: odd fp16 plane bases, row tails
    (130, 70, 32, 48),   # the largest fp32 coordinate error found
    (1, 1, 8, 8),        # clamped neighbours, i1 == i0
    (3, 1, 4, 4),
    (2, 2, 1, 1),
]
ONE_CHANNEL = [(16, 16, 16, 16), (5, 7, 16, 12), (23, 7, 7, 13), (67, 67, 8, 8), (1, 1, 8, 8)]
# (H, W, OH, OW, C, B)
RESIZE_CASES = [s + (3, B) for s in SHAPES for B in (1, 3)] + [s + (1, 3) for s in ONE_CHANNEL] + [ONE_CHANNEL[2] + (1, 1)]
SCALE, SHIFT = 2.0, -1.0


def resize_id(c):
    return "%dx%d-%dx%d-c%d-b%d" % c


@functools.lru_cache(maxsize=None)
def resize_case(c):
    """-> dict: x [B,H,W,C], the upstream gradients g32 (full fp32) and g16 (exactly representable in fp16) [B,OH,OW,C], and the
    restatement's results with the affine 2 x - 1 (out, gx32, gx16) and without it (out_plain, gx32_plain), each in fp64 ("...64") and
    in fp32 ("...32"), computed once per process; arrays, not to be written to"""
    H, W, OH, OW, C, B = c
    gen = torch.Generator().manual_seed(1000 + RESIZE_CASES.index(c))
    x = torch.rand(B, H, W, C, generator=gen).numpy()
    g32 = torch.randn(B, OH, OW, C, generator=gen).numpy()
    g16 = torch.randn(B, OH, OW, C, generator=gen).half().float().numpy()
    d = dict(x=x, g32=g32, g16=g16)
    for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
        d["out" + tag], (d["gx32" + tag], d["gx16" + tag]) = reference_resize(x, OH, OW, SCALE, SHIFT, (g32, g16), dtype)
        d["out_plain" + tag], (d["gx32_plain" + tag],) = reference_resize(x, OH, OW, 1.0, 0.0, (g32,), dtype)
    for a in d.values():
        a.setflags(write=False)
    return d


def untouched(n_in, n_out):
    """-> bool [n_in]: the input indices no output reads with a weight other than zero, from the fp32 map (the kernel's: the same
    operations in the same order)"""
    i0, i1, l0, l1 = axis_torch(n_in, n_out, torch.float32)
    hit = np.zeros(n_in, bool)
    hit[i0[l0 != 0].numpy()] = True
    hit[i1[l1 != 0].numpy()] = True
    return ~hit


def check(what, got, y64, y32, half=False):
    """the bound: |got - y64| <= 4 max(|y32 - y64|_max, 2^-22 |y64|_max) (+ per entry, for an fp16 result, 2^-11 |y64|, or 2^-25 below
    2^-14); prints the measured error beside it"""
    got, y64, y32 = np.asarray(got, np.float64), np.asarray(y64, np.float64), np.asarray(y32, np.float64)
    assert got.shape == y64.shape, (what, got.shape, y64.shape)
    assert np.isfinite(got).all(), what
    e32 = np.abs(y32 - y64).max()
    bound = np.full(y64.shape, 4 * max(e32, FLOOR * np.abs(y64).max()))
    if half:
        bound = bound + np.where(np.abs(y64) >= 2.0 ** -14, 2.0 ** -11 * np.abs(y64), 2.0 ** -25)
    err = np.abs(got - y64)
    k = np.argmax(err - bound)
    print(f"{what}: err {err.flat[k]:.3e} bound {bound.flat[k]:.3e} (largest err {err.max():.3e}, fp32 torch {e32:.3e})")
    assert (err <= bound).all(), (what, err.flat[k], bound.flat[k])


def to_layout(a, planar):
    """[B,OH,OW,C] -> the layout a kernel takes or gives"""
    return np.ascontiguousarray(np.moveaxis(a, 3, 1)) if planar else np.ascontiguousarray(a)


def from_layout(a, planar):
    return np.moveaxis(a, 1, 3) if planar else a


# ---- the SDS loss --------------------------------------------------------------------------------------------------------------
def sds_torch(latents, grad, clip):
    """guidance/stable_diffusion.py:298-312 on tensors of one dtype (grad already through nan_to_num in fp32)
    -> (loss_sds, loss_sds_each [B], grad_norm)"""
    B = latents.shape[0]
    if clip is not None:
        grad = grad.clamp(-clip, clip)
    target = (latents - grad).detach()
    loss = 0.5 * torch.nn.functional.mse_loss(latents, target, reduction="sum") / B
    each = 0.5 * torch.nn.functional.mse_loss(latents, target, reduction="none").flatten(1).sum(1)
    return loss, each.detach(), grad.norm()


def reference_sds(latents, grad, clip, dtype, scale=1.0):
    """float32 arrays -> (loss, each [B], norm, d (scale * loss) / d latents) as float64 arrays, on the CPU in `dtype`"""
    lt = torch.as_tensor(np.asarray(latents)).to(dtype).requires_grad_(True)
    g = torch.nan_to_num(torch.as_tensor(np.asarray(grad))).to(dtype)  # (sanitised in fp32, then converted exactly)
    loss, each, norm = sds_torch(lt, g, clip)
    (scale * loss).backward()
    return loss.detach().double().numpy(), each.double().numpy(), norm.double().numpy(), lt.grad.double().numpy()


SDS_SHAPES = [(1, 4, 8, 8), (3, 4, 8, 8), (2, 4, 5, 7), (4, 4, 64, 64)]
# (shape, clip, kind)
SDS_CASES = [(s, clip, "rand") for s in SDS_SHAPES for clip in (None, 1.0)] + [(s, 1.0, "nonfinite") for s in SDS_SHAPES] + \
            [((3, 4, 8, 8), None, "zeros"), ((2, 4, 5, 7), 1.0, "zeros")]


def sds_id(c):
    return "%s-clip%s-%s" % ("x".join(map(str, c[0])), c[1], c[2])


def sds_inputs(c, seed_offset=0):
    """-> (latents, grad) float32 arrays"""
    shape, _, kind = c
    gen = torch.Generator().manual_seed(2000 + SDS_CASES.index(c) + 100 * seed_offset)
    latents = torch.randn(shape, generator=gen)
    grad = 1.5 * torch.randn(shape, generator=gen)  # (a third of the entries beyond a clip of 1)
    if kind == "zeros":
        grad = torch.zeros(shape)
    if kind == "nonfinite":
        flat = grad.view(-1)
        at = 1 + torch.randperm(flat.numel() - 1, generator=gen)[:9]
        flat[at[:3]], flat[at[3:6]], flat[at[6:]] = float("nan"), float("inf"), float("-inf")
        flat[0] = float("nan")
    return latents.numpy(), grad.numpy()


@functools.lru_cache(maxsize=None)
def sds_case(c):
    """-> dict(latents, grad, loss64, each64, norm64, g64, and the same in fp32), computed once per process"""
    latents, grad = sds_inputs(c)
    d = dict(latents=latents, grad=grad)
    for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
        d["loss" + tag], d["each" + tag], d["norm" + tag], d["g" + tag] = reference_sds(latents, grad, c[1], dtype)
    for a in d.values():
        a.setflags(write=False)
    return d


def check_sds(c, loss, each, norm, g, scale=1.0):
    d = sds_case(c)
    name = sds_id(c)
    check(name + " loss", loss, d["loss64"], d["loss32"])
    check(name + " each", each, d["each64"], d["each32"])
    check(name + " norm", norm, d["norm64"], d["norm32"])
    if g is not None:
        check(name + " grad", g, scale * d["g64"], scale * d["g32"])
        assert not np.asarray(g)[np.isnan(d["grad"])].any()  # a NaN entry of grad: a zero gradient
