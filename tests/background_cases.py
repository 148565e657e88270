"""The MLP background of gsgen_amd.background restated in torch ops, and the cases its tests share (tests/test_background_host.py on
the CPU emulator, tests/test_gpu_background.py on the GPU).

`background_torch` is the oracle: DESIGN.md's definition ("MLP background") in plain torch ops -- rays from the camera, e = 2 d - 1,
nine SH terms and seven ones, two 16-wide ReLU layers without biases, a sigmoid, nan_to_num -- with autograd for the gradients.  It
shares no code with the kernel (gsgen_amd/csrc/background.hip); the SH constants are written out again here.  Run in fp64 it is the
truth, run in fp32 it is what a user composes from torch ops, and its fp32 error sets the kernel's accuracy bound (`check`): an error
may be at most 4 x the fp32 restatement's own error against fp64, floored at 2^-22 of the tensor's largest entry.  No other tolerance.

The ReLU kink.  A ReLU's gradient jumps at 0, so a pre-activation whose sign differs between two correct fp32 evaluations would
make a gradient differ by a whole term, and no rounding bound covers that.  `case` therefore asserts that no fp64 pre-activation
of any pixel lies within 64 x the case's largest fp32-vs-fp64 pre-activation error of zero -- no pixel is excluded; the seeds
below were searched for on the CPU (the first of 1, 2, ... for which this holds).  What the search can find depends on the size: the
expected number of pixels that close to a kink grows with the pixel count (about one per thousand pixels for every kink line that
crosses the image).  The two small shapes use ordinary lenses (fx about W) and a dozen units change sign inside the image; at the
two large shapes no seed in reach passes with an ordinary lens, so those cameras have longer lenses (fx about 6 W and 3 W): fewer
kink lines cross a view, but some still do (the counts are beside the cases).

The backward kernel gives a workgroup a run of max(4, ceil(P / 262144)) * 256 consecutive pixels and sums eight partials per pass
of the final reduction (background.hip: kMinIters, kThreads, kMaxGroups, kSlices), hence the shapes:
    1 x 16 x 16      one partial workgroup
    2 x 37 x 53      tail lanes, P no multiple of 64, a workgroup's run crossing the two views
    3 x 64 x 64      several workgroups per view
    1 x 160 x 200    32 workgroups: more than one pass of the final reduction
"""
import functools
import math

import numpy as np
import torch

N_PARAMS, WIDTH = 768, 16
INIT_BOUND = math.sqrt(6.0 / 32.0)
FLOOR = 2.0 ** -22
KINK_MARGIN = 64.0


def rays_torch(c2w, intr, H, W):
    """c2w [B,3,4], intr [B,4] = fx fy cx cy (one dtype) -> d [B,H,W,3] = R ((x - cx) / fx, (y - cy) / fy, 1), not normalised"""
    dt, dev = c2w.dtype, c2w.device
    x, y = torch.arange(W, dtype=dt, device=dev), torch.arange(H, dtype=dt, device=dev)
    qx = (x[None, :] - intr[:, 2:3]) / intr[:, 0:1]           # [B,W]
    qy = (y[None, :] - intr[:, 3:4]) / intr[:, 1:2]           # [B,H]
    B = c2w.shape[0]
    cam = torch.stack((qx[:, None, :].expand(B, H, W), qy[:, :, None].expand(B, H, W), torch.ones(B, H, W, dtype=dt, device=dev)), -1)
    return torch.einsum("bij,bhwj->bhwi", c2w[:, :, :3], cam)


def encode_torch(d):
    """d [...,3] -> u [...,16]: the nine real SH terms of degree < 3 at e = 2 d - 1, then seven ones"""
    e = 2 * d - 1
    x, y, z = e[..., 0], e[..., 1], e[..., 2]
    one = torch.ones_like(x)
    return torch.stack((0.28209479177387814 * one, -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
                        1.0925484305920792 * x * y, -1.0925484305920792 * y * z, 0.94617469575755997 * z * z - 0.31539156525251999,
                        -1.0925484305920792 * x * z, 0.54627421529603959 * x * x - 0.54627421529603959 * y * y,
                        one, one, one, one, one, one, one), -1)


def background_torch(params, d, want_pre=False):
    """params [768] = W0 | W1 | W2 ([16 out][16 in] row-major each; rows 3..15 of W2 unused), d [...,3] -> bg [...,3]"""
    W0, W1, W2 = params[:256].view(16, 16), params[256:512].view(16, 16), params[512:560].view(3, 16)
    z1 = encode_torch(d) @ W0.T
    z2 = torch.relu(z1) @ W1.T
    bg = torch.nan_to_num(torch.sigmoid(torch.relu(z2) @ W2.T))
    return (bg, z1, z2) if want_pre else bg


def over_torch(rgb, opacity, bg):
    """the heads path's composite: rgb [B,H,W,3] + (1 - opacity [B,H,W,1]) bg"""
    return rgb + (1 - opacity) * bg


# name -> ((B, H, W), lens = fx / W, seed)
CASES = {
    "one-1x16x16": ((1, 16, 16), 1.0, 1),            # 13 of the 32 hidden units change sign inside the image
    "tail-2x37x53": ((2, 37, 53), 1.0, 204),         # 12
    "views-3x64x64": ((3, 64, 64), 6.0, 275),        # 15, over the three views
    "passes-1x160x200": ((1, 160, 200), 3.0, 99),    # 1
}
NAMES = sorted(CASES)


def make_inputs(shape, lens, seed):
    """-> dict of float32 tensors: c2w [B,3,4] (random rotations), intr [B,4] (fx != fy, off-centre cx, cy), params [768]
    (U(-sqrt(6/32), sqrt(6/32))), rgb [B,H,W,3], opacity [B,H,W,1] in [0, 1], grad [B,H,W,3]"""
    B, H, W = shape
    gen = torch.Generator().manual_seed(1000 + seed)
    q, r = torch.linalg.qr(torch.randn(B, 3, 3, generator=gen, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=1, dim2=2))[:, None, :]
    q = q * torch.linalg.det(q)[:, None, None]                      # proper rotations
    c2w = torch.cat((q, torch.randn(B, 3, 1, generator=gen, dtype=torch.float64)), 2).float()
    f = lens * W * (0.9 + 0.2 * torch.rand(B, 2, generator=gen, dtype=torch.float64))
    c = torch.tensor([W / 2.0, H / 2.0], dtype=torch.float64) + (torch.rand(B, 2, generator=gen, dtype=torch.float64) - 0.5) * 0.3 * min(H, W)
    intr = torch.cat((f, c), 1).float()
    params = ((torch.rand(N_PARAMS, generator=gen, dtype=torch.float64) * 2 - 1) * INIT_BOUND).float()
    rgb = torch.rand(B, H, W, 3, generator=gen)
    opacity = torch.rand(B, H, W, 1, generator=gen)
    grad = torch.randn(B, H, W, 3, generator=gen)
    return dict(c2w=c2w, intr=intr, params=params, rgb=rgb, opacity=opacity, grad=grad)


def evaluate(inp, shape, dtype):
    """the restatement in `dtype` on the CPU -> dict of tensors in `dtype`: dirs, z1, z2, bg, out (the composite), gp_plain = d <grad,
    bg> / d params, gp_over = d <grad, out> / d params, g_opacity = d <grad, out> / d opacity"""
    B, H, W = shape
    t = {k: v.to(dtype) for k, v in inp.items()}
    p = t["params"].clone().requires_grad_(True)
    op = t["opacity"].clone().requires_grad_(True)
    d = rays_torch(t["c2w"], t["intr"], H, W)
    bg, z1, z2 = background_torch(p, d, want_pre=True)
    out = over_torch(t["rgb"], op, bg)
    (gp_plain,) = torch.autograd.grad((bg * t["grad"]).sum(), p, retain_graph=True)
    gp_over, g_op = torch.autograd.grad((out * t["grad"]).sum(), (p, op))
    return dict(dirs=d, z1=z1.detach(), z2=z2.detach(), bg=bg.detach(), out=out.detach(), gp_plain=gp_plain, gp_over=gp_over, g_opacity=g_op)


def kink_report(r64, r32):
    """-> (the smallest |fp64 pre-activation|, the largest fp32-vs-fp64 pre-activation error) over both hidden layers and all pixels"""
    z64 = torch.cat((r64["z1"].reshape(-1), r64["z2"].reshape(-1)))
    z32 = torch.cat((r32["z1"].reshape(-1), r32["z2"].reshape(-1))).double()
    return float(z64.abs().min()), float((z32 - z64).abs().max())


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(shape, inputs as float32 tensors (not to be written to), r64, r32): computed once per process; asserts the kink guard"""
    shape, lens, seed = CASES[name]
    inp = make_inputs(shape, lens, seed)
    r64, r32 = evaluate(inp, shape, torch.float64), evaluate(inp, shape, torch.float32)
    zmin, zerr = kink_report(r64, r32)
    assert zmin >= KINK_MARGIN * zerr, f"{name}: a pre-activation at {zmin:.3e} is within {KINK_MARGIN} x {zerr:.3e} of a ReLU kink: pick another seed"
    assert all(bool(torch.isfinite(v).all()) for v in r64.values())
    return dict(shape=shape, r64=r64, r32=r32, **inp)


def cam_blocks(c, stride_floats=16):
    """the case's cameras as gsgen_pack_camera lays them out: [B, stride] float32, floats 0..11 the c2w rows, 12..15 fx fy cx cy"""
    B = c["c2w"].shape[0]
    blocks = torch.full((B, stride_floats), 7.0)
    blocks[:, :12] = c["c2w"].reshape(B, 12)
    blocks[:, 12:16] = c["intr"]
    return blocks


def tensor_bound(x64, x32):
    """-> (the bound, e32): 4 x the largest error e32 of the fp32 result against the fp64 one, floored at 2^-22 of the largest entry"""
    e32 = float((x32.double() - x64).abs().max())
    return 4 * max(e32, FLOOR * float(x64.abs().max())), e32


def bound(name, what):
    """-> (the bound, the fp32 restatement's own error) for result `what` of case `name`"""
    c = case(name)
    return tensor_bound(c["r64"][what], c["r32"][what])


def check(name, what, got, scale=1.0):
    """got (array or tensor, any shape with the result's element count) against the fp64 restatement of `what`, times `scale`"""
    c = case(name)
    x64 = c["r64"][what]
    got = torch.as_tensor(np.asarray(got.detach().cpu() if isinstance(got, torch.Tensor) else got)).double().reshape(x64.shape)
    b, e32 = bound(name, what)
    err = float((got - scale * x64).abs().max())
    line = f"{name} {what}: err {err:.3e} (fp32 torch {scale * e32:.3e}, bound {scale * b:.3e}, largest entry {scale * float(x64.abs().max()):.3e})"
    print(line)
    assert bool(torch.isfinite(got).all()), line
    assert err <= scale * b, line
