"""The seam between the rendered batch and the diffusion guidance of the text-to-3D step on the GPU (gsgen_amd/csrc/guidance_seam.hip
through the C ABI): the guidance's input image from the render, and the SDS loss from the UNet's gradient.

Going in, the reference runs (guidance/stable_diffusion.py:274-284 with encode_images at :143-149; stable_diffusion_vsd.py:419,
:586-590, make_it_3d.py:124-128 and deep_floyd.py:196-201 do the same)
    rgb.permute(0, 3, 1, 2) -> F.interpolate(.., (512, 512), mode="bilinear", align_corners=False) -> * 2.0 -> - 1.0 -> .to(fp16)
and coming out (stable_diffusion.py:298-312)
    nan_to_num -> clamp -> latents - grad -> mse_loss(reduction="sum") -> * 0.5 -> / bs, plus loss_sds_each and grad.norm():
some sixteen launches forward and ten backward, torch's bilinear backward among them (a zero fill and a float-atomic scatter, so the
image gradient differs in its last bits from run to run).  Here the way in is one launch forward and one backward, the way out two
and one.  DESIGN.md ("Guidance seam") has the definitions and the two deliberate points: the affine is applied once, after the
interpolation (the bilinear weights sum to 1, so DeepFloyd's affine-first form is the same function), and the loss is summed from
g'^2 directly (the reference's latents - (latents - g') is g' up to one rounding of latents).

Images are [B, H, W, C] or [H, W, C] float32 CUDA (HIP) tensors, channels last as the renderer delivers them, C 1 or 3; a [H, W, C]
image is a batch of one.  Everything runs on the current stream with its workspace from torch's caching allocator, never
synchronises with the host, can be captured by `torch.cuda.graph` and replayed on new values in the same tensors, and is
bit-identical from run to run (no float atomics: the resize's backward is a gather).
"""
import torch
from torch.autograd.function import once_differentiable

from . import _capi

LAYOUTS = ("BCHW", "BHWC")
MAX_SIDE = 1 << 16   # gsgen_amd/csrc/guidance_seam.hip: kMaxSide
MAX_BATCH = 65535    # (the SDS loss: one grid row per image)


def _lib():
    lib = _capi.load()
    if not hasattr(lib, "guidance_input_forward"):
        raise RuntimeError(f"{lib.path} was built without the guidance seam kernels (gsgen_amd/csrc/guidance_seam.hip): rebuild it "
                           "(python -m gsgen_amd.build)")
    return lib


# The per-axis tables of one (H, W, OH, OW) quadruple, built on the device by the first forward that needs them and kept: one small
# tensor per (device, stream, quadruple).  Under stream capture nothing is kept: a captured launch has not run when the capture ends,
# so a table made there is rebuilt by the graph itself on every replay, in memory the graph owns.
_TABLES = {}


def _tables(lib, dev, H, W, OH, OW):
    """-> (uint8 tensor, its size, build: whether the forward about to be enqueued must write the tables first)"""
    nbytes = lib.guidance_input_workspace_bytes(H, W, OH, OW)
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(nbytes, device=dev, dtype=torch.uint8), nbytes, 1
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream, H, W, OH, OW)
    hit = _TABLES.get(key)
    if hit is not None:
        return hit, nbytes, 0
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    _TABLES[key] = ws
    return ws, nbytes, 1


class _GuidanceInput(torch.autograd.Function):
    """x [B,H,W,C] float32 contiguous -> scale * bilinear(x) + shift at OH x OW, planar [B,C,OH,OW] or channels last [B,OH,OW,C],
    float16 or float32"""

    @staticmethod
    def forward(ctx, x, OH, OW, scale, shift, half, planar):
        B, H, W, C = x.shape
        dev = x.device
        lib = _lib()
        ws, nbytes, build = _tables(lib, dev, H, W, OH, OW)
        out = torch.empty((B, C, OH, OW) if planar else (B, OH, OW, C), device=dev, dtype=torch.float16 if half else torch.float32)
        lib.guidance_input_forward(x.data_ptr(), B, H, W, C, OH, OW, scale, shift, int(half), int(planar), out.data_ptr(), build,
                                   ws.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(ws)
            ctx.args = (B, H, W, C, OH, OW, scale, planar, nbytes)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (ws,) = ctx.saved_tensors
        B, H, W, C, OH, OW, scale, planar, nbytes = ctx.args
        if g.dtype not in (torch.float16, torch.float32):
            g = g.to(torch.float32)
        g = g.contiguous()
        grad = torch.empty((B, H, W, C), device=g.device, dtype=torch.float32)
        _lib().guidance_input_backward(g.data_ptr(), int(g.dtype == torch.float16), int(planar), B, H, W, C, OH, OW, scale, grad.data_ptr(),
                                       ws.data_ptr(), nbytes, torch.cuda.current_stream(g.device).cuda_stream)
        return grad, None, None, None, None, None, None


def _size(size):
    if isinstance(size, (tuple, list)):
        if len(size) != 2:
            raise ValueError(f"gsgen_amd.guidance: size must be an integer or (height, width), got {size!r}")
        oh, ow = size
    else:
        oh = ow = size
    if int(oh) != oh or int(ow) != ow or not (1 <= int(oh) <= MAX_SIDE and 1 <= int(ow) <= MAX_SIDE):
        raise ValueError(f"gsgen_amd.guidance: size must be positive integers up to {MAX_SIDE}, got {size!r}")
    return int(oh), int(ow)


def _check(rgb, size, dtype, layout):
    """-> (OH, OW); every check comes before the device check, so that a CPU tensor reaches each of them"""
    if not isinstance(rgb, torch.Tensor) or rgb.dim() not in (3, 4):
        raise ValueError(f"gsgen_amd.guidance: rgb must be a [B, H, W, C] or [H, W, C] tensor, got shape "
                         f"{tuple(getattr(rgb, 'shape', ())) or type(rgb)}")
    oh, ow = _size(size)
    if layout not in LAYOUTS:
        raise ValueError(f"gsgen_amd.guidance: layout must be one of {LAYOUTS}, got {layout!r}")
    if dtype not in (torch.float16, torch.float32):
        raise NotImplementedError(f"gsgen_amd.guidance: the output is float16 or float32, got {dtype}")
    H, W, C = rgb.shape[-3:]
    if rgb.numel() == 0:
        raise ValueError(f"gsgen_amd.guidance: an empty batch or an empty image cannot be resized, got shape {tuple(rgb.shape)}")
    if C not in (1, 3):
        raise NotImplementedError(f"gsgen_amd.guidance: images of {C} channels -- the kernels take 1 or 3 (channels last)")
    if H > MAX_SIDE or W > MAX_SIDE:
        raise NotImplementedError(f"gsgen_amd.guidance: a {H} x {W} image -- the kernels take sides up to {MAX_SIDE}")
    if rgb.dtype != torch.float32:
        raise NotImplementedError(f"gsgen_amd.guidance: images must be float32, got {rgb.dtype}")
    if not rgb.is_cuda:
        raise ValueError("gsgen_amd.guidance: images must be CUDA (HIP) tensors -- there is no CPU implementation")
    return oh, ow


def to_guidance(rgb, size=(512, 512), scale=2.0, shift=-1.0, dtype=torch.float16, layout="BCHW"):
    """scale * F.interpolate(rgb as [B,C,H,W], size, mode="bilinear", align_corners=False) + shift in `dtype` (float16 or float32),
    as [B, C, OH, OW] (layout "BCHW") or [B, OH, OW, C] ("BHWC"); differentiable with respect to rgb.  `size`: an integer or
    (height, width)."""
    oh, ow = _check(rgb, size, dtype, layout)
    if rgb.dim() == 3:
        rgb = rgb[None]
    return _GuidanceInput.apply(rgb.contiguous(), oh, ow, float(scale), float(shift), dtype == torch.float16, layout == "BCHW")


def vae_input(rgb, size=512, dtype=torch.float16):
    """what encode_images hands the VAE (stable_diffusion.py:143-149, :274-284): 2 * resize(rgb) - 1 as [B, 3, size, size]"""
    return to_guidance(rgb, size, 2.0, -1.0, dtype, "BCHW")


def if_input(rgb):
    """DeepFloyd's input (deep_floyd.py:196-201): [B, 3, 64, 64] float32 with the affine applied"""
    return to_guidance(rgb, 64, 2.0, -1.0, torch.float32, "BCHW")


def rgb_as_latents(rgb):
    """stable_diffusion.py:276-278: the render resized to [B, C, 64, 64] float32 and used as latents, no affine"""
    return to_guidance(rgb, 64, 1.0, 0.0, torch.float32, "BCHW")


def resize(img, size):
    """channels last in, channels last float32 out, no affine: the per-step resize of the image-conditioned step's target image and
    depth map (trainer.py:661-673).  A [H, W, C] image comes back as [OH, OW, C].  Differentiable, by the same kernel."""
    out = to_guidance(img, size, 1.0, 0.0, torch.float32, "BHWC")
    return out[0] if img.dim() == 3 else out


class _SdsLoss(torch.autograd.Function):
    """latents, grad [B, ...] float32 contiguous -> (loss 0-dim, loss_each [B], grad_norm 0-dim).  Only the loss is differentiable,
    with respect to latents."""

    @staticmethod
    def forward(ctx, latents, grad, clip):
        B = grad.shape[0]
        n = grad.numel() // B
        dev = grad.device
        lib = _lib()
        ctx.set_materialize_grads(False)
        nbytes = lib.sds_loss_workspace_bytes(B, n)
        wsb = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        out = torch.empty(2 + B, device=dev, dtype=torch.float32)
        lib.sds_loss_forward(grad.data_ptr(), B, n, int(clip is not None), 0.0 if clip is None else clip, out.data_ptr(), wsb.data_ptr(),
                             nbytes, torch.cuda.current_stream(dev).cuda_stream)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(wsb)
            ctx.args = (B, n, nbytes, latents.shape)
        loss, norm, each = out[0], out[1], out[2:]
        ctx.mark_non_differentiable(norm, each)
        return loss, each, norm

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, _g_each, _g_norm):
        if g_loss is None:
            return None, None, None
        (wsb,) = ctx.saved_tensors
        B, n, nbytes, shape = ctx.args
        g = g_loss.to(torch.float32).contiguous()  # (0-dim, on the device: the kernel reads it there)
        grad = torch.empty(shape, device=wsb.device, dtype=torch.float32)
        _lib().sds_loss_backward(B, n, g.data_ptr(), grad.data_ptr(), wsb.data_ptr(), nbytes, torch.cuda.current_stream(wsb.device).cuda_stream)
        return grad, None, None


def sds_loss(latents, grad, grad_clip_val=None):
    """stable_diffusion.py:298-312: with g' = clamp(nan_to_num(grad), -grad_clip_val, grad_clip_val) (the clamp only when the value
    is given) -> (loss_sds = 0.5 * sum g'^2 / B, loss_sds_each [B] = 0.5 * sum_b g'^2, grad_norm = sqrt(sum g'^2)), float32.  Only
    loss_sds is differentiable, and only with respect to latents: d loss_sds / d latents = g' / B, as the reference's
    0.5 * mse_loss(latents, (latents - g').detach(), reduction="sum") / B gives it.  `grad` is treated as detached."""
    for name, t in (("latents", latents), ("grad", grad)):
        if not isinstance(t, torch.Tensor) or t.dim() < 2:
            raise ValueError(f"gsgen_amd.guidance: {name} must be a [B, ...] tensor, got shape {tuple(getattr(t, 'shape', ())) or type(t)}")
    if latents.shape != grad.shape:
        raise ValueError(f"gsgen_amd.guidance: latents and grad differ in shape: {tuple(latents.shape)} and {tuple(grad.shape)}")
    clip = None
    if grad_clip_val is not None:
        clip = float(grad_clip_val)
        if not clip >= 0.0:
            raise ValueError(f"gsgen_amd.guidance: grad_clip_val must be a number >= 0 or None, got {grad_clip_val!r}")
    if grad.numel() == 0:
        raise ValueError(f"gsgen_amd.guidance: an empty batch or empty latents have no loss, got shape {tuple(grad.shape)}")
    if grad.shape[0] > MAX_BATCH:
        raise NotImplementedError(f"gsgen_amd.guidance: a batch of {grad.shape[0]} -- the kernels take up to {MAX_BATCH}")
    if latents.dtype != torch.float32 or grad.dtype != torch.float32:
        raise NotImplementedError(f"gsgen_amd.guidance: latents and grad must be float32, got {latents.dtype} and {grad.dtype}")
    if not latents.is_cuda or not grad.is_cuda:
        raise ValueError("gsgen_amd.guidance: latents and grad must be CUDA (HIP) tensors -- there is no CPU implementation")
    if latents.device != grad.device:
        raise ValueError("gsgen_amd.guidance: latents and grad must be on one device")
    return _SdsLoss.apply(latents, grad.detach().contiguous(), clip)
