"""The learned MLP background of the reference (gs/backgrounds.py:88-114, conf/renderer/mlp_bg.yaml) on the GPU, fused with its
composite (gsgen_amd/csrc/background.hip through the C ABI).

The reference builds it from tinycudann -- tcnn.NetworkWithInputEncoding(3, 3, SphericalHarmonics degree 3, FullyFusedMLP ReLU
16 x 2) -- which is CUDA only.  Here the whole chain runs per pixel in registers: ray direction from the camera block, e = 2 d - 1,
nine SH terms padded with ones to 16, two 16-wide ReLU layers without biases, three outputs, a sigmoid, nan_to_num, and -- in
`over` -- the composite rgb + (1 - opacity) bg.  DESIGN.md ("MLP background") has the definition.  It is a reading of tinycudann
that no reference run pins (the 2 d - 1 input map, the ones padding and the flat parameter layout are the points a check against
tcnn would settle), in fp32 where tcnn rounds to fp16.

`MLPBackground(cfg)` keeps the reference's names: the 768 parameters live in `self.mlp.params` (W0 | W1 | W2, each [16 out][16 in]
row-major; rows 3..15 of W2 are padding, never read, gradient exactly 0), so the reference's `bg` state dict (key `mlp.params`)
loads, and `bg(rays_d)` with rays_d [H, W, 3] is the reference's call.  `images` and `over` take the directions from per-view
camera blocks in device memory instead (gsgen_pack_camera's layout: floats 0..11 the c2w rows, 12..15 fx fy cx cy; a float32 CUDA
tensor [B, >= 16], e.g. BatchRenderer's own blocks or `camera_blocks(...)`).

Everything runs on the current stream with its workspace from torch's caching allocator and never synchronises with the host --
the backward reads the upstream gradient from device memory and RECOMPUTES the forward, nothing per-pixel is saved -- so a forward +
backward can be captured by `torch.cuda.graph`; a replay reads the parameters and the camera blocks that are in their tensors then.
The same holds eagerly: the backward reads the camera blocks as they are when it runs.  The weight gradient is summed without
float atomics: image and gradients are bit-identical from run to run.  A pixel whose network output is not finite gets bg = 0 and
contributes nothing to any gradient (torch would give NaN there).
"""
import math

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _capi

N_PARAMS = 768                      # background.hip: kParams
INIT_BOUND = math.sqrt(6.0 / 32.0)  # U(-sqrt(6 / (fan_in + fan_out)), ...) of a 16 x 16 layer


def _lib():
    lib = _capi.load()
    if not hasattr(lib, "mlp_background_forward"):
        raise RuntimeError(f"{lib.path} was built without the MLP background kernels (gsgen_amd/csrc/background.hip): rebuild it "
                           "(python -m gsgen_amd.build)")
    return lib


def _p(t):
    return None if t is None else t.data_ptr()


class _MLPBackground(torch.autograd.Function):
    """params [768]; cams [B, S >= 16] (rows S floats apart) or None; dirs [B,H,W,3] or None; rgb [B,H,W,3] and opacity [B,H,W,1] or
    both None; all float32, contiguous but for cams' row stride -> out [B,H,W,3].  Differentiable to params, rgb and opacity."""

    @staticmethod
    def forward(ctx, params, cams, dirs, rgb, opacity, B, H, W):
        dev = params.device
        lib = _lib()
        out = torch.empty(B, H, W, 3, device=dev, dtype=torch.float32)
        stride = 0 if cams is None else 4 * cams.stride(0)
        lib.mlp_background_forward(params.data_ptr(), _p(cams), stride, _p(dirs), B, H, W, _p(rgb), _p(opacity), out.data_ptr(),
                                   torch.cuda.current_stream(dev).cuda_stream)
        ctx.save_for_backward(params, cams, dirs, opacity)
        ctx.args = (B, H, W, stride)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        params, cams, dirs, opacity = ctx.saved_tensors
        B, H, W, stride = ctx.args
        dev = params.device
        lib = _lib()
        g = grad.to(torch.float32).contiguous()
        g_params = g_opacity = None
        if ctx.needs_input_grad[0] or (opacity is not None and ctx.needs_input_grad[4]):
            g_params = torch.empty(N_PARAMS, device=dev, dtype=torch.float32)
            if opacity is not None and ctx.needs_input_grad[4]:
                g_opacity = torch.empty_like(opacity)
            nbytes = lib.mlp_background_workspace_bytes(B, H, W)
            wsb = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            lib.mlp_background_backward(params.data_ptr(), _p(cams), stride, _p(dirs), B, H, W, _p(opacity), g.data_ptr(),
                                        g_params.data_ptr(), _p(g_opacity), wsb.data_ptr(), nbytes,
                                        torch.cuda.current_stream(dev).cuda_stream)
        # d out / d rgb = 1: the upstream gradient itself, no kernel
        return g_params, None, None, (grad if ctx.needs_input_grad[3] else None), g_opacity, None, None, None


def _check_params(params):
    if not isinstance(params, torch.Tensor) or params.dim() != 1 or params.shape[0] != N_PARAMS:
        raise ValueError(f"gsgen_amd.background: params must be a [{N_PARAMS}] tensor (W0 | W1 | W2, each [16, 16] row-major), got shape "
                         f"{tuple(getattr(params, 'shape', ())) or type(params)}")


def _check_cams(cams, B=None):
    if not isinstance(cams, torch.Tensor) or cams.dim() != 2 or cams.shape[1] < 16:
        raise ValueError("gsgen_amd.background: cams must be a [B, >= 16] tensor of camera blocks (floats 0..11 the c2w rows, 12..15 fx fy cx "
                         f"cy), got shape {tuple(getattr(cams, 'shape', ())) or type(cams)}")
    if B is not None and cams.shape[0] != B:
        raise ValueError(f"gsgen_amd.background: {cams.shape[0]} camera blocks for a batch of {B} images")
    if cams.stride(1) != 1 or (cams.shape[0] > 1 and cams.stride(0) < 16):
        raise ValueError(f"gsgen_amd.background: camera blocks must be contiguous rows, got strides {tuple(cams.stride())}")
    if cams.requires_grad:
        raise NotImplementedError("gsgen_amd.background: cams requires a gradient -- the background is not differentiated with respect to the camera")


def _check_devices(named):
    """dtype, then device: every shape check comes first, so CPU tensors reach each of them"""
    for name, t in named:
        if t.dtype != torch.float32:
            raise NotImplementedError(f"gsgen_amd.background: {name} must be float32, got {t.dtype}")
    for name, t in named:
        if not t.is_cuda:
            raise ValueError(f"gsgen_amd.background: {name} must be a CUDA (HIP) tensor -- there is no CPU implementation")
    for name, t in named[1:]:
        if t.device != named[0][1].device:
            raise ValueError(f"gsgen_amd.background: {named[0][0]} and {name} must be on one device")


def _check_size(B, H, W):
    if B * H * W == 0:
        raise ValueError("gsgen_amd.background: an empty batch or an empty image has no background")
    if B * H * W > 1 << 31:
        raise NotImplementedError(f"gsgen_amd.background: {B} x {H} x {W} pixels -- the kernels take up to 2^31")


def mlp_background(params, dirs):
    """bg(dirs): dirs [..., 3] ray directions, used as they are (the reference passes them unnormalised) -> [..., 3]"""
    _check_params(params)
    if not isinstance(dirs, torch.Tensor) or dirs.dim() < 1 or dirs.shape[-1] != 3:
        raise ValueError(f"gsgen_amd.background: dirs must be a [..., 3] tensor, got shape {tuple(getattr(dirs, 'shape', ())) or type(dirs)}")
    P = dirs.numel() // 3
    _check_size(1, 1, P)
    if dirs.requires_grad:
        raise NotImplementedError("gsgen_amd.background: dirs requires a gradient -- the background is not differentiated with respect to the rays")
    _check_devices((("params", params), ("dirs", dirs)))
    out = _MLPBackground.apply(params.contiguous(), None, dirs.contiguous().view(1, 1, P, 3), None, None, 1, 1, P)
    return out.view(dirs.shape)


def mlp_background_images(params, cams, H, W):
    """-> [B, H, W, 3]: the background of every pixel (x, y) of the B cameras whose blocks are the rows of cams"""
    _check_params(params)
    _check_cams(cams)
    B, H, W = cams.shape[0], int(H), int(W)
    _check_size(B, H, W)
    _check_devices((("params", params), ("cams", cams)))
    return _MLPBackground.apply(params.contiguous(), cams, None, None, None, B, H, W)


def mlp_background_over(params, rgb, opacity, cams):
    """-> rgb + (1 - opacity) * bg, one launch: rgb [B,H,W,3], opacity [B,H,W,1] or [B,H,W] (the heads render's outputs), cams [B, >= 16].
    Autograd reaches params, rgb (its gradient is the upstream gradient itself) and opacity (-sum_c g_c bg_c)."""
    _check_params(params)
    if not isinstance(rgb, torch.Tensor) or rgb.dim() != 4 or rgb.shape[-1] != 3:
        raise ValueError(f"gsgen_amd.background: rgb must be a [B, H, W, 3] tensor, got shape {tuple(getattr(rgb, 'shape', ())) or type(rgb)}")
    B, H, W = rgb.shape[:3]
    if not isinstance(opacity, torch.Tensor) or tuple(opacity.shape) not in ((B, H, W, 1), (B, H, W)):
        raise ValueError(f"gsgen_amd.background: opacity must be [B, H, W, 1] or [B, H, W] like rgb {tuple(rgb.shape)}, got shape "
                         f"{tuple(getattr(opacity, 'shape', ())) or type(opacity)}")
    _check_cams(cams, B)
    _check_size(B, H, W)
    _check_devices((("params", params), ("rgb", rgb), ("opacity", opacity), ("cams", cams)))
    return _MLPBackground.apply(params.contiguous(), cams, None, rgb.contiguous(), opacity.contiguous().view(B, H, W, 1), B, H, W)


def camera_blocks(c2w, intrinsics, device=None):
    """[B, 16] float32 camera blocks for a stand-alone caller: c2w [B, 3 | 4, 4] poses, intrinsics [B, 4] = fx fy cx cy or B
    CameraInfo-like objects (fx, fy, cx, cy); tensors or arrays.  On `device` (default: c2w's, if it is a tensor)."""
    if device is None and isinstance(c2w, torch.Tensor):
        device = c2w.device
    c2w = torch.as_tensor(np.asarray(c2w.detach().cpu()) if isinstance(c2w, torch.Tensor) else np.asarray(c2w, np.float32)).float()
    if c2w.dim() != 3 or c2w.shape[1] not in (3, 4) or c2w.shape[2] != 4:
        raise ValueError(f"gsgen_amd.background: c2w must be [B, 3 | 4, 4], got shape {tuple(c2w.shape)}")
    B = c2w.shape[0]
    if not isinstance(intrinsics, (torch.Tensor, np.ndarray)):
        intrinsics = np.asarray([[ci.fx, ci.fy, ci.cx, ci.cy] for ci in intrinsics], np.float32)
    intr = torch.as_tensor(np.asarray(intrinsics.detach().cpu()) if isinstance(intrinsics, torch.Tensor) else intrinsics).float()
    if tuple(intr.shape) != (B, 4):
        raise ValueError(f"gsgen_amd.background: intrinsics must be [{B}, 4] = fx fy cx cy, got shape {tuple(intr.shape)}")
    blocks = torch.cat((c2w[:, :3, :].reshape(B, 12), intr), 1).contiguous()
    return blocks if device is None else blocks.to(device)


def _get(cfg, key, default=None):
    if cfg is None:
        return default
    if hasattr(cfg, "get"):
        try:
            return cfg.get(key, default)
        except Exception:
            pass
    return getattr(cfg, key, default)


class _Params(nn.Module):
    """stands where the reference has the tcnn module: one flat parameter vector `params`"""

    def __init__(self, generator=None):
        super().__init__()
        self.params = nn.Parameter((torch.rand(N_PARAMS, generator=generator) * 2.0 - 1.0) * INIT_BOUND)


class MLPBackground(nn.Module):
    """gs/backgrounds.py:88-114.  cfg: the `background` node of conf/renderer/mlp_bg.yaml (type, device; random_aug is refused).
    The parameters are drawn U(-sqrt(6/32), sqrt(6/32)) from torch's CPU generator (torch.manual_seed seeds it; or pass one)."""

    type = "mlp"

    def __init__(self, cfg=None, generator=None):
        super().__init__()
        if bool(_get(cfg, "random_aug", False)):
            raise NotImplementedError("gsgen_amd.background: random_aug with background.type 'mlp' -- the fused composite draws one learned "
                                      "colour per pixel and has no per-camera random replacement (conf/renderer/mlp_bg.yaml does not use it)")
        self.cfg = cfg
        self.mlp = _Params(generator)
        dev = _get(cfg, "device")
        if dev is not None:
            self.to(dev)

    def forward(self, dirs):
        """the reference's call bg(rays_d): dirs [H, W, 3] (any [..., 3]) -> the same shape"""
        return mlp_background(self.mlp.params, dirs)

    def images(self, cams, B, H, W):
        """-> [B, H, W, 3] for the first B camera blocks of cams"""
        _check_cams(cams)
        return mlp_background_images(self.mlp.params, cams[:int(B)], H, W)

    def over(self, rgb, opacity, cams):
        """-> rgb + (1 - opacity) * bg: the fused composite behind a heads render (one camera block per image)"""
        return mlp_background_over(self.mlp.params, rgb, opacity, cams)
