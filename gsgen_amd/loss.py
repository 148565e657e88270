"""The image loss of the reference's image-supervised training modes on the GPU (gsgen_amd/csrc/loss.hip through the C ABI).

The reference computes it in utils/loss.py:7-47 as
    ssim_weight * kornia.losses.ssim_loss(out, gt, window_size, reduction="mean") + (1 - ssim_weight) * {mse | l1}_loss(out, gt)
(trainer.py:156, :659-680, :740; conf/renderer/legacy.yaml:46-47); kornia is five conv2d calls and some twenty elementwise kernels
forward and as many backward.  Here the forward is one pass over the two images and the backward another.  The functions below
keep the reference's names and arguments, so a trainer changes one import.  DESIGN.md ("Image loss") restates kornia 0.6.0's
definition, which the kernels follow.

Images are [B, H, W, C] or [H, W, C] float32 CUDA (HIP) tensors, channels last as the renderer delivers them (no `moveaxis`
copy); C is 1 or 3, window_size odd in 3..11, H and W at least (window_size + 1) / 2 (torch's own limit for reflect padding).
Every function returns a 0-dim tensor; autograd reaches `out` only.  The loss runs on the current stream with its workspace from
torch's caching allocator and never synchronises with the host -- the backward reads the upstream gradient from device memory --
so a forward + backward can be captured by `torch.cuda.graph` and replayed on new image values in the same tensors.  Loss and
gradient are bit-identical from run to run (no float atomics).
"""
import torch
from torch.autograd.function import once_differentiable

from . import _capi

WINDOW_MAX = 11               # gsgen_amd/csrc/loss.hip: kWsMax
_BASE = {"l2": 0, "l1": 1}    # loss.hip: kL2, kL1


def _lib():
    lib = _capi.load()
    if not hasattr(lib, "image_loss_forward"):
        raise RuntimeError(f"{lib.path} was built without the image loss kernels (gsgen_amd/csrc/loss.hip): rebuild it "
                           "(python -m gsgen_amd.build)")
    return lib


class _ImageLoss(torch.autograd.Function):
    """-> float32 [3]: total, ssim term, base term (means).  Only the total is differentiable."""

    @staticmethod
    def forward(ctx, out, gt, ws, w, base):
        B, H, W, C = out.shape
        dev = out.device
        lib = _lib()
        want_grad = bool(ctx.needs_input_grad[0])
        ctx.set_materialize_grads(False)  # (no zero tensor for the two logging terms)
        nbytes = lib.image_loss_workspace_bytes(B, H, W, C, ws, int(want_grad))
        wsb = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        loss = torch.empty(3, device=dev, dtype=torch.float32)
        lib.image_loss_forward(out.data_ptr(), gt.data_ptr(), B, H, W, C, ws, w, base, int(want_grad), loss.data_ptr(), wsb.data_ptr(),
                               nbytes, torch.cuda.current_stream(dev).cuda_stream)
        if want_grad:
            ctx.save_for_backward(out, gt, wsb)
            ctx.args = (B, H, W, C, ws, w, base, nbytes)
        total, parts = loss[0], loss[1:]
        ctx.mark_non_differentiable(parts)
        return total, parts

    @staticmethod
    @once_differentiable
    def backward(ctx, g_total, _g_parts):
        if g_total is None:
            return None, None, None, None, None
        out, gt, wsb = ctx.saved_tensors
        B, H, W, C, ws, w, base, nbytes = ctx.args
        g = g_total.to(torch.float32).contiguous()  # (0-dim, on the device: the kernel reads it there)
        grad = torch.empty_like(out)
        _lib().image_loss_backward(out.data_ptr(), gt.data_ptr(), B, H, W, C, ws, w, base, g.data_ptr(), grad.data_ptr(), wsb.data_ptr(),
                                   nbytes, torch.cuda.current_stream(out.device).cuda_stream)
        return grad, None, None, None, None


def _check(out, gt, window_size, kind):
    for name, t in (("out", out), ("gt", gt)):
        if not isinstance(t, torch.Tensor) or t.dim() not in (3, 4):
            raise ValueError(f"gsgen_amd.loss: {name} must be a [B, H, W, C] or [H, W, C] tensor, got shape "
                             f"{tuple(getattr(t, 'shape', ())) or type(t)}")
    if out.shape != gt.shape:
        raise ValueError(f"gsgen_amd.loss: out and gt differ in shape: {tuple(out.shape)} and {tuple(gt.shape)}")
    if kind not in _BASE:
        raise NotImplementedError(f"gsgen_amd.loss: type must be one of {sorted(_BASE)}, got {kind!r}")
    ws = int(window_size)
    if ws != window_size or ws < 3 or ws % 2 == 0:
        raise ValueError(f"gsgen_amd.loss: window_size must be an odd integer >= 3, got {window_size!r}")
    H, W, C = out.shape[-3:]
    p = (ws - 1) // 2
    if ws <= WINDOW_MAX and (H <= p or W <= p):
        raise ValueError(f"gsgen_amd.loss: a {H} x {W} image is too small for window_size {ws}: reflect padding by {p} needs more "
                         f"than {p} rows and columns")
    if out.dim() == 4 and out.shape[0] == 0:
        raise ValueError("gsgen_amd.loss: an empty batch has no mean")
    if C not in (1, 3):
        raise NotImplementedError(f"gsgen_amd.loss: images of {C} channels -- the kernels take 1 or 3 (channels last)")
    if ws > WINDOW_MAX:
        raise NotImplementedError(f"gsgen_amd.loss: window_size {ws} -- the kernels take 3..{WINDOW_MAX}")
    if out.dtype != torch.float32 or gt.dtype != torch.float32:
        raise NotImplementedError(f"gsgen_amd.loss: images must be float32, got {out.dtype} and {gt.dtype}")
    if gt.requires_grad:
        raise NotImplementedError("gsgen_amd.loss: gt requires a gradient -- the loss is differentiated with respect to out only")
    if not out.is_cuda or not gt.is_cuda:
        raise ValueError("gsgen_amd.loss: images must be CUDA (HIP) tensors -- there is no CPU implementation")
    if out.device != gt.device:
        raise ValueError("gsgen_amd.loss: out and gt must be on one device")
    return ws


def _run(out, gt, window_size, ssim_weight, kind):
    ws = _check(out, gt, window_size, kind)
    if out.dim() == 3:
        out, gt = out[None], gt[None]
    return _ImageLoss.apply(out.contiguous(), gt.detach().contiguous(), ws, float(ssim_weight), _BASE[kind])


def ssim_loss(img1, img2, window_size=11):
    """kornia.losses.ssim_loss(img1, img2, window_size, reduction="mean") = mean(clamp((1 - ssim) / 2, 0, 1)), for channels-last
    images (kornia takes [B, C, H, W]); the gradient goes to img1"""
    return _run(img1, img2, window_size, 1.0, "l2")[0]


def image_loss(out, gt, ssim_weight=0.2, type="l1", window_size=11):
    """ssim_weight * ssim_loss(out, gt, window_size) + (1 - ssim_weight) * (mse_loss | l1_loss)(out, gt), type "l2" | "l1"
    (the body of the closures of utils/loss.py:29-47)"""
    return _run(out, gt, window_size, ssim_weight, type)[0]


def image_loss_terms(out, gt, ssim_weight=0.2, type="l1", window_size=11):
    """-> (total, ssim_loss, base loss): the total as image_loss returns it, and its two unweighted terms for logging (float32
    0-dim, no gradient), from the same launch"""
    total, parts = _run(out, gt, window_size, ssim_weight, type)
    return total, parts[0], parts[1]


def get_image_loss(ssim_weight=0.2, type="l1"):
    """utils/loss.py:29-47: -> fn(out, gt) on [B, H, W, 3] images, window 11"""
    if type not in _BASE:  # (the reference raises NotImplementedError here too)
        raise NotImplementedError(f"gsgen_amd.loss: type must be one of {sorted(_BASE)}, got {type!r}")

    def fn(out, gt):
        return image_loss(out, gt, ssim_weight, type, 11)
    return fn


def get_loss_fn(cfg):
    """utils/loss.py:7-26: -> fn(out, gt) on [H, W, 3] images from cfg.loss_fn ("l2" | "l1"), cfg.ssim_loss_mult and
    cfg.ssim_loss_win_size"""
    if cfg.loss_fn not in _BASE:  # (the reference raises NotImplementedError here too)
        raise NotImplementedError(f"gsgen_amd.loss: cfg.loss_fn must be one of {sorted(_BASE)}, got {cfg.loss_fn!r}")
    kind, w, ws = cfg.loss_fn, float(cfg.ssim_loss_mult), int(cfg.ssim_loss_win_size)

    def fn(out, gt):
        return image_loss(out, gt, w, kind, ws)
    return fn
