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

The depth loss of the image-conditioned step (utils/loss.py:50-66) is here too: `depth_loss` with the reference's signature,
`pearson_depth_loss` and `pearson_depth_loss_terms` (gsgen_amd/csrc/depth_loss.hip; see the section further down).  It is capturable
in the same way, with the mask as data, and differentiates with respect to both depth maps.

The regularisers of the text-to-3D step on the rendered opacity and z_var maps (trainer.py:345-382) are the last section:
`map_loss`, `map_loss_terms`, `sparsity_loss`, `opague_loss`, `z_var_loss` and `get_map_loss` (gsgen_amd/csrc/map_loss.hip).
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


# --- the Pearson depth loss (gsgen_amd/csrc/depth_loss.hip) ------------------------------------------------------------------
# utils/loss.py:50-66, called at trainer.py:424-440 and :659-689: (1 / B) sum_b (1 - pearson(nan_to_num(pred_b)[m_b], gt_b[m_b])),
# there a Python loop with a boolean gather per image (a host synchronisation) on top of torchmetrics.  Here: two launches forward,
# one backward, no host synchronisation, capturable with the mask as data.  DESIGN.md ("Depth loss") has the definition and its one
# deliberate difference: a degenerate image (fewer than two masked pixels, or all masked values of pred or of gt equal) contributes
# 1 and a zero gradient where torchmetrics returns NaN; the per-image correlation reports NaN for it.
def _depth_lib():
    lib = _capi.load()
    if not hasattr(lib, "depth_loss_forward"):
        raise RuntimeError(f"{lib.path} was built without the depth loss kernels (gsgen_amd/csrc/depth_loss.hip): rebuild it "
                           "(python -m gsgen_amd.build)")
    return lib


class _DepthLoss(torch.autograd.Function):
    """pred [B,H,W], gt [B,H,W] or [1,H,W], mask uint8 [B,H,W] or [1,H,W] or None, all contiguous -> (loss 0-dim, corr [B]).
    Only the loss is differentiable, to pred and gt."""

    @staticmethod
    def forward(ctx, pred, gt, mask):
        B, P = pred.shape[0], pred.shape[1] * pred.shape[2]
        dev = pred.device
        lib = _depth_lib()
        ctx.set_materialize_grads(False)
        gt_stride = P if gt.shape[0] == B else 0   # (a batch of one against a batch of one: either)
        mask_stride = 0 if mask is None or mask.shape[0] != B else P
        nbytes = lib.depth_loss_workspace_bytes(B, P)
        wsb = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        loss = torch.empty(1 + B, device=dev, dtype=torch.float32)
        lib.depth_loss_forward(pred.data_ptr(), gt.data_ptr(), gt_stride, mask.data_ptr() if mask is not None else None, mask_stride, B, P,
                               loss.data_ptr(), wsb.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream)
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            ctx.save_for_backward(pred, gt, wsb, *(() if mask is None else (mask,)))
            ctx.args = (B, P, gt_stride, mask_stride, nbytes)
        total, corr = loss[0], loss[1:]
        ctx.mark_non_differentiable(corr)
        return total, corr

    @staticmethod
    @once_differentiable
    def backward(ctx, g_total, _g_corr):
        if g_total is None:
            return None, None, None
        pred, gt, wsb, *rest = ctx.saved_tensors
        mask = rest[0] if rest else None
        B, P, gt_stride, mask_stride, nbytes = ctx.args
        g = g_total.to(torch.float32).contiguous()  # (0-dim, on the device: the kernel reads it there)
        grad_pred = torch.empty_like(pred) if ctx.needs_input_grad[0] else None
        grad_gt = torch.empty_like(gt) if ctx.needs_input_grad[1] else None
        _depth_lib().depth_loss_backward(pred.data_ptr(), gt.data_ptr(), gt_stride, mask.data_ptr() if mask is not None else None,
                                         mask_stride, B, P, g.data_ptr(), grad_pred.data_ptr() if grad_pred is not None else None,
                                         grad_gt.data_ptr() if grad_gt is not None else None, wsb.data_ptr(), nbytes,
                                         torch.cuda.current_stream(pred.device).cuda_stream)
        return grad_pred, grad_gt, None


def _depth_images(name, t):
    """-> t as [B, H, W]: [B,H,W,1] and [B,H,W] keep their batch; [H,W,1] and [H,W] are a batch of one (a 3-dim tensor whose last
    size is 1 is read as [H,W,1])"""
    if not isinstance(t, torch.Tensor) or t.dim() not in (2, 3, 4):
        raise ValueError(f"gsgen_amd.loss: {name} must be a [B, H, W, 1], [B, H, W], [H, W, 1] or [H, W] tensor, got shape "
                         f"{tuple(getattr(t, 'shape', ())) or type(t)}")
    if t.dim() == 4:
        if t.shape[-1] != 1:
            raise ValueError(f"gsgen_amd.loss: {name} must have one channel, got shape {tuple(t.shape)}")
        return t[..., 0]
    if t.dim() == 3:
        return t[..., 0][None] if t.shape[-1] == 1 else t
    return t[None]


def _check_depth(pred_depth, depth_gt, mask):
    """-> (pred [B,H,W], gt [B,H,W] or [1,H,W], mask [B,H,W] or [1,H,W] or None): views, nothing copied"""
    pred, gt = _depth_images("pred_depth", pred_depth), _depth_images("depth_gt", depth_gt)
    B, H, W = pred.shape
    if gt.shape[1:] != (H, W) or gt.shape[0] not in (1, B):
        raise ValueError(f"gsgen_amd.loss: pred_depth and depth_gt differ in shape: {tuple(pred_depth.shape)} and {tuple(depth_gt.shape)} "
                         "(depth_gt may have a batch of one, or none, against a batched pred_depth)")
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dim() not in (2, 3):
            raise ValueError(f"gsgen_amd.loss: mask must be a [B, H, W] or [H, W] tensor, got shape "
                             f"{tuple(getattr(mask, 'shape', ())) or type(mask)}")
        if mask.dim() == 2:
            mask = mask[None]
        if mask.shape[1:] != (H, W) or mask.shape[0] not in (1, B):
            raise ValueError(f"gsgen_amd.loss: a mask of shape {tuple(mask.shape)} does not fit depth images of shape {(B, H, W)}")
        if mask.dtype not in (torch.bool, torch.uint8):
            raise NotImplementedError(f"gsgen_amd.loss: mask must be bool or uint8, got {mask.dtype}")
    if B == 0 or H * W == 0:
        raise ValueError("gsgen_amd.loss: an empty batch or an empty image has no correlation")
    if B > 65535:
        raise NotImplementedError(f"gsgen_amd.loss: a batch of {B} depth images -- the kernels take up to 65535")
    if pred.dtype != torch.float32 or gt.dtype != torch.float32:
        raise NotImplementedError(f"gsgen_amd.loss: depth images must be float32, got {pred.dtype} and {gt.dtype}")
    tensors = (pred, gt) if mask is None else (pred, gt, mask)
    if not all(t.is_cuda for t in tensors):
        raise ValueError("gsgen_amd.loss: depth images and mask must be CUDA (HIP) tensors -- there is no CPU implementation")
    if any(t.device != pred.device for t in tensors):
        raise ValueError("gsgen_amd.loss: pred_depth, depth_gt and mask must be on one device")
    return pred, gt, mask


def pearson_depth_loss_terms(pred_depth, depth_gt, mask=None):
    """-> (loss, corr [B]): the loss as pearson_depth_loss returns it and every image's Pearson correlation (float32, no gradient,
    NaN for a degenerate image), from the same launch"""
    pred, gt, mask = _check_depth(pred_depth, depth_gt, mask)
    B = pred.shape[0]
    if gt.shape[0] != B and gt.requires_grad:
        gt = gt.expand(B, -1, -1)  # (made contiguous below: autograd sums the batch's gradients onto the one image)
    if mask is not None:
        mask = mask.detach().contiguous()
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)  # (the same bytes: a captured replay reads the caller's mask)
    return _DepthLoss.apply(pred.contiguous(), gt.contiguous(), mask)


def pearson_depth_loss(pred_depth, depth_gt, mask=None):
    """(1 / B) sum_b (1 - r_b), r_b the Pearson correlation of nan_to_num(pred_depth[b]) and depth_gt[b] over the pixels where
    mask[b] is true (all, without a mask), clamped to [-1, 1]; 0-dim float32.  Depth images are [B,H,W,1], [B,H,W], [H,W,1] or [H,W]
    float32; depth_gt and mask ([B,H,W] or [H,W], bool or uint8) may have a batch of one, or none, against a batched pred_depth and
    are then shared by stride, not copied.  Autograd reaches pred_depth and depth_gt, whichever requires a gradient (utils/loss.py's
    callers pass the rendered depth on either side: trainer.py:432, :683)."""
    return pearson_depth_loss_terms(pred_depth, depth_gt, mask)[0]


def depth_loss(pearson, pred_depth, depth_gt, mask=None):
    """utils/loss.py:50-66 with its signature: `pearson` (there a torchmetrics.PearsonCorrCoef) is ignored and may be None"""
    return pearson_depth_loss(pred_depth, depth_gt, mask)


# --- the map regularisers (gsgen_amd/csrc/map_loss.hip) -------------------------------------------------------------------------
# trainer.py:345-382: sparsity = mean(sqrt(opacity^2 + 0.01)), opague = binary_cross_entropy(c, c) with c = clamp(opacity, 1e-3,
# 1 - 1e-3) (utils/ops.py:51-55) and z_var = mean(z_var / c * (c > 0.5)), each times a scheduled weight, there some twenty torch
# launches forward and as many backward.  Here: two launches forward, one backward, no host synchronisation, capturable, and with
# the weights in a device tensor a replay takes the next step's weights.  DESIGN.md ("Map regularisers") has the definition.
_MAP_TERMS = ("sparsity", "opague", "z_var")


def _map_lib():
    lib = _capi.load()
    if not hasattr(lib, "map_loss_forward"):
        raise RuntimeError(f"{lib.path} was built without the map regulariser kernels (gsgen_amd/csrc/map_loss.hip): rebuild it "
                           "(python -m gsgen_amd.build)")
    return lib


class _MapLoss(torch.autograd.Function):
    """opacity, z_var (or None): contiguous float32 maps of one shape; mask: the terms' bits; w_host: three floats; weights: float32
    [3] on the device or None -> (total 0-dim, terms [3]).  Only the total is differentiable, to opacity and z_var."""

    @staticmethod
    def forward(ctx, opacity, z_var, mask, w_host, weights):
        P = opacity.numel()
        dev = opacity.device
        lib = _map_lib()
        ctx.set_materialize_grads(False)
        nbytes = lib.map_loss_workspace_bytes(P)
        wsb = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        loss = torch.empty(4, device=dev, dtype=torch.float32)
        wh = (_capi.f32 * 3)(*w_host)
        lib.map_loss_forward(opacity.data_ptr(), z_var.data_ptr() if z_var is not None else None, P, mask, wh,
                             weights.data_ptr() if weights is not None else None, loss.data_ptr(), wsb.data_ptr(), nbytes,
                             torch.cuda.current_stream(dev).cuda_stream)
        if ctx.needs_input_grad[0] or (z_var is not None and ctx.needs_input_grad[1]):
            ctx.save_for_backward(opacity, wsb, *(() if z_var is None else (z_var,)), *(() if weights is None else (weights,)))
            ctx.args = (P, mask, w_host, nbytes, z_var is not None, weights is not None)
        total, terms = loss[0], loss[1:]
        ctx.mark_non_differentiable(terms)
        return total, terms

    @staticmethod
    @once_differentiable
    def backward(ctx, g_total, _g_terms):
        if g_total is None:
            return None, None, None, None, None
        P, mask, w_host, nbytes, has_z, has_w = ctx.args
        opacity, wsb, *rest = ctx.saved_tensors
        z_var = rest.pop(0) if has_z else None
        weights = rest.pop(0) if has_w else None
        g = g_total.to(torch.float32).contiguous()  # (0-dim, on the device: the kernel reads it there)
        grad_o = torch.empty_like(opacity) if ctx.needs_input_grad[0] else None
        grad_z = torch.empty_like(z_var) if has_z and ctx.needs_input_grad[1] else None
        wh = (_capi.f32 * 3)(*w_host)
        _map_lib().map_loss_backward(opacity.data_ptr(), z_var.data_ptr() if has_z else None, P, mask, wh,
                                     weights.data_ptr() if has_w else None, g.data_ptr(),
                                     grad_o.data_ptr() if grad_o is not None else None, grad_z.data_ptr() if grad_z is not None else None,
                                     wsb.data_ptr(), nbytes, torch.cuda.current_stream(opacity.device).cuda_stream)
        return grad_o, grad_z, None, None, None


def _check_maps(opacity, z_var, w_host, weights):
    """-> (opacity, z_var or None as [B,H,W] views, the terms' bit mask): nothing copied"""
    o = _depth_images("opacity", opacity)
    z = None if z_var is None else _depth_images("z_var", z_var)
    if z is not None and z.shape != o.shape:
        raise ValueError(f"gsgen_amd.loss: opacity and z_var differ in shape: {tuple(opacity.shape)} and {tuple(z_var.shape)}")
    if weights is None:
        mask = sum(1 << k for k in range(3) if w_host[k] != 0)
        if mask & 4 and z is None:
            raise ValueError("gsgen_amd.loss: a z_var weight without z_var: z_var not in output, should turn off the `rgb_only` flag")
    else:
        if not isinstance(weights, torch.Tensor) or tuple(weights.shape) != (3,):
            raise ValueError(f"gsgen_amd.loss: weights must be a float32 [3] tensor (sparsity, opague, z_var), got "
                             f"{tuple(getattr(weights, 'shape', ())) or type(weights)}")
        if weights.dtype != torch.float32:
            raise NotImplementedError(f"gsgen_amd.loss: weights must be float32, got {weights.dtype}")
        if weights.requires_grad:
            raise NotImplementedError("gsgen_amd.loss: weights require a gradient -- the loss is differentiated with respect to the maps only")
        mask = 3 if z is None else 7
    if o.numel() == 0:
        raise ValueError("gsgen_amd.loss: an empty map has no mean")
    if o.numel() >= 2 ** 32:
        raise NotImplementedError(f"gsgen_amd.loss: maps of {o.numel()} pixels -- the kernels take fewer than 2^32")
    if o.dtype != torch.float32 or (z is not None and z.dtype != torch.float32):
        raise NotImplementedError(f"gsgen_amd.loss: maps must be float32, got {o.dtype}" + ("" if z is None else f" and {z.dtype}"))
    tensors = [t for t in (o, z, weights) if t is not None]
    if not all(t.is_cuda for t in tensors):
        raise ValueError("gsgen_amd.loss: opacity, z_var and weights must be CUDA (HIP) tensors -- there is no CPU implementation")
    if any(t.device != o.device for t in tensors):
        raise ValueError("gsgen_amd.loss: opacity, z_var and weights must be on one device")
    return o, z, mask


def map_loss_terms(opacity, z_var=None, sparsity=0.0, opague=0.0, z_var_weight=0.0, weights=None):
    """-> (total, terms [3]): total = sparsity * T_s + opague * T_o + z_var_weight * T_z and the three unweighted means (float32, no
    gradient) from the same launch:
        T_s = mean(sqrt(opacity^2 + 0.01)),  T_o = mean(-(c log c + (1 - c) log(1 - c))),  T_z = mean(z_var / c * (c > 0.5)),
    c = clamp(opacity, 1e-3, 1 - 1e-3) (trainer.py:345-382).  The maps are [B,H,W,1], [B,H,W], [H,W,1] or [H,W] float32 of one shape.
    A term whose weight is 0 is not evaluated and reports 0 (the reference's `> 0.0` tests).  With `weights`, a float32 [3] device
    tensor, the three Python numbers are ignored, every term whose map is present is evaluated and the weights are read on the device:
    a captured forward + backward replays with the values then in that tensor.  Autograd reaches opacity and z_var, whichever
    requires a gradient."""
    w_host = (float(sparsity), float(opague), float(z_var_weight))
    o, z, mask = _check_maps(opacity, z_var, w_host, weights)
    if not o.is_contiguous():
        o = o.contiguous()
    if z is not None:
        if not mask & 4:
            z = None  # (not read)
        elif not z.is_contiguous():
            z = z.contiguous()
    return _MapLoss.apply(o, z, mask, w_host, None if weights is None else weights.detach())


def map_loss(opacity, z_var=None, sparsity=0.0, opague=0.0, z_var_weight=0.0, weights=None):
    """the total of map_loss_terms (0-dim float32)"""
    return map_loss_terms(opacity, z_var, sparsity, opague, z_var_weight, weights)[0]


def sparsity_loss(opacity):
    """trainer.py:349: (opacity ** 2 + 0.01).sqrt().mean()"""
    return map_loss_terms(opacity, sparsity=1.0)[0]


def opague_loss(opacity):
    """trainer.py:361-362: binary_cross_entropy(c, c) with c = opacity.clamp(1e-3, 1 - 1e-3)"""
    return map_loss_terms(opacity, opague=1.0)[0]


def z_var_loss(z_var, opacity):
    """trainer.py:374-377: (z_var / c * (c > 0.5)).mean() with c = opacity.clamp(1e-3, 1 - 1e-3)"""
    return map_loss_terms(opacity, z_var, z_var_weight=1.0)[0]


def get_map_loss(cfg_loss, max_steps=None):
    """trainer.py:345-382: -> fn(out, step) -> (loss, {"sparsity", "opague", "z_var"}) from cfg_loss.sparsity, .opague and .z_var (numbers
    or the reference's scheduled lists, evaluated per step by gsgen_amd.model.schedule_value) on out["opacity"] and out["z_var"] of the
    model's dict.  Every value returned is a 0-dim device tensor (the three terms unweighted, for the writer): nothing is read back."""
    from .model import _get, schedule_value
    specs = [_get(cfg_loss, k, 0.0) for k in _MAP_TERMS]

    def fn(out, step):
        w = [schedule_value(0.0 if s is None else s, step, max_steps) for s in specs]
        if not any(w):
            zero = torch.zeros((), dtype=torch.float32, device=next(iter(out.values())).device)
            return zero, dict.fromkeys(_MAP_TERMS, zero)
        if "opacity" not in out:
            raise ValueError("gsgen_amd.loss: opacity not in output, should turn off the `rgb_only` flag")
        total, terms = map_loss_terms(out["opacity"], out.get("z_var"), w[0], w[1], w[2])
        return total, {k: terms[i] for i, k in enumerate(_MAP_TERMS)}
    return fn
