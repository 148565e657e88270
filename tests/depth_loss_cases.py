"""The Pearson depth loss of gsgen_amd.loss restated in torch ops, and the cases its tests share (tests/test_depth_loss_host.py on
the CPU emulator, tests/test_gpu_depth_loss.py on the GPU).

`depth_loss_torch` is the oracle: the loop of the reference's utils/loss.py:50-66 with torchmetrics' PearsonCorrCoef written out as
the centred two-pass formula (mean, then the sums of the centred products) in plain torch ops, autograd for the gradients, and the
degenerate images handled as DESIGN.md ("Depth loss") defines them.  It shares no code with the kernel
(gsgen_amd/csrc/depth_loss.hip).  `nan_to_num` is applied to the fp32 values before any conversion.  Run in fp64 it is the truth, run
in fp32 it is what a user composes from torch ops, and its fp32 error sets the kernel's accuracy bound (`check_bound`): no fixed
tolerance.

The kernel reduces an image in chunks of 4096 pixels, one workgroup each (depth_loss.hip: kChunk), so the shape at which an image
spans several workgroups is (1, 160, 200): 32 000 pixels, eight workgroups, the last one partial.
"""
import functools

import numpy as np
import torch

KCHUNK = 4096  # depth_loss.hip: kChunk (tests/test_depth_loss_host.py checks it against the compiled file)


def depth_loss_torch(x, y, mask=None):
    """x [B,H,W] (already through nan_to_num), y [B,H,W] or [1,H,W], one dtype; mask bool [B,H,W] or [1,H,W] or None
    -> (the 0-dim loss, corr [B] detached: NaN for a degenerate image)"""
    B = x.shape[0]
    loss = torch.zeros((), dtype=x.dtype, device=x.device)
    corr = []
    for b in range(B):
        xb, yb = x[b], y[b if y.shape[0] == B else 0]
        if mask is not None:
            m = mask[b if mask.shape[0] == B else 0]
            xb, yb = xb[m], yb[m]
        xb, yb = xb.reshape(-1), yb.reshape(-1)
        n = xb.numel()
        if n < 2 or bool((xb == xb[0]).all()) or bool((yb == yb[0]).all()):  # degenerate: r = 0, no gradient
            loss = loss + 1
            corr.append(torch.full((), float("nan"), dtype=x.dtype, device=x.device))
            continue
        dx, dy = xb - xb.sum() / n, yb - yb.sum() / n
        r = torch.clamp((dx * dy).sum() / torch.sqrt((dx * dx).sum() * (dy * dy).sum()), -1, 1)
        loss = loss + (1 - r)
        corr.append(r.detach())
    return loss / B, torch.stack(corr)


def reference_depth_loss(pred, gt, mask, dtype, scale=1.0):
    """pred [B,H,W], gt [B,H,W] or [1,H,W] float32 arrays, mask a bool array or None -> (loss as a Python float, d loss / d pred,
    d loss / d gt as float64 arrays of the inputs' shapes, corr [B] float64), on the CPU in `dtype`.  The gradient to pred is zero
    where pred was not finite, as torch.nan_to_num's backward makes it."""
    p32 = torch.as_tensor(np.asarray(pred))
    x = torch.nan_to_num(p32).to(dtype).requires_grad_(True)  # (sanitised in fp32, then converted exactly)
    y = torch.as_tensor(np.asarray(gt)).to(dtype).requires_grad_(True)
    m = None if mask is None else torch.as_tensor(np.asarray(mask)).bool()
    L, corr = depth_loss_torch(x, y, m)
    if L.requires_grad:
        (scale * L).backward()
    gx = torch.zeros_like(x) if x.grad is None else x.grad
    gy = torch.zeros_like(y) if y.grad is None else y.grad
    gx = gx * torch.isfinite(p32)
    return float(L.item()), gx.double().numpy(), gy.double().numpy(), corr.double().numpy()


# (B, H, W): the smallest sizes at which each mechanism can break
S2, S35, S1961, S4096, S32000 = (1, 1, 2), (2, 5, 7), (2, 37, 53), (3, 64, 64), (1, 160, 200)
# name -> (values, (B, H, W), mask kind, shared gt)
_LIST = [
    ("exact2", S2, "none", False),        # n = 2: r = +1 exactly
    ("exact2anti", S2, "none", False),    # r = -1 exactly
    ("affine", S35, "none", False),       # less than one wave
    ("affine", S35, "rand70", False),
    ("affine", S1961, "none", False),     # a multiple of nothing
    ("affine", S1961, "rand70", False),
    ("affine", S4096, "none", False),     # a multiple of everything: one full workgroup per image
    ("affine", S4096, "rand70", False),
    ("affine", S32000, "none", False),    # eight workgroups per image, the last partial
    ("affine", S32000, "rand70", False),
    ("near", S1961, "rand70", False),
    ("near", S32000, "none", False),
    ("anti", S35, "none", False),
    ("anti", S4096, "rand70", False),
    ("offset100", S35, "none", False),    # the cancellation case
    ("offset100", S1961, "none", False),
    ("offset100", S4096, "rand70", False),
    ("offset100", S32000, "rand70", False),
    ("nans", S35, "rand70", False),       # a few scattered NaN pixels in pred
    ("nans", S1961, "none", False),
    ("nans", S32000, "rand70", False),
    ("constpred", S1961, "none", False),  # pred = 0.9f everywhere: degenerate whatever P is
    ("constpred", S4096, "none", False),
    ("constpred", S32000, "rand70", False),
    ("constgt", S35, "none", False),
    ("constgt", S1961, "rand70", False),
    ("constgt", S32000, "none", False),
    ("allnan", S1961, "none", False),     # what the renderer emits for a camera whose pair list overflowed
    ("onenan", S1961, "rand70", False),   # ... for one view of a batch of two
    ("affine", S1961, "two", False),      # exactly two true pixels, the first and the last of the image
    ("affine", S32000, "two", False),     # ... in two different workgroups
    ("offset100", S1961, "two", False),
    ("affine", S1961, "onefalse", False),  # all false in one image of a batch of two
    ("affine", S4096, "sharedmask", False),
    ("affine", S4096, "rand70", True),    # one gt shared by the batch
    ("offset100", S1961, "sharedmask", True),
    ("nans", S4096, "none", True),
]


def _name(values, shape, mask, shared_gt):
    return f"{values}-{shape[0]}x{shape[1]}x{shape[2]}-{mask}" + ("-sharedgt" if shared_gt else "")


CASES = {_name(*c): c + (300 + i,) for i, c in enumerate(_LIST)}
NAMES = sorted(CASES)
assert len(CASES) == len(_LIST)


def make_depths(values, B, H, W, seed, shared_gt=False):
    """-> (pred [B,H,W], gt [B,H,W] or [1,H,W]) float32"""
    gen = torch.Generator().manual_seed(seed)
    if values in ("exact2", "exact2anti"):
        assert (B, H, W) == (1, 1, 2)
        gt = torch.tensor([[[2.0, 6.0]]] if values == "exact2" else [[[6.0, 2.0]]])
        return torch.tensor([[[1.0, 3.0]]]).numpy(), gt.numpy()
    Bg = 1 if shared_gt else B
    yy, xx = torch.meshgrid(torch.linspace(0, 3, H, dtype=torch.float64), torch.linspace(0, 3, W, dtype=torch.float64), indexing="ij")
    offset = 100.0 if values == "offset100" else 3.0
    gt = offset + torch.sin(2 * xx + yy)[None] + 0.3 * torch.rand(Bg, H, W, generator=gen, dtype=torch.float64)  # depth-like, spread ~ 0.7
    noise = torch.randn(B, H, W, generator=gen, dtype=torch.float64)
    sy = gt.std().item()
    if values in ("affine", "offset100", "nans", "onenan", "constgt"):
        pred = 0.5 * gt + (offset - 2.0) + 0.5 * sy * 0.484 * noise  # r ~ 0.9
    elif values == "near":
        pred = 0.5 * gt + 1.0 + 0.01 * noise
    elif values == "anti":
        pred = -0.5 * gt + 6.0 + 0.5 * sy * 0.484 * noise
    elif values == "constpred":
        pred = torch.full((B, H, W), 0.9, dtype=torch.float64)
    elif values == "allnan":
        pred = torch.full((B, H, W), float("nan"), dtype=torch.float64)
    else:
        raise ValueError(values)
    pred = pred.expand(B, H, W).clone()
    if values == "nans":
        hit = torch.rand(B, H, W, generator=gen) < max(0.01, 3.0 / (H * W))
        hit.view(-1)[1] = True
        pred[hit] = float("nan")
    if values == "onenan":
        pred[1] = float("nan")
    if values == "constgt":
        gt = torch.full((Bg, H, W), 2.5, dtype=torch.float64)
    return pred.float().numpy(), gt.float().numpy()


def make_mask(kind, B, H, W, seed):
    """-> a bool array [B,H,W] or [1,H,W], or None"""
    gen = torch.Generator().manual_seed(seed + 5000)
    if kind == "none":
        return None
    if kind in ("rand70", "onefalse"):
        m = torch.rand(B, H, W, generator=gen) < 0.7
        if kind == "onefalse":
            m[1] = False
    elif kind == "sharedmask":
        m = torch.rand(1, H, W, generator=gen) < 0.7
    elif kind == "two":
        m = torch.zeros(B, H, W, dtype=torch.bool)
        m[:, 0, 0] = True
        m[:, -1, -1] = True
    else:
        raise ValueError(kind)
    return m.numpy()


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(pred, gt, mask, L64, gp64, gg64, c64, L32, gp32, gg32, c32): the inputs (arrays, not to be written to) and the
    restatement's results in fp64 (the truth) and fp32 (its own error is the yardstick), computed once per process"""
    values, (B, H, W), mkind, shared_gt, seed = CASES[name]
    pred, gt = make_depths(values, B, H, W, seed, shared_gt)
    mask = make_mask(mkind, B, H, W, seed)
    L64, gp64, gg64, c64 = reference_depth_loss(pred, gt, mask, torch.float64)
    L32, gp32, gg32, c32 = reference_depth_loss(pred, gt, mask, torch.float32)
    for arr in (pred, gt, mask, gp64, gg64, c64, gp32, gg32, c32):
        if arr is not None:
            arr.setflags(write=False)
    return dict(values=values, pred=pred, gt=gt, mask=mask, L64=L64, gp64=gp64, gg64=gg64, c64=c64, L32=L32, gp32=gp32, gg32=gg32, c32=c32)


FLOOR = 2.0 ** -22  # four ulps at 1: the loss is 1 - r with |r| <= 1


def bound_report(name, L, gp=None, gg=None, scale=1.0):
    """-> ([(what, error, bound), ...], a line for the log).  The bounds: 4 x the fp32 restatement's own error against fp64, floored at
    2^-22 for the loss (relative to 1) and at 2^-22 of the largest entry for each gradient tensor.  `scale`: the upstream scalar the
    gradients were taken with (the restatement's are linear in it)."""
    c = case(name)
    rows = [("L", abs(float(L) - c["L64"]), 4 * max(abs(c["L32"] - c["L64"]), FLOOR), abs(c["L32"] - c["L64"]))]
    for what, g, g64, g32 in (("gpred", gp, c["gp64"], c["gp32"]), ("ggt", gg, c["gg64"], c["gg32"])):
        if g is None:
            continue
        g = np.asarray(g, np.float64).reshape(g64.shape)
        e32 = scale * np.abs(g32 - g64).max()
        rows.append((what, np.abs(g - scale * g64).max(), 4 * max(e32, FLOOR * scale * np.abs(g64).max()), e32))
    line = f"{name}: L64 {c['L64']:.9f} " + " ".join(f"{w}: err {e:.2e} (fp32 torch {e32:.2e}, bound {b:.2e})" for w, e, b, e32 in rows)
    return [r[:3] for r in rows], line


def check_bound(name, L, gp=None, gg=None, scale=1.0):
    rows, line = bound_report(name, L, gp, gg, scale)
    print(line)
    assert np.isfinite(float(L)), line
    for g in (gp, gg):
        assert g is None or np.isfinite(np.asarray(g)).all(), line
    for what, err, bound in rows:
        assert err <= bound, (what, line)


def check_corr(name, corr):
    """the per-image correlations: NaN exactly where the restatement finds the image degenerate, else within the loss's bound"""
    c = case(name)
    corr = np.asarray(corr, np.float64)
    assert corr.shape == c["c64"].shape
    assert (np.isnan(corr) == np.isnan(c["c64"])).all(), (name, corr, c["c64"])
    live = ~np.isnan(c["c64"])
    if live.any():
        e32 = np.abs(c["c32"][live] - c["c64"][live]).max()
        assert np.abs(corr[live] - c["c64"][live]).max() <= 4 * max(e32, FLOOR), (name, corr, c["c64"])
