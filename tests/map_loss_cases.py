"""The map regularisers of gsgen_amd.loss restated in torch ops, and the cases their tests share (tests/test_map_loss_host.py on the
CPU emulator, tests/test_gpu_map_loss.py on the GPU).

`map_loss_torch` is the oracle: the three expressions of the reference's trainer.py:345-382 (with utils/ops.py:51-55 for
binary_cross_entropy) in plain torch ops, autograd for the gradients.  It shares no code with the kernel
(gsgen_amd/csrc/map_loss.hip).  The constants are the fp32 values torch's fp32 ops use, converted exactly, so the fp64 run is the
truth about the SAME function: a double 0.999 as the upper bound would flip the clamp's gradient mask at opacity == float32(0.999).
Run in fp64 it is the truth, run in fp32 it is what a user composes from torch ops, and its fp32 error sets the kernel's accuracy
bound (`check_bound`): no fixed tolerance.

The kernel reduces the batch in chunks of 2048 pixels, one workgroup each (map_loss.hip: kChunk), and its final stage sweeps 256
partials at a time (kThreads); the shapes below are derived from the two.
"""
import functools

import numpy as np
import torch

KCHUNK = 2048  # map_loss.hip: kChunk (tests/test_map_loss_host.py checks both against the compiled file)
KSWEEP = 256   # map_loss.hip: kThreads, the partials one final-stage sweep covers

LO = float(np.float32(1e-3))        # what torch.clamp compares fp32 values with
HI = float(np.float32(1.0 - 1e-3))
EPS = float(np.float32(0.01))       # what `opacity ** 2 + 0.01` adds in fp32
HALF = 0.5
TERMS = ("sparsity", "opague", "z_var")
W = (0.5, 0.25, 2.0)                # the weights of the three-term runs (any: the bounds scale with them)


def binary_cross_entropy(input, target):
    """utils/ops.py:51-55"""
    return -(target * torch.log(input) + (1 - target) * torch.log(1 - input))


def map_loss_torch(o, v=None):
    """o, v: tensors of one shape and dtype -> the per-pixel summands (s, e, z) of trainer.py:349, :361-362 and :374-377 (z None
    without v); each term is its summands' mean"""
    s = (o ** 2 + EPS).sqrt()
    c = o.clamp(LO, HI)
    e = binary_cross_entropy(c, c)
    z = None
    if v is not None:
        c = o.clamp(LO, HI)
        z = v / c * (c > HALF)
    return s, e, z


@functools.lru_cache(maxsize=None)
def reference(name, dtype, weights=W):
    """-> dict(T [3], mean_abs [3], total, go, gv): the terms, the means of |summand|, sum_k weights[k] T_k and its gradients
    (upstream scalar 1) as float64 arrays, from the restatement on the CPU in `dtype`.  A term whose weight is 0 is left out of the
    total, as the kernel's mask leaves it out."""
    o32, v32 = inputs(name)
    o = torch.tensor(o32).to(dtype).requires_grad_(True)
    v = torch.tensor(v32).to(dtype).requires_grad_(True)
    summands = map_loss_torch(o, v)
    T = [x.mean() for x in summands]
    total = sum(w * t for w, t in zip(weights, T) if w != 0)
    total.backward()
    zero = torch.zeros_like(o)
    out = dict(T=np.array([float(t.detach()) for t in T]), mean_abs=np.array([float(x.detach().abs().mean()) for x in summands]),
               total=float(total.detach()), go=(zero if o.grad is None else o.grad).double().numpy(), gv=(zero if v.grad is None else v.grad).double().numpy())
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# (B, H, W): the smallest sizes at which each mechanism can break
S3, S70, SONE, SONE1, S32000, SSWEEP = (1, 1, 3), (2, 5, 7), (1, 32, KCHUNK // 32), (1, 1, KCHUNK + 1), (1, 160, 200), (1, 1, KSWEEP * KCHUNK + 5)
_LIST = [
    ("uniform", S3),        # less than one vector
    ("uniform", S70),       # less than a wave of vectors, not a multiple of 4
    ("uniform", SONE),      # exactly one chunk
    ("uniform", SONE1),     # one chunk plus one pixel
    ("uniform", S32000),    # several chunks, the last partial
    ("uniform", SSWEEP),    # one chunk more than a final-stage sweep
    ("disc", SONE),         # rendered-like: 0 outside, saturating inside, z_var on the rim
    ("disc", S32000),
    ("half", S70),          # the cancellation in log(1 - c) - log c
    ("half", S32000),
    ("zeros", S70),         # below the clamp everywhere
    ("zeros", SONE1),
    ("ones", S70),          # above it
    ("ones", SONE1),
    ("boundary", S70),      # lo, hi and 0.5 exactly and one ulp to either side
    ("boundary", SONE1),
    ("zoffset", S70),       # z_var + 100
    ("zoffset", S32000),
    ("nan_o", S70),         # one NaN pixel in opacity
    ("nan_o", S32000),
    ("nan_z", S70),         # one NaN in z_var where opacity <= 0.5
    ("nan_z", S32000),
]
CASES = {f"{v}-{s[0]}x{s[1]}x{s[2]}": (v, s, 700 + i) for i, (v, s) in enumerate(_LIST)}
NAMES = sorted(CASES)
assert len(CASES) == len(_LIST)

f32 = np.float32
BOUNDARY = np.array([x for mid in (f32(LO), f32(HI), f32(0.5)) for x in (np.nextafter(mid, f32(0)), mid, np.nextafter(mid, f32(1)))], f32)
NAN_AT = 5  # the flat index of the NaN pixel of the nan_* cases


def make_maps(values, B, H, W, seed):
    """-> (opacity, z_var) float32 [B,H,W]"""
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand(B, H, W, generator=gen, dtype=torch.float64)
    v = 1e-2 * torch.rand(B, H, W, generator=gen, dtype=torch.float64)
    if values in ("uniform", "zoffset", "nan_o", "nan_z", "boundary"):
        o = u
    elif values == "disc":
        yy, xx = torch.meshgrid(torch.linspace(-1, 1, H, dtype=torch.float64), torch.linspace(-1, 1, W, dtype=torch.float64), indexing="ij")
        r = torch.sqrt(xx * xx + yy * yy)[None] / (0.6 + 0.1 * torch.arange(B, dtype=torch.float64)[:, None, None])
        o = torch.sigmoid((1 - r) * 12)
        o = torch.where(o < 1e-3, torch.zeros_like(o), o)          # exactly 0 outside
        o = torch.where(o > 1 - 1e-4, torch.ones_like(o), o)       # exactly 1 well inside
        v = 1e-2 * torch.exp(-((r - 1) / 0.15) ** 2) * (0.5 + u)   # about 1e-2 on the rim
    elif values == "half":
        o = 0.5 + 1e-3 * (2 * u - 1)
    elif values == "zeros":
        o = torch.zeros(B, H, W, dtype=torch.float64)
    elif values == "ones":
        o = torch.ones(B, H, W, dtype=torch.float64)
    else:
        raise ValueError(values)
    o, v = o.float().numpy(), v.float().numpy()
    if values == "zoffset":
        v = (v + f32(100)).astype(f32)
    if values == "boundary":
        o.reshape(-1)[:BOUNDARY.size] = BOUNDARY
    if values == "nan_o":
        o.reshape(-1)[NAN_AT] = np.nan
    if values == "nan_z":
        o.reshape(-1)[NAN_AT] = f32(0.25)
        v.reshape(-1)[NAN_AT] = np.nan
    return o, v


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (opacity, z_var) float32 [B,H,W] arrays, not to be written to, made once per process"""
    values, (B, H, W), seed = CASES[name]
    o, v = make_maps(values, B, H, W, seed)
    o.setflags(write=False)
    v.setflags(write=False)
    return o, v


def clean_of(name):
    """the NaN case's maps with the NaN pixel replaced (-> opacity, z_var): the run its other pixels' gradients must equal"""
    o, v = (a.copy() for a in inputs(name))
    o.reshape(-1)[NAN_AT] = f32(0.25)
    v.reshape(-1)[NAN_AT] = f32(1e-2)
    return o, v


FLOOR = 2.0 ** -22


def bound_report(name, out4=None, go=None, gv=None, weights=W, scale=1.0):
    """-> ([(what, error, bound), ...], a line for the log).  out4 = (total, T_s, T_o, T_z) as the kernel reports them, go / gv its
    gradients taken with the upstream scalar `scale`.  Per term: |got - T64| <= 4 max(|T32 - T64|, 2^-22 mean|summand64|); the total's
    bound is the weighted sum of its terms' (it is linear in them) plus half an ulp of its fp32 rounding; per gradient tensor:
    max|got - g64| <= 4 max(max|g32 - g64|, 2^-22 max|g64|), both scaled by `scale`.  A term whose truth is NaN must be NaN; the NaN
    pixel of a nan_* case is left out of the gradient comparison (torch's value there is not pinned)."""
    r64, r32 = reference(name, torch.float64, weights), reference(name, torch.float32, weights)
    rows = []
    if out4 is not None:
        out4 = np.asarray(out4, np.float64)
        tb, nan_total = 2.0 ** -24 * abs(r64["total"]) if np.isfinite(r64["total"]) else 0.0, False
        for k, what in enumerate(TERMS):
            if weights[k] == 0:
                rows.append((what, abs(out4[1 + k]), 0.0, 0.0))  # a masked-off term reports 0
                continue
            if np.isnan(r64["T"][k]):
                rows.append((what, 0.0 if np.isnan(out4[1 + k]) else np.inf, 0.0, 0.0))
                nan_total = True
                continue
            e32 = abs(r32["T"][k] - r64["T"][k])
            b = 4 * max(e32, FLOOR * r64["mean_abs"][k])
            rows.append((what, abs(out4[1 + k] - r64["T"][k]), b, e32))
            tb += abs(weights[k]) * b
        if nan_total:
            rows.append(("total", 0.0 if np.isnan(out4[0]) else np.inf, 0.0, 0.0))
        else:
            rows.append(("total", abs(out4[0] - r64["total"]), tb, abs(r32["total"] - r64["total"])))
    keep = np.ones(r64["go"].size, bool)
    if CASES[name][0] in ("nan_o", "nan_z"):
        keep[NAN_AT] = False
    for what, g, key in (("gopacity", go, "go"), ("gz_var", gv, "gv")):
        if g is None:
            continue
        g = np.asarray(g, np.float64).reshape(-1)[keep]
        g64, g32 = r64[key].reshape(-1)[keep], r32[key].reshape(-1)[keep]
        e32 = scale * np.abs(g32 - g64).max()
        rows.append((what, np.abs(g - scale * g64).max(), 4 * max(e32, FLOOR * scale * np.abs(g64).max()), e32))
    line = f"{name} w={weights}: " + " ".join(f"{w}: err {e:.2e} (fp32 torch {e32:.2e}, bound {b:.2e})" for w, e, b, e32 in rows)
    return [r[:3] for r in rows], line


def check_bound(name, out4=None, go=None, gv=None, weights=W, scale=1.0):
    rows, line = bound_report(name, out4, go, gv, weights, scale)
    print(line)
    for what, err, bound in rows:
        assert err <= bound, (what, line)  # (a NaN error fails)


def masks(o):
    """-> (in, m) of an fp32 opacity array as numpy decides them in fp32: the clamp's gradient mask and c > 0.5"""
    o = np.asarray(o, f32)
    with np.errstate(invalid="ignore"):
        inside = (o >= f32(LO)) & (o <= f32(HI))
        c = np.where(o < f32(LO), f32(LO), np.where(o > f32(HI), f32(HI), o))
        return inside, c > f32(0.5)
