"""Farthest point sampling on the GPU (gsgen_amd/csrc/fps.hip through the C ABI).

The reference takes this from pytorch3d's `sample_farthest_points` (utils/ops.py:76-100), which does not exist for ROCm; the Point-E
guidance calls it in every step (guidance/point_e.py:120-127, :169-179), the initialisers once (utils/initialize.py:379,
utils/viewer/pcd.py:183).  The functions below keep pytorch3d's and the reference wrapper's signatures and results.  They take CUDA
(HIP) tensors and run on the current stream, the workspace comes from torch's caching allocator, and they do not synchronise with
the host: with `start_idx` given as a device tensor a call can be captured by `torch.cuda.graph` and replayed on new point values
and new starts in the same tensors.

The rule: idx[0] is the start; m[p] = +inf; after pick s, m[p] = min(m[p], d2(p, s)) with d2 the fp32 sum of squared coordinate
differences, left to right; the next pick is the point of the largest m, ties to the LOWEST index (an fp32 NumPy loop reproduces
every index).  A point with a NaN / Inf coordinate is never picked.  A start that is out of range or not finite is replaced by the
lowest-index finite point.  When K exceeds the number of pickable points of a cloud the rest of its row is padding: index -1, zero
coordinates.  Exact duplicates: once every remaining m is 0 the rule picks the lowest index again.

`method`: "brute" (D = 3 or 6: one 1024-thread workgroup per cloud scans the whole cloud per pick), "bucket" (D = 3: the same
picks, skipping the spatial buckets a new pick cannot change), "auto" (bucket for D = 3 and L >= AUTO_BUCKET_MIN_POINTS).
"""
import torch

from . import _capi

# the implementation's boundaries (gsgen_amd/csrc/fps.hip: kThreads, kRegPoints, kBucketsMax, kAutoBucketMin)
BRUTE_THREADS = 1024          # threads of the one workgroup that samples a cloud
BRUTE_REG_POINTS = 16         # brute: m stays in registers while L <= BRUTE_THREADS * BRUTE_REG_POINTS
BUCKETS_MAX = 4096            # bucket: spatial buckets at most
AUTO_BUCKET_MIN_POINTS = 65536  # auto: bucket from this many points (D = 3); measured, see DESIGN.md

_METHODS = {"auto": 0, "brute": 1, "bucket": 2}


def _lib():
    lib = _capi.load()
    if not hasattr(lib, "fps"):
        raise RuntimeError(f"{lib.path} was built without the sampling kernel (gsgen_amd/csrc/fps.hip): rebuild it "
                           "(python -m gsgen_amd.build)")
    return lib


def _starts(B, L, lengths, random_start_point, start_idx, dev):
    """-> int32 [B] on dev"""
    if start_idx is not None:
        if random_start_point:
            raise ValueError("gsgen_amd.fps: start_idx and random_start_point=True exclude each other")
        s = start_idx if isinstance(start_idx, torch.Tensor) else torch.as_tensor(start_idx)
        if s.dim() == 0:
            s = s.reshape(1).expand(B)
        if s.dim() != 1 or s.shape[0] != B:
            raise ValueError(f"gsgen_amd.fps: start_idx must hold one start per cloud ([{B}]), got {tuple(s.shape)}")
        if s.dtype.is_floating_point or s.dtype == torch.bool:
            raise ValueError(f"gsgen_amd.fps: start_idx must be an integer tensor, got {s.dtype}")
        if torch.cuda.is_current_stream_capturing() and not s.is_cuda:
            raise ValueError("gsgen_amd.fps: inside a stream capture start_idx must be a device tensor (a replay reads it anew)")
        return s.to(device=dev, dtype=torch.int32).contiguous()
    if not random_start_point:
        return torch.zeros(B, device=dev, dtype=torch.int32)
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("gsgen_amd.fps: random_start_point=True draws its starts on the host and cannot be captured; "
                           "pass start_idx as a device tensor")
    if lengths is not None:
        lens = [int(v) for v in lengths.tolist()]
    else:
        lens = [L] * B
    return torch.stack([torch.randint(max(n, 1), ()) for n in lens]).to(device=dev, dtype=torch.int32)


@torch.no_grad()
def fps_raw(points, K, start_idx, lengths=None, method="auto", shared=False):
    """The kernel's own output, idx int32 [B, K].  points: [B, L, D] float32 CUDA (a batch stride of 0 is a shared cloud), or
    [L, D] with shared=True: every entry of start_idx [B] samples that one cloud.  start_idx int32 [B] on the device."""
    if method not in _METHODS:
        raise ValueError(f"gsgen_amd.fps: method must be one of {sorted(_METHODS)}, got {method!r}")
    K = int(K)
    if K < 1:
        raise ValueError(f"gsgen_amd.fps: K = {K} samples")
    B = start_idx.shape[0]
    L, D = points.shape[-2], points.shape[-1]
    if D not in (3, 6):
        raise NotImplementedError(f"gsgen_amd.fps: points of dimension {D} -- the kernels take D = 3 and D = 6")
    if method == "bucket" and D != 3:
        raise NotImplementedError(f"gsgen_amd.fps: method 'bucket' takes D = 3, got D = {D}")
    if L == 0 or B == 0:
        raise ValueError(f"gsgen_amd.fps: {B} clouds of {L} points")
    dev = points.device
    if shared or (points.dim() == 3 and points.stride(0) == 0) or B == 1:
        pts = (points if points.dim() == 2 else points[0]).contiguous()
        stride = 0
    else:
        pts = points.contiguous()
        stride = L * D
    lib = _lib()
    idx = torch.empty(B, K, device=dev, dtype=torch.int32)
    m = _METHODS[method]
    nbytes = lib.fps_workspace_bytes(L, D, B, K, m)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    lib.fps(pts.data_ptr(), L, D, stride, 0 if lengths is None else lengths.data_ptr(), start_idx.data_ptr(), B, K, idx.data_ptr(),
            ws.data_ptr(), nbytes, m, torch.cuda.current_stream(dev).cuda_stream)
    return idx


def _check_points(points, dims):
    if not isinstance(points, torch.Tensor) or points.dim() not in dims:
        want = " or ".join("[B, L, D]" if d == 3 else "[L, D]" for d in dims)
        raise ValueError(f"gsgen_amd.fps: points must be a {want} tensor, got {getattr(points, 'shape', type(points))}")
    if not points.is_cuda:
        raise ValueError("gsgen_amd.fps: points must be a CUDA (HIP) tensor -- there is no CPU implementation")
    if points.dtype != torch.float32:
        raise NotImplementedError(f"gsgen_amd.fps: points must be float32, got {points.dtype}")


def _gather(points3, idx):
    """sampled [B, K, D] through torch indexing (autograd reaches points); padded entries (-1) are zero rows"""
    idx = idx.long()
    pad = idx < 0
    rows = torch.gather(points3, 1, idx.clamp(min=0)[:, :, None].expand(-1, -1, points3.shape[2]))
    return rows.masked_fill(pad[:, :, None], 0.0), idx


def sample_farthest_points(points, lengths=None, K=50, random_start_point=False, *, start_idx=None, method="auto"):
    """pytorch3d's sample_farthest_points: points [B, L, D] (D = 3 or 6), lengths [B] or None -> (sampled [B, K, D], idx [B, K]
    int64).  Padded entries hold index -1 and zero coordinates.  `sampled` is gathered with torch indexing, so autograd reaches
    `points`.  A batch stride of 0 (an `expand`) is sampled as one shared cloud.

    random_start_point=True draws `torch.randint(L_b, ())` per cloud from torch's CPU generator, in batch order (pytorch3d's own
    draw is not reproduced: the same seed gives other starts there); it reads `lengths` on the host and raises inside a stream
    capture.  start_idx [B] (keyword only, an extension) fixes the starts instead; as a device tensor it is read by the kernel."""
    _check_points(points, (3,))
    B, L, _ = points.shape
    if isinstance(K, (list, tuple, torch.Tensor)):
        raise NotImplementedError("gsgen_amd.fps: a per-cloud K is not implemented; K is one int")
    lens = None
    if lengths is not None:
        if not isinstance(lengths, torch.Tensor) or lengths.shape != (B,):
            raise ValueError(f"gsgen_amd.fps: lengths must be a [{B}] tensor, got {getattr(lengths, 'shape', type(lengths))}")
        lens = lengths.to(device=points.device, dtype=torch.int32).contiguous()
    starts = _starts(B, L, lens, random_start_point, start_idx, points.device)
    idx = fps_raw(points.detach(), K, starts, lens, method)
    return _gather(points, idx)


def farthest_point_sampling(mean, K, random_start_point=False, *, start_idx=None, method="auto"):
    """utils/ops.py:76-100: mean [L, D] -> (pts [K, D], idx [K]); mean [B, L, D] -> ([B, K, D], [B, K]).
    The shared cloud: mean [L, D] with start_idx a [B] tensor -> ([B, K, D], [B, K]): B samplings of the one cloud, each from its
    own start, without B copies of it (guidance/point_e.py repeats the cloud batch_size times)."""
    _check_points(mean, (2, 3))
    if mean.dim() == 3:
        return sample_farthest_points(mean, None, K, random_start_point, start_idx=start_idx, method=method)
    L = mean.shape[0]
    if isinstance(start_idx, torch.Tensor) and start_idx.dim() == 1:
        starts = _starts(start_idx.shape[0], L, None, random_start_point, start_idx, mean.device)
        idx = fps_raw(mean.detach(), K, starts, None, method, shared=True)
        return _gather(mean[None].expand(starts.shape[0], -1, -1), idx)
    pts, idx = sample_farthest_points(mean[None], None, K, random_start_point, start_idx=start_idx, method=method)
    return pts[0], idx[0]
