"""Point-cloud normals and local coordinate frames on the GPU (k_point_normals in gsgen_amd/csrc/knn.hip through the C ABI).

The reference takes `estimate_pointcloud_normals` from pytorch3d.ops (utils/ops.py:9-12, :62-72); pytorch3d does not exist for
ROCm.  The functions below keep the reference's and pytorch3d's call shapes.  They take CUDA (HIP) tensors and run on the current
stream, with the workspace from torch's caching allocator and no host synchronisation, so a call can be captured by
`torch.cuda.graph` and replayed on new point values in the same tensor.

One launch searches each point's `neighborhood_size` nearest points (the point itself included, as pytorch3d's
knn_points(p, p, K) returns it; the list is gsgen_amd.knn's for the same K) and, from the list in registers, forms the covariance
of the neighbourhood and its eigen-frame: eigenvalues ascending (`curvatures`), frame columns n (the normal: smallest eigenvalue),
y, z (largest).  neighborhood_size is 3..64; pytorch3d's default of 50 is inside it.

Differences from pytorch3d, both deliberate:
  * The results carry NO autograd graph (pytorch3d's are differentiable through its eigen-solver).  The reference feeds them to
    the colour override of a visualisation (normal_as_rgb) and to pbr shading only.
  * With disambiguate_directions, where neither v nor -v has at least half of the neighbours on its side, pytorch3d's sign is
    whatever its solver produced; here it is the direction with a positive sum of projections, and failing that the one whose
    first non-zero component is positive.  Everywhere else the rule is pytorch3d's.
A non-finite point, and a point with fewer than neighborhood_size finite points around it, gets zeros.
"""
import torch

from . import _capi

K_MIN, K_MAX = 3, 64
OUTPUTS = ("normals", "curvature", "frames")
_SHAPES = {"normals": (3,), "curvature": (3,), "frames": (3, 3)}


def _lib():
    lib = _capi.load()
    if not hasattr(lib, "point_normals"):
        raise RuntimeError(f"{lib.path} was built without gsgen_point_normals (gsgen_amd/csrc/knn.hip): rebuild it (python -m gsgen_amd.build)")
    return lib


def _check_cloud(points, K):
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"gsgen_amd.normals: points must be a [N, 3] tensor, got {getattr(points, 'shape', type(points))}")
    if not points.is_cuda:
        raise ValueError("gsgen_amd.normals: points must be a CUDA (HIP) tensor -- there is no CPU implementation")
    if K >= points.shape[0]:
        # (pytorch3d's wording, verbatim: it reads the wrong way round there too)
        raise ValueError("The neighborhood_size argument has to be >= size of each of the point clouds.")
    if not K_MIN <= K <= K_MAX:
        raise NotImplementedError(f"gsgen_amd.normals: neighborhood_size = {K} is not in {K_MIN}..{K_MAX}")
    return points.shape[0]


@torch.no_grad()
def normals_raw(points, K, disambiguate=True, want=OUTPUTS):
    """points [N,3] -> dict of the kernel's own outputs named in `want`: normals [N,3], curvature [N,3] (eigenvalues ascending),
    frames [N,3,3] (columns n, y, z: frames[:, :, 0] == normals), float32"""
    K = int(K)
    N = _check_cloud(points, K)
    want = tuple(want)
    if not want or any(w not in OUTPUTS for w in want):
        raise ValueError(f"gsgen_amd.normals: want = {want!r} must name at least one of {OUTPUTS}")
    pts = points.detach().to(torch.float32).contiguous()
    dev = pts.device
    lib = _lib()
    out = {w: torch.empty((N,) + _SHAPES[w], device=dev, dtype=torch.float32) for w in want}
    ptr = lambda w: out[w].data_ptr() if w in out else None  # noqa: E731
    nbytes = lib.point_normals_workspace_bytes(N, K)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    lib.point_normals(pts.data_ptr(), N, K, 1 if disambiguate else 0, ptr("normals"), ptr("curvature"), ptr("frames"), ws.data_ptr(),
                      nbytes, torch.cuda.current_stream(dev).cuda_stream)
    return out


def _clouds(points):
    if not isinstance(points, torch.Tensor) or points.dim() not in (2, 3) or points.shape[-1] != 3:
        raise ValueError(f"gsgen_amd.normals: points must be a [B, N, 3] (or [N, 3]) tensor, got {getattr(points, 'shape', type(points))}")
    return points if points.dim() == 3 else points[None]


@torch.no_grad()
def estimate_normal(pos, neighborhood_size=50, disambiguate_directions=True):
    """utils/ops.py:62-72: pos [N,3] -> unit normals [N,3]"""
    return normals_raw(pos, neighborhood_size, disambiguate_directions, want=("normals",))["normals"]


@torch.no_grad()
def estimate_pointcloud_normals(points, neighborhood_size=50, disambiguate_directions=True):
    """pytorch3d.ops.estimate_pointcloud_normals: points [B,N,3] -> normals [B,N,3] (one call per cloud; [N,3] in, [N,3] out)"""
    clouds = _clouds(points)
    out = torch.stack([estimate_normal(c, neighborhood_size, disambiguate_directions) for c in clouds])
    return out if points.dim() == 3 else out[0]


@torch.no_grad()
def estimate_pointcloud_local_coord_frames(points, neighborhood_size=50, disambiguate_directions=True):
    """pytorch3d.ops.estimate_pointcloud_local_coord_frames: points [B,N,3] -> (curvatures [B,N,3] ascending, frames [B,N,3,3],
    columns ordered as the curvatures); [N,3] in: no batch axis out"""
    clouds = _clouds(points)
    res = [normals_raw(c, neighborhood_size, disambiguate_directions, want=("curvature", "frames")) for c in clouds]
    cur, fr = torch.stack([r["curvature"] for r in res]), torch.stack([r["frames"] for r in res])
    return (cur, fr) if points.dim() == 3 else (cur[0], fr[0])
