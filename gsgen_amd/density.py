"""The Gaussian density lattice of the mesh export (utils/export.py:20-120) on the GPU: gsgen_density_grid (gsgen_amd/csrc/knn.hip).

For every point of a reso^3 lattice over [-L, L]^3 the reference searches the K + 1 nearest Gaussian centres (pytorch3d, in batches
of 256 lattice points), drops the nearest and sums opacity * exp(-1/2 d^T Sigma^-1 d) over the K others.  Here one fused launch does
the search and the sum: no index or distance array is written.  The rest of `to_mesh` is in gsgen_amd.mesh (marching cubes on the
GPU, fed with the returned grid: density_mesh, mesh_from_ckpt) and gsgen_amd.io.write_obj.  field_at evaluates the same field at
points of the caller's own, with its gradient and a term-weighted colour (gsgen_density_points: the mesh's vertex normals and
colours, gsgen_amd.mesh.vertex_attributes).

The functions take CUDA (HIP) tensors, run on the current stream without host synchronisation (get_density_val_grid_from_ckpt's
`L < 0` takes the reference's own `.item()`), record no autograd graph, and can be captured by `torch.cuda.graph`.
"""
import collections

import torch

from . import _capi
from .knn import K_MAX


def _lib():
    lib = _capi.load()
    if not hasattr(lib, "density_grid"):
        raise RuntimeError(f"{lib.path} was built without gsgen_density_grid (gsgen_amd/csrc/knn.hip): rebuild it "
                           "(python -m gsgen_amd.build)")
    return lib


@torch.no_grad()
def density_grid_axes(mean, qvec, scale, opacity, axis_x, axis_y, axis_z, K=3, skip_nearest=True):
    """the kernel's own form: lattice coordinates as three 1-D tensors -> [len(axis_x), len(axis_y), len(axis_z)] float32"""
    K, skip = int(K), int(bool(skip_nearest))
    if mean.dim() != 2 or mean.shape[1] != 3 or not mean.is_cuda:
        raise ValueError(f"gsgen_amd.density: mean must be a [N, 3] CUDA (HIP) tensor, got {tuple(mean.shape)} on {mean.device}")
    N, dev = mean.shape[0], mean.device
    if not 1 <= K or K + skip > K_MAX:
        raise ValueError(f"gsgen_amd.density: K + skip_nearest = {K + skip} is not in 1..{K_MAX}")
    if N == 0 or K + skip > N:
        raise ValueError(f"gsgen_amd.density: {K + skip} neighbours of {N} Gaussians")
    if tuple(qvec.shape) != (N, 4) or tuple(scale.shape) != (N, 3) or opacity.numel() != N:
        raise ValueError(f"gsgen_amd.density: qvec {tuple(qvec.shape)}, scale {tuple(scale.shape)}, opacity {tuple(opacity.shape)} "
                         f"for {N} Gaussians")
    f = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
    mean, qvec, scale, opacity = f(mean), f(qvec), f(scale), f(opacity).reshape(-1)
    ax, ay, az = (f(a).reshape(-1) for a in (axis_x, axis_y, axis_z))
    lib = _lib()
    out = torch.empty(ax.numel(), ay.numel(), az.numel(), device=dev, dtype=torch.float32)
    nbytes = lib.density_grid_workspace_bytes(N, K)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    lib.density_grid(mean.data_ptr(), qvec.data_ptr(), scale.data_ptr(), opacity.data_ptr(), N, ax.data_ptr(), ay.data_ptr(),
                     az.data_ptr(), ax.numel(), ay.numel(), az.numel(), K, skip, out.data_ptr(), ws.data_ptr(), nbytes,
                     torch.cuda.current_stream(dev).cuda_stream)
    return out


Field = collections.namedtuple("Field", "density grad rgb")


@torch.no_grad()
def field_at(mean, qvec, scale, opacity, points, K=3, skip_nearest=True, color=None, density=True, grad=True):
    """The field of density_grid_axes at points [..., 3] of the caller's own (gsgen_density_points: one fused search-and-sum launch,
    no index or distance array) -> Field(density [...], grad [..., 3], rgb [..., 3]), None for what was not asked for.  density is
    bit-identical to the lattice at the same coordinates; grad is its gradient with the neighbour set held fixed; rgb, computed
    when color [N, 3] is given, is the average of the K + skip_nearest nearest centres' colours weighted by their terms (the
    nearest counts even where the field drops it; the nearest centre's colour where every term underflows).  A non-finite point
    gives zeros."""
    K, skip = int(K), int(bool(skip_nearest))
    if mean.dim() != 2 or mean.shape[1] != 3 or not mean.is_cuda:
        raise ValueError(f"gsgen_amd.density: mean must be a [N, 3] CUDA (HIP) tensor, got {tuple(mean.shape)} on {mean.device}")
    N, dev = mean.shape[0], mean.device
    if not 1 <= K or K + skip > K_MAX:
        raise ValueError(f"gsgen_amd.density: K + skip_nearest = {K + skip} is not in 1..{K_MAX}")
    if N == 0 or K + skip > N:
        raise ValueError(f"gsgen_amd.density: {K + skip} neighbours of {N} Gaussians")
    if tuple(qvec.shape) != (N, 4) or tuple(scale.shape) != (N, 3) or opacity.numel() != N:
        raise ValueError(f"gsgen_amd.density: qvec {tuple(qvec.shape)}, scale {tuple(scale.shape)}, opacity {tuple(opacity.shape)} "
                         f"for {N} Gaussians")
    if color is not None and tuple(color.shape) != (N, 3):
        raise ValueError(f"gsgen_amd.density: color {tuple(color.shape)} for {N} Gaussians")
    if points.dim() < 1 or points.shape[-1] != 3:
        raise ValueError(f"gsgen_amd.density: points must be [..., 3], got {tuple(points.shape)}")
    f = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
    mean, qvec, scale, opacity = f(mean), f(qvec), f(scale), f(opacity).reshape(-1)
    color = None if color is None else f(color)
    lead = tuple(points.shape[:-1])
    pts = f(points).reshape(-1, 3)
    Q = pts.shape[0]
    if Q > 0xffffffff:
        raise NotImplementedError(f"gsgen_amd.density: {Q} points -- the kernel takes up to 2^32 - 1")
    lib = _lib()
    if not hasattr(lib, "density_points"):
        raise RuntimeError(f"{lib.path} was built without gsgen_density_points (gsgen_amd/csrc/knn.hip): rebuild it "
                           "(python -m gsgen_amd.build)")
    new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)  # noqa: E731
    out_d = new(Q) if density else None
    out_g = new(Q, 3) if grad else None
    out_c = new(Q, 3) if color is not None else None
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    if Q and (density or grad or color is not None):
        nbytes = lib.density_points_workspace_bytes(N, K)
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        lib.density_points(mean.data_ptr(), qvec.data_ptr(), scale.data_ptr(), opacity.data_ptr(), ptr(color), N, pts.data_ptr(), Q, K,
                           skip, ptr(out_d), ptr(out_g), ptr(out_c), ws.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream)
    return Field(None if out_d is None else out_d.reshape(lead), None if out_g is None else out_g.reshape(lead + (3,)),
                 None if out_c is None else out_c.reshape(lead + (3,)))


@torch.no_grad()
def density_grid(mean, qvec, scale, opacity, L, reso, K=3, skip_nearest=True):
    """-> [reso, reso, reso] float32 on the device: the density at the points of torch.linspace(-L, L, reso)^3 (indexing "ij": x
    slowest), from activated scale [N,3] and opacity [N].  skip_nearest=True is the reference: the K + 1 nearest centres with the
    nearest dropped (utils/export.py:94-96 through utils/ops.py:129-134); False sums the K nearest.  The lattice coordinates are
    torch.linspace's on the device of `mean` (density_grid_axes takes coordinates of the caller's own)."""
    axis = torch.linspace(-L, L, int(reso), device=mean.device)
    return density_grid_axes(mean, qvec, scale, opacity, axis, axis, axis, K, skip_nearest)


@torch.no_grad()
def get_density_val_grid_from_ckpt(ckpt, batch_size=256, L=-1.0, reso=128, K=3):
    """utils/export.py:66-120 -> (grid [reso,reso,reso], L): ckpt holds the raw fields "mean", "qvec", "svec" (log scale) and "alpha"
    (logit opacity) on the GPU.  L < 0 takes mean.abs().max().item() * 1.1 -- one host sync, the reference's own.  batch_size is
    accepted for the signature and ignored: the lattice is one launch."""
    del batch_size
    if L < 0.0:
        L = ckpt["mean"].abs().max().item() * 1.1
    grid = density_grid(ckpt["mean"], ckpt["qvec"], torch.exp(ckpt["svec"]), torch.sigmoid(ckpt["alpha"]), L, reso, K, True)
    return grid, L
