"""A triangle mesh to an evenly spaced point cloud on the GPU (gsgen_amd/csrc/mesh_sample.hip through the C ABI), and the mesh
initialisation of the reference built on it.

The reference turns a mesh into its initial Gaussians with trimesh (utils/mesh.py:52-69 `load_mesh_as_pcd_trimesh`, utils/
initialize.py:285-332 `mesh_initlization`): `sample_surface_even` = area-weighted surface samples thinned by `remove_close` (a
cKDTree on the host) so that no two are closer than sqrt(area / (3 n)).  trimesh is not needed here; the functions below keep its
call shapes on CUDA (HIP) tensors (numpy arrays are uploaded to the current device):

    mesh_area(verts, tris)                          device double scalar
    sample_surface(verts, tris, count, ...)         (points [count,3], face_index [count], extras): no host synchronisation
    remove_close(points, radius)                    (points[mask], mask): trimesh.points.remove_close
    sample_surface_even(verts, tris, count, ...)    (points, face_index[, attributes]), at most count rows
    load_mesh_as_pcd(verts_or_path, tris, num_points)   the reference's top-up loop -> (points [num_points,3], random colours)
    mesh_initialize(cfg, verts, tris, colors)       the initial_values dict of GaussianSplattingRenderer

Definitions (DESIGN.md "Mesh sampling"): a face is chosen as np.searchsorted(cumsum(area), u * total) chooses it, except that
u = 0 skips leading zero-area faces; the greedy remove_close keeps point i iff no kept j < i lies in the CLOSED ball
d2(i, j) <= r * r (fp32).  Deliberate differences from trimesh: the random stream is torch's (`generator`), not NumPy's; faces with
a non-finite vertex or an index out of range weigh 0 instead of poisoning the sum; non-finite points are removed by remove_close.
"""
import math
import os

import numpy as np
import torch

from . import _capi

MAX_ATTR = 8      # mesh_sample.hip: kMaxAttr
ROUND_GROUP = 8   # rounds enqueued between two reads of the undecided count


def _lib():
    lib = _capi.load()
    if not hasattr(lib, "mesh_sample"):
        raise RuntimeError(f"{lib.path} was built without the mesh sampling kernels (gsgen_amd/csrc/mesh_sample.hip): rebuild it "
                           "(python -m gsgen_amd.build)")
    return lib


def _mesh(verts, tris):
    """-> (verts float32 [V,3], tris int32 [F,3]) contiguous on one CUDA (HIP) device"""
    if not isinstance(verts, torch.Tensor):
        verts = torch.as_tensor(np.asarray(verts, np.float32)).cuda()
    if not verts.is_cuda:
        raise ValueError("gsgen_amd.mesh_sample: verts must be a CUDA (HIP) tensor -- there is no CPU implementation")
    if not isinstance(tris, torch.Tensor):
        tris = torch.as_tensor(np.asarray(tris, np.int64))
    if verts.dim() != 2 or verts.shape[1] != 3 or tris.dim() != 2 or tris.shape[1] != 3:
        raise ValueError(f"gsgen_amd.mesh_sample: verts must be [V, 3] and tris [F, 3], got {tuple(verts.shape)} and {tuple(tris.shape)}")
    if tris.dtype.is_floating_point or tris.dtype == torch.bool:
        raise ValueError(f"gsgen_amd.mesh_sample: tris must hold integers, got {tris.dtype}")
    return verts.detach().to(torch.float32).contiguous(), tris.to(verts.device).to(torch.int32).contiguous()


@torch.no_grad()
def _sample_raw(verts, tris, uniforms, attributes=None, points=True, face=True, barycentric=False, normals=False):
    """one gsgen_mesh_sample call -> dict of the outputs asked for and "status" (float64 [2]: element 1 is the total area, the
    bytes of element 0 are the int32 pair bad_faces, zero_area_flag).  uniforms None: the weights and the scan alone."""
    dev = verts.device
    V, F = verts.shape[0], tris.shape[0]
    M = 0 if uniforms is None else uniforms.shape[0]
    A = 0 if attributes is None else attributes.shape[1]
    out = {"status": torch.zeros(2, device=dev, dtype=torch.float64)}
    if points:
        out["points"] = torch.full((M, 3), float("nan"), device=dev) if F == 0 else torch.empty(M, 3, device=dev)
    if face:
        out["face"] = torch.full((M,), -1, device=dev, dtype=torch.int32) if F == 0 else torch.empty(M, device=dev, dtype=torch.int32)
    if barycentric:
        out["barycentric"] = torch.full((M, 2), float("nan"), device=dev) if F == 0 else torch.empty(M, 2, device=dev)
    if A:
        out["attributes"] = torch.full((M, A), float("nan"), device=dev) if F == 0 else torch.empty(M, A, device=dev)
    if normals:
        out["normals"] = torch.full((M, 3), float("nan"), device=dev) if F == 0 else torch.empty(M, 3, device=dev)
    if F == 0:
        out["status"].view(torch.int32)[1] = 1  # (no faces: total area 0)
        return out
    lib = _lib()
    nbytes = lib.mesh_sample_workspace_bytes(F)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    ptr = lambda k: out[k].data_ptr() if k in out and M else None  # noqa: E731
    lib.mesh_sample(verts.data_ptr() if V else None, V, tris.data_ptr(), F, uniforms.data_ptr() if M else None, M,
                    attributes.data_ptr() if A else None, A, ptr("points"), ptr("face"), ptr("barycentric"), ptr("attributes"),
                    ptr("normals"), out["status"].data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream)
    return out


def _check_attributes(attributes, verts):
    if attributes is None:
        return None
    if not isinstance(attributes, torch.Tensor):
        attributes = torch.as_tensor(np.asarray(attributes, np.float32))
    if attributes.dim() != 2 or attributes.shape[0] != verts.shape[0] or not 1 <= attributes.shape[1] <= MAX_ATTR:
        raise ValueError(f"gsgen_amd.mesh_sample: attributes must be [V, A] with A in 1..{MAX_ATTR}, got {tuple(attributes.shape)} "
                         f"for {verts.shape[0]} vertices")
    return attributes.detach().to(verts.device).to(torch.float32).contiguous()


@torch.no_grad()
def mesh_area(verts, tris):
    """-> the total area of the mesh, a float64 scalar on the device (no host synchronisation)"""
    verts, tris = _mesh(verts, tris)
    return _sample_raw(verts, tris, None, points=False, face=False)["status"][1]


@torch.no_grad()
def sample_surface(verts, tris, count, *, uniforms=None, generator=None, attributes=None, normals=False, barycentric=False):
    """trimesh.sample.sample_surface: `count` area-weighted samples of the mesh -> (points [count,3] float32, face_index [count]
    int64), then, in this order, each extra that was asked for: attributes [count,A] (per-vertex `attributes` [V,A], A in 1..8,
    interpolated as the points are), normals [count,3] (the face's unit normal), barycentric [count,2] (the weights of v1 and v2).
    uniforms: [count,3] float32 in [0,1) = (u_face, r1, r2); default torch.rand(count, 3, generator=generator) on the device.  No
    host synchronisation.  A mesh of total area 0: NaN points, face_index -1."""
    verts, tris = _mesh(verts, tris)
    count = int(count)
    if count < 0:
        raise ValueError(f"gsgen_amd.mesh_sample: count = {count}")
    attributes = _check_attributes(attributes, verts)
    if uniforms is None:
        uniforms = torch.rand(count, 3, generator=generator, device=verts.device, dtype=torch.float32)
    elif tuple(uniforms.shape) != (count, 3):
        raise ValueError(f"gsgen_amd.mesh_sample: uniforms must be [{count}, 3], got {tuple(uniforms.shape)}")
    uniforms = uniforms.detach().to(verts.device).to(torch.float32).contiguous()
    out = _sample_raw(verts, tris, uniforms, attributes, barycentric=barycentric, normals=normals)
    extras = [out[k] for k in ("attributes", "normals", "barycentric") if k in out]
    return (out["points"], out["face"].long(), *extras)


@torch.no_grad()
def remove_close(points, radius):
    """trimesh.points.remove_close: -> (points[mask], mask [N] bool).  Point i is kept iff no KEPT point j < i lies within the closed
    ball (dx dx + dy dy) + dz dz <= radius * radius in fp32: the greedy loop in index order.  Non-finite points are removed.  The
    device decides in rounds (one launch each); this loop enqueues them ROUND_GROUP at a time and reads the undecided count after
    each group -- the only host synchronisation.  Chains of dependent points need as many rounds as they are long."""
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3 or not points.is_cuda:
        raise ValueError(f"gsgen_amd.mesh_sample: points must be a [N, 3] CUDA (HIP) tensor, got {getattr(points, 'shape', type(points))}")
    radius = float(radius)
    if not radius >= 0.0:
        raise ValueError(f"gsgen_amd.mesh_sample: radius = {radius} must be >= 0")
    N, dev = points.shape[0], points.device
    if N == 0:
        return points, torch.zeros(0, device=dev, dtype=torch.bool)
    pts = points.detach().to(torch.float32).contiguous()
    lib = _lib()
    keep = torch.empty(N, device=dev, dtype=torch.uint8)
    remaining = torch.empty(1, device=dev, dtype=torch.int32)
    nbytes = lib.remove_close_workspace_bytes(N)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    stream = torch.cuda.current_stream(dev).cuda_stream
    lib.remove_close_init(pts.data_ptr(), N, radius, keep.data_ptr(), ws.data_ptr(), nbytes, stream)
    before = N
    while True:
        lib.remove_close_rounds(ROUND_GROUP, N, radius, keep.data_ptr(), remaining.data_ptr(), ws.data_ptr(), nbytes, stream)
        left = int(remaining.item())
        if left == 0:
            break
        if left >= before:  # (the undecided point of lowest index always decides: a correct kernel cannot get here)
            raise RuntimeError(f"gsgen_amd.mesh_sample.remove_close: {left} points undecided after a group of rounds, {before} before it")
        before = left
    mask = keep.bool()
    return points[mask], mask


@torch.no_grad()
def sample_surface_even(verts, tris, count, radius=None, *, generator=None, attributes=None):
    """trimesh.sample.sample_surface_even: 3 * count surface samples, thinned by remove_close(radius), the first `count` survivors in
    sample order -> (points, face_index[, attributes]) with at most `count` rows (fewer is a valid result, as in trimesh).  radius
    None: sqrt(area / (3 count)), from one host read of the area.  A mesh of total area 0 raises ValueError."""
    verts, tris = _mesh(verts, tris)
    count = int(count)
    if count <= 0:
        raise ValueError(f"gsgen_amd.mesh_sample: count = {count} must be positive")
    attributes = _check_attributes(attributes, verts)
    uniforms = torch.rand(3 * count, 3, generator=generator, device=verts.device, dtype=torch.float32)
    out = _sample_raw(verts, tris, uniforms, attributes)
    area = float(out["status"][1].item())
    if not area > 0.0:
        raise ValueError("gsgen_amd.mesh_sample: the mesh has no area to sample (every face is degenerate, non-finite or out of range)")
    if radius is None:
        radius = math.sqrt(area / (3 * count))
    points, mask = remove_close(out["points"], radius)
    res = [points[:count], out["face"][mask][:count].long()]
    if attributes is not None:
        res.append(out["attributes"][mask][:count])
    return tuple(res)


def _read_mesh(path):
    """-> (verts, tris, colors float32 in [0, 1] or None) of a .obj or .ply file (gsgen_amd.io's readers, by suffix)"""
    from . import io
    suffix = os.path.splitext(str(path))[1].lower()
    if suffix == ".obj":
        verts, tris, _, colors = io.read_obj_attributes(path)
        return verts, tris, colors
    if suffix == ".ply":
        verts, tris, _, colors = io.read_ply_mesh(path)
        return verts, tris, None if colors is None else colors.astype(np.float32) / 255.0
    raise NotImplementedError(f"gsgen_amd.mesh_sample: unknown mesh file {path} (.obj and .ply are read)")


def _even_cloud(verts, tris, num_points, generator, attributes):
    """utils/mesh.py:54-66: sample_surface_even until num_points rows are there -> (points, attributes or None)"""
    n = int(num_points)
    points, attrs = [], []
    while n > 0:
        res = sample_surface_even(verts, tris, n, generator=generator, attributes=attributes)
        p = res[0]
        if p.shape[0] == 0:  # (trimesh's loop would spin here)
            raise RuntimeError("gsgen_amd.mesh_sample: sample_surface_even returned no points")
        n -= p.shape[0]
        points.append(p if n >= 0 else p[:n])
        if attributes is not None:
            attrs.append(res[2] if n >= 0 else res[2][:n])
    points = torch.cat(points, dim=0) if len(points) > 1 else points[0]
    return points, (torch.cat(attrs, dim=0) if attributes is not None else None)


@torch.no_grad()
def load_mesh_as_pcd(verts_or_path, tris=None, num_points=4096, generator=None):
    """utils/mesh.py:52-69 (`load_mesh_as_pcd_trimesh`) -> (points [num_points,3] float32 on the device, torch.rand_like(points)).
    With tris None the first argument is the path of a .obj (gsgen_amd.io.read_obj) or .ply (read_ply_mesh) file."""
    if tris is None:
        from . import io
        suffix = os.path.splitext(str(verts_or_path))[1].lower()
        if suffix == ".obj":
            verts, tris = io.read_obj(verts_or_path)
        elif suffix == ".ply":
            verts, tris = io.read_ply_mesh(verts_or_path)[:2]
        else:
            raise NotImplementedError(f"gsgen_amd.mesh_sample: unknown mesh file {verts_or_path} (.obj and .ply are read)")
    else:
        verts = verts_or_path
    verts, tris = _mesh(verts, tris)
    points, _ = _even_cloud(verts, tris, num_points, generator, None)
    return points, torch.rand(points.shape, generator=generator, device=points.device, dtype=points.dtype)


def _cfg(cfg, key, default=None):
    from .model import _get
    return _get(cfg, key, default)


@torch.no_grad()
def mesh_initialize(cfg, verts=None, tris=None, colors=None, generator=None):
    """utils/initialize.py:285-332 (`mesh_initlization`) -> the initial_values dict of gsgen_amd.model.GaussianSplattingRenderer
    (mean, color, svec, qvec, alpha on the device, "raw": False).  The mesh is (verts, tris) or, when verts is None, the file
    cfg.mesh.  cfg.num_points points are sampled evenly, centred, scaled by cfg.mean_std / (max norm + 1e-5) and flipped as
    cfg.flip_yz / cfg.flip_xy ask; svec = cfg.svec_val, or gsgen_amd.knn.nearest_neighbor_initialize(mean, 3) when svec_val <= 0;
    colours are random unless cfg.random_color is False and per-vertex `colors` [V,3] (or the file's) exist, which are then
    interpolated at the samples."""
    if verts is None:
        path = _cfg(cfg, "mesh")
        if path is None or not os.path.exists(str(path)):
            raise FileNotFoundError(f"Mesh path {path} does not exist")
        verts, tris, file_colors = _read_mesh(path)
        colors = file_colors if colors is None else colors
    verts, tris = _mesh(verts, tris)
    num_points = int(_cfg(cfg, "num_points"))
    random_color = bool(_cfg(cfg, "random_color", True))
    use_colors = not random_color and colors is not None
    xyz, rgb = _even_cloud(verts, tris, num_points, generator, _check_attributes(colors[..., :3], verts) if use_colors else None)
    if rgb is None:
        rgb = torch.rand(xyz.shape, generator=generator, device=xyz.device, dtype=xyz.dtype)
    xyz = xyz - xyz.mean(dim=0, keepdim=True)
    xyz = xyz / (xyz.norm(dim=-1).max() + 1e-5)
    xyz = xyz * float(_cfg(cfg, "mean_std"))
    if _cfg(cfg, "flip_yz", False):
        x, y, z = xyz.chunk(3, dim=-1)
        xyz = torch.cat([x, z, y], dim=-1)
    if _cfg(cfg, "flip_xy", False):
        x, y, z = xyz.chunk(3, dim=-1)
        xyz = torch.cat([y, x, z], dim=-1)
    xyz = xyz.contiguous()
    svec_val = float(_cfg(cfg, "svec_val"))
    if svec_val > 0.0:
        svec = torch.ones(num_points, 3, dtype=torch.float32, device=xyz.device) * svec_val
    else:
        from .knn import nearest_neighbor_initialize
        svec = nearest_neighbor_initialize(xyz, k=3)[..., None].repeat(1, 3).to(xyz.device)
    alpha = torch.ones(num_points, dtype=torch.float32, device=xyz.device) * float(_cfg(cfg, "alpha_val"))
    qvec = torch.zeros(num_points, 4, dtype=torch.float32, device=xyz.device)
    qvec[:, 0] = 1.0
    return {"mean": xyz, "color": rgb, "svec": svec, "qvec": qvec, "alpha": alpha, "raw": False}
