"""Marching cubes on the GPU (gsgen_marching_cubes, gsgen_amd/csrc/marching_cubes.hip) and the mesh export of the reference built
on it: utils/export.py:123-155 (`to_mesh`) calls PyMCubes and mcubes.export_obj on the host; here the density lattice of
gsgen_amd.density goes to triangles without leaving the device, and gsgen_amd.io.write_obj writes the file.

    verts, tris, L = mesh_from_ckpt(ckpt)          # ckpt: the raw fields on the GPU (gsgen_amd.io.load_checkpoint(..., "cuda")[0])
    gsgen_amd.io.write_obj("mesh.obj", verts, tris)
    verts, tris, normals, colors, L = colored_mesh_from_ckpt(ckpt)     # + vertex normals and colours (vertex_attributes)
    gsgen_amd.io.write_obj("mesh.obj", verts, tris, normals, colors)   # or write_ply_mesh

Conventions (DESIGN.md "Marching cubes"): a lattice point is inside iff grid - thresh > 0 in fp32 (NaN is outside), as in the
reference's in-tree shap_e/rendering/mc.py, against which the kernels are pinned.  PyMCubes is not available to pin against: its
tie-breaking at grid == thresh and its triangle order may differ.  Vertices come one per sign-changing lattice edge, x-edges
first, then y-, then z-edges, each in raster order; triangles in cube raster order with normals from inside to outside (here:
from high density to low).  marching_cubes returns lattice index coordinates, as the reference's `marching_cubes(grid, L, reso,
thresh)` does (it ignores L); density_mesh and mesh_from_ckpt DELIBERATELY differ from `to_mesh` and return world coordinates
x = idx * (2 L / (reso - 1)) - L, the coordinates of the Gaussians the mesh was made from.

Everything runs on the current stream.  marching_cubes synchronises once, to read the two counts that size its outputs;
marching_cubes_into never does and can be captured by `torch.cuda.graph`.  Outputs are bit-identical from run to run.
"""
import torch

from . import _capi

MAX_POINTS = 1 << 30  # marching_cubes.hip: kMaxPoints


def _lib():
    lib = _capi.load()
    if not hasattr(lib, "marching_cubes"):
        raise RuntimeError(f"{lib.path} was built without the marching cubes kernels (gsgen_amd/csrc/marching_cubes.hip): rebuild "
                           "it (python -m gsgen_amd.build)")
    return lib


def _check_grid(grid):
    if not isinstance(grid, torch.Tensor) or grid.dim() != 3:
        raise ValueError(f"gsgen_amd.mesh: grid must be a [X, Y, Z] tensor, got shape {tuple(getattr(grid, 'shape', ())) or type(grid)}")
    if min(grid.shape) < 2:
        raise ValueError(f"gsgen_amd.mesh: a lattice of {tuple(grid.shape)} points has no cubes: every dimension must be at least 2")
    if grid.numel() > MAX_POINTS:
        raise NotImplementedError(f"gsgen_amd.mesh: a lattice of {grid.numel()} points -- the kernels take up to 2^30")
    if not grid.is_cuda:
        raise ValueError("gsgen_amd.mesh: grid must be a CUDA (HIP) tensor -- there is no CPU implementation")
    return grid.detach().to(torch.float32).contiguous()


def _check_out(name, buf, dtype):
    if buf is None:
        return 0, 0
    if buf.dim() != 2 or buf.shape[1] != 3 or buf.dtype != dtype or not buf.is_contiguous() or not buf.is_cuda:
        raise ValueError(f"gsgen_amd.mesh: {name} must be a contiguous [capacity, 3] {dtype} CUDA (HIP) tensor, got "
                         f"{tuple(buf.shape)} {buf.dtype} on {buf.device}")
    return buf.shape[0], buf.data_ptr() if buf.shape[0] else 0


@torch.no_grad()
def marching_cubes_into(grid, thresh, verts_buf, tris_buf, counts):
    """The capturable form: no host synchronisation, the caller's buffers.  verts_buf [cap_v, 3] float32 and tris_buf [cap_t, 3]
    int32 (either may be None: nothing of that kind is written) receive the rows that fit; counts (int32 [3] on the device) receives
    {V, F, overflow}: the true numbers of vertices and triangles, and 1 when either exceeds its buffer.  With the flag set, a written
    triangle may name a vertex that was dropped.  Returns None."""
    grid = _check_grid(grid)
    dev = grid.device
    if not isinstance(counts, torch.Tensor) or counts.numel() != 3 or counts.dtype != torch.int32 or not counts.is_contiguous() \
            or counts.device != dev:
        raise ValueError("gsgen_amd.mesh: counts must be a contiguous int32 tensor of 3 elements on the device of grid")
    vcap, vptr = _check_out("verts_buf", verts_buf, torch.float32)
    tcap, tptr = _check_out("tris_buf", tris_buf, torch.int32)
    for buf in (verts_buf, tris_buf):
        if buf is not None and buf.device != dev:
            raise ValueError("gsgen_amd.mesh: the output buffers must be on the device of grid")
    lib = _lib()
    X, Y, Z = grid.shape
    nbytes = lib.marching_cubes_workspace_bytes(X, Y, Z)
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    lib.marching_cubes(grid.data_ptr(), X, Y, Z, float(thresh), vptr, vcap, tptr, tcap, counts.data_ptr(), ws.data_ptr(), nbytes,
                       torch.cuda.current_stream(dev).cuda_stream)


@torch.no_grad()
def marching_cubes(grid, thresh, index_dtype=torch.int32):
    """-> (verts [V,3] float32 in lattice index coordinates, tris [F,3] index_dtype) of the surface grid == thresh of a [X, Y, Z]
    CUDA (HIP) tensor (made contiguous float32 if it is not).  A counting pass, one host read of its three integers -- the only
    synchronisation, inherent in outputs whose shape depends on the data --, then an emit pass into tensors of the exact size.  A
    lattice that is all outside or all inside returns two (0, 3) tensors."""
    if index_dtype not in (torch.int32, torch.int64):
        raise ValueError(f"gsgen_amd.mesh: index_dtype must be torch.int32 or torch.int64, got {index_dtype}")
    grid = _check_grid(grid)
    dev = grid.device
    counts = torch.empty(3, device=dev, dtype=torch.int32)
    marching_cubes_into(grid, thresh, None, None, counts)
    V, F, _ = (c & 0xffffffff for c in counts.tolist())
    if V > 0x7fffffff or F > 0x7fffffff:
        raise NotImplementedError(f"gsgen_amd.mesh: {V} vertices and {F} triangles do not fit int32 indices")
    verts = torch.empty(V, 3, device=dev, dtype=torch.float32)
    tris = torch.empty(F, 3, device=dev, dtype=torch.int32)
    if V or F:
        marching_cubes_into(grid, thresh, verts, tris, counts)
    return verts, tris.to(index_dtype)


def index_to_world(verts, L, reso):
    """lattice index coordinates of a reso^3 lattice over [-L, L]^3 -> world coordinates, in fp32: idx * (2 L / (reso - 1)) - L"""
    return verts * (2.0 * float(L) / (int(reso) - 1)) - float(L)


@torch.no_grad()
def density_mesh(mean, qvec, scale, opacity, L, reso, K=3, thresh=0.5, skip_nearest=True):
    """-> (verts [V,3] float32 in WORLD coordinates, tris [F,3] int32): gsgen_amd.density.density_grid (activated scale [N,3] and
    opacity [N]; the reso^3 lattice over [-L, L]^3) fed straight into marching_cubes on the device.  The reference's
    marching_cubes(grid, L, reso, thresh) returns index coordinates and ignores L; mapping them to the Gaussians' own
    coordinates is a deliberate difference (index_to_world; marching_cubes(density_grid(...), thresh) is the reference's form)."""
    from .density import density_grid
    verts, tris = marching_cubes(density_grid(mean, qvec, scale, opacity, L, reso, K, skip_nearest), thresh)
    return index_to_world(verts, L, reso), tris


@torch.no_grad()
def mesh_from_ckpt(ckpt, reso=128, K=3, thresh=0.5, L=-1.0):
    """get_density_val_grid_from_ckpt followed by to_mesh (utils/export.py:66-155) -> (verts in world coordinates, tris, L).  ckpt
    holds the raw fields "mean", "qvec", "svec", "alpha" on the GPU; L < 0 takes mean.abs().max() * 1.1 (the reference's own host
    read).  Write the result with gsgen_amd.io.write_obj."""
    from .density import get_density_val_grid_from_ckpt
    grid, L = get_density_val_grid_from_ckpt(ckpt, L=L, reso=reso, K=K)
    verts, tris = marching_cubes(grid, thresh)
    return index_to_world(verts, L, reso), tris, L


@torch.no_grad()
def vertex_attributes(verts, mean, qvec, scale, opacity, color=None, K=3, skip_nearest=True):
    """-> (normals [V,3], colors [V,3] or None) of mesh vertices in WORLD coordinates, from the field they were meshed from
    (gsgen_amd.density.field_at: one fused launch).  normal = -grad / |grad|: from high density to low, the side the triangles'
    winding faces; a zero or non-finite gradient gives a zero normal.  colors (when color [N,3] is given): the field's
    term-weighted average over the K + skip_nearest nearest centres.  Use the (K, skip_nearest) of the field that was meshed:
    DESIGN.md "Vertex normals and colours".  No vertices: empty tensors, no launch."""
    from .density import field_at
    if verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError(f"gsgen_amd.mesh: verts must be [V, 3], got {tuple(verts.shape)}")
    if verts.shape[0] == 0:
        empty = torch.empty(0, 3, device=mean.device, dtype=torch.float32)
        return empty, (None if color is None else empty.clone())
    _, grad, rgb = field_at(mean, qvec, scale, opacity, verts, K, skip_nearest, color=color, density=False, grad=True)
    big = grad.abs().amax(dim=1, keepdim=True)  # (scaled first: the squares of a tiny gradient must not underflow)
    ok = torch.isfinite(big) & (big > 0)
    g = grad / torch.where(ok, big, torch.ones_like(big))
    normals = torch.where(ok, -g / g.norm(dim=1, keepdim=True), torch.zeros_like(grad))
    return normals, rgb


@torch.no_grad()
def colored_density_mesh(mean, qvec, scale, opacity, color, L, reso, K=3, thresh=0.5, skip_nearest=True):
    """density_mesh with vertex_attributes of the same field -> (verts [V,3] world, tris [F,3] int32, normals [V,3], colors [V,3]);
    color [N,3] activated"""
    verts, tris = density_mesh(mean, qvec, scale, opacity, L, reso, K, thresh, skip_nearest)
    normals, colors = vertex_attributes(verts, mean, qvec, scale, opacity, color, K, skip_nearest)
    return verts, tris, normals, colors


@torch.no_grad()
def colored_mesh_from_ckpt(ckpt, reso=128, K=3, thresh=0.5, L=-1.0):
    """mesh_from_ckpt with vertex normals and colours -> (verts, tris, normals, colors, L).  ckpt also holds the raw "color";
    colours are sigmoid(color), as to_splat activates them (utils/export.py:254).  Write the result with
    gsgen_amd.io.write_obj(path, verts, tris, normals, colors) or write_ply_mesh."""
    verts, tris, L = mesh_from_ckpt(ckpt, reso=reso, K=K, thresh=thresh, L=L)
    normals, colors = vertex_attributes(verts, ckpt["mean"], ckpt["qvec"], torch.exp(ckpt["svec"]), torch.sigmoid(ckpt["alpha"]),
                                        torch.sigmoid(ckpt["color"]), K, True)
    return verts, tris, normals, colors, L
