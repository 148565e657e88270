"""gsgen_amd -- MI355X (gfx950) differentiable Gaussian-splatting rasterizer, a drop-in for the
`_gs` extension of gsgen3d/gsgen.

    gsgen_amd/ext/_gs    the compiled `_gs` module (csrc/torch_gs.cpp over the C ABI): the reference's pybind surface
    gsgen_amd._gs        ctypes mirror of the same 23 names (no compiler needed at install time)
    gsgen_amd.renderer   HIP projection, fused RGB + heads, the fused `render_frame`
    gsgen_amd.batch      camera batches: one enqueue per stage for all cameras of a batch
    gsgen_amd.dist       camera sharding across GPUs (one process per GPU, RCCL all_gather)
    gsgen_amd.optim      one flat Adam step over the replicated parameters
    gsgen_amd.densify    the reference's densify / prune bookkeeping, identical on every rank (pure torch)
    gsgen_amd.io         the reference's checkpoint / .ply / .splat formats
    gsgen_amd.loss       the fused SSIM + L1 / L2 image loss of utils/loss.py (ssim_loss, image_loss, get_image_loss, get_loss_fn)
                         and its Pearson depth loss (depth_loss, pearson_depth_loss, pearson_depth_loss_terms); the trainer's map
                         regularisers (map_loss, map_loss_terms, sparsity_loss, opague_loss, z_var_loss, get_map_loss)
    gsgen_amd.background the learned MLP background of conf/renderer/mlp_bg.yaml fused with its composite (MLPBackground, mlp_background,
                         mlp_background_images, mlp_background_over)
    gsgen_amd.mesh       marching cubes on the GPU and the mesh export built on it (marching_cubes, density_mesh, mesh_from_ckpt), with vertex
                         normals and colours from the same field (vertex_attributes, colored_density_mesh, colored_mesh_from_ckpt)
    gsgen_amd.mesh_sample  a triangle mesh to an evenly spaced point cloud on the GPU, trimesh's call shapes (mesh_area, sample_surface,
                         remove_close, sample_surface_even), and the reference's mesh initialisation on it (load_mesh_as_pcd, mesh_initialize)
    gsgen_amd.guidance   the seam between the rendered batch and the diffusion guidance: the fused resize + affine + fp16 cast of the
                         guidance's input (to_guidance, vae_input, if_input, rgb_as_latents, resize) and the SDS loss (sds_loss)
    gsgen_amd.build      hipcc build of gsgen_amd/lib/libgsgen_hip.so (C ABI: include/gsgen_hip.h)

There is no CPU implementation in this package: every entry point needs the HIP library and
a GPU, and raises if either is missing.
"""
import sys

__version__ = "0.1.0"


def __getattr__(name):  # (lazy: importing the package must not import torch)
    if name == "PairListOverflow":
        from .renderer import PairListOverflow
        return PairListOverflow
    if name in ("ssim_loss", "image_loss", "get_image_loss", "get_loss_fn", "depth_loss", "pearson_depth_loss", "pearson_depth_loss_terms",
                "map_loss", "map_loss_terms", "sparsity_loss", "opague_loss", "z_var_loss", "get_map_loss"):
        from . import loss
        return getattr(loss, name)
    if name in ("MLPBackground", "mlp_background", "mlp_background_images", "mlp_background_over"):
        from . import background
        return getattr(background, name)
    if name == "mesh":
        import importlib
        return importlib.import_module(".mesh", __name__)
    if name in ("marching_cubes", "marching_cubes_into", "density_mesh", "mesh_from_ckpt", "vertex_attributes", "colored_density_mesh",
                "colored_mesh_from_ckpt"):
        from . import mesh
        return getattr(mesh, name)
    if name == "mesh_sample":
        import importlib
        return importlib.import_module(".mesh_sample", __name__)
    if name in ("mesh_area", "sample_surface", "remove_close", "sample_surface_even", "load_mesh_as_pcd", "mesh_initialize"):
        from . import mesh_sample
        return getattr(mesh_sample, name)
    if name == "guidance":
        import importlib
        return importlib.import_module(".guidance", __name__)
    if name in ("to_guidance", "vae_input", "if_input", "rgb_as_latents", "sds_loss"):
        from . import guidance
        return getattr(guidance, name)
    raise AttributeError(name)


def compiled_gs():
    """The compiled `_gs` CPython module (gsgen_amd/ext/_gs.*.so, built by gsgen_amd.build.build_torch_ext from
    csrc/torch_gs.cpp: torch::Tensor in, C ABI underneath -- what the reference builds from gs/src/bindings.cpp), or
    None when it has not been built."""
    import glob
    import importlib.util
    import os
    hits = glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ext", "_gs.*.so"))
    if not hits:
        return None
    import torch  # noqa: F401  (its HIP runtime and libtorch go first: one libamdhip64 per process)
    spec = importlib.util.spec_from_file_location("_gs", hits[0])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def install_as_gs(compiled=True):
    """Register this package's `_gs` as the top-level module `_gs`, which is what the reference's Python imports
    (`import _gs as _backend`, gs/renderer.py:20-24): the compiled extension when it is built (compiled=True, ~5 us of
    host time per call), else the ctypes mirror gsgen_amd._gs (same names, argument orders and errors)."""
    mod = compiled_gs() if compiled else None
    if mod is None:
        from . import _gs as mod
    sys.modules["_gs"] = mod
    return mod
