"""gsgen_amd.mesh_sample.mesh_initialize on the MI355X (utils/initialize.py:285-332 restated on the GPU sampler): shapes and
dtypes, the centring and scaling identities, both flips, svec from the neighbour search, interpolated vertex colours, a mesh file,
and the round trip model -> to_mesh -> mesh_initialize -> a new model that renders."""
import numpy as np
import pytest
import torch

import mesh_sample_cases as MC
import scenes as S

pytestmark = pytest.mark.gpu
DEV = "cuda"


def cfg(**kw):
    base = dict(num_points=1500, mean_std=0.8, svec_val=0.02, alpha_val=0.8)
    base.update(kw)
    return base


def gen(seed=7):
    return torch.Generator(device=DEV).manual_seed(seed)


def test_mesh_initialize_on_an_icosphere():
    from gsgen_amd.knn import nearest_neighbor_initialize
    from gsgen_amd.mesh_sample import mesh_initialize
    verts, tris = MC.icosphere(3)
    verts = verts * np.float32(2.5) + np.asarray([3.0, -1.0, 0.5], np.float32)  # (off centre, not unit size)
    iv = mesh_initialize(cfg(), verts, tris, generator=gen())
    assert set(iv) == {"mean", "color", "svec", "qvec", "alpha", "raw"} and iv["raw"] is False
    shapes = {"mean": (1500, 3), "color": (1500, 3), "svec": (1500, 3), "qvec": (1500, 4), "alpha": (1500,)}
    for k, s in shapes.items():
        assert iv[k].shape == s and iv[k].dtype == torch.float32 and iv[k].is_cuda, k
    mean = iv["mean"].double()
    assert float(mean.mean(0).abs().max()) < 1e-6  # centred
    assert abs(float(mean.norm(dim=1).max()) - 0.8) < 1e-4  # max norm = mean_std (up to the 1e-5 of the reference's division)
    assert float(mean.norm(dim=1).min()) > 0.7  # a sphere stays a sphere (the sample mean is not its centre exactly)
    assert bool((iv["svec"] == 0.02).all()) and bool((iv["alpha"] == 0.8).all())
    assert bool((iv["qvec"] == torch.tensor([1.0, 0, 0, 0], device=DEV)).all())
    assert 0 <= float(iv["color"].min()) and float(iv["color"].max()) < 1 and float(iv["color"].std()) > 0.2  # random colours
    # the flips permute the columns of the same cloud (same generator state)
    yz = mesh_initialize(cfg(flip_yz=True), verts, tris, generator=gen())["mean"]
    xy = mesh_initialize(cfg(flip_xy=True), verts, tris, generator=gen())["mean"]
    both = mesh_initialize(cfg(flip_yz=True, flip_xy=True), verts, tris, generator=gen())["mean"]
    assert torch.equal(yz, iv["mean"][:, [0, 2, 1]]) and torch.equal(xy, iv["mean"][:, [1, 0, 2]])
    assert torch.equal(both, iv["mean"][:, [0, 2, 1]][:, [1, 0, 2]])
    # svec_val <= 0: the mean squared distance to the three nearest neighbours, on every axis
    nn = mesh_initialize(cfg(svec_val=-1.0), verts, tris, generator=gen())
    assert torch.equal(nn["mean"], iv["mean"])
    want = nearest_neighbor_initialize(nn["mean"], k=3)
    assert torch.equal(nn["svec"].cpu(), want[:, None].repeat(1, 3)) and float(want.min()) > 0
    # cfg.num_points is honoured through the top-up loop, and an attribute-style cfg works
    class Cfg:
        num_points, mean_std, svec_val, alpha_val = 4000, 1.0, 0.01, 0.5
    assert mesh_initialize(Cfg(), verts, tris, generator=gen())["mean"].shape == (4000, 3)


def test_vertex_colours_are_interpolated_when_random_color_is_off(tmp_path):
    from gsgen_amd import io as GIO
    from gsgen_amd.mesh_sample import mesh_initialize
    verts, tris = MC.icosphere(2)
    colors = (0.25 + 0.25 * (verts + 1)).astype(np.float32)  # an affine function of the position: interpolation reproduces it
    iv = mesh_initialize(cfg(num_points=800, mean_std=1.0, random_color=False), verts, tris, colors, generator=gen())
    # mean = (p - c) / (max |p - c| + 1e-5) with p on the mesh: the colour at p is 0.25 + 0.25 (p + 1); undo the normalisation
    # through the sampler itself: the same generator state draws the same samples
    from gsgen_amd.mesh_sample import _even_cloud, _mesh
    p, a = _even_cloud(*_mesh(verts, tris), 800, gen(), torch.tensor(colors, device=DEV))
    assert torch.equal(a, iv["color"])
    bound = 2 * MC.C_POINT * MC.EPS * 2.0  # (both sides carry the bound, on values up to 1 (positions) and 0.75 (colours))
    assert float((iv["color"].double() - (0.25 + 0.25 * (p.double() + 1))).abs().max()) <= bound
    rnd = mesh_initialize(cfg(num_points=800, mean_std=1.0), verts, tris, colors, generator=gen())  # random_color defaults to True
    assert not torch.equal(rnd["color"], iv["color"]) and torch.equal(rnd["mean"], iv["mean"])
    # from a file (cfg.mesh): .obj keeps float colours
    path = tmp_path / "ball.obj"
    GIO.write_obj(path, verts, tris, None, colors)
    fv = mesh_initialize(cfg(num_points=800, mean_std=1.0, random_color=False, mesh=str(path)), generator=gen())
    assert torch.equal(fv["mean"], iv["mean"]) and float((fv["color"] - iv["color"]).abs().max()) <= 1e-6
    with pytest.raises(FileNotFoundError):
        mesh_initialize(cfg(mesh=str(tmp_path / "none.obj")))


def test_round_trip_model_to_mesh_to_a_new_model():
    """a small seeded model -> to_mesh at reso 32 -> mesh_initialize -> a new GaussianSplattingRenderer whose forward renders a
    finite image that is not the background alone"""
    from gsgen_amd.mesh_sample import mesh_initialize
    from gsgen_amd.model import GaussianSplattingRenderer
    from gsgen_amd.renderer import CameraInfo
    mcfg = dict(device=DEV, svec_act="exp", alpha_act="sigmoid", color_act="sigmoid", tile_size=16, T_thresh=1e-4, depth_detach=True,
                background=dict(type="fixed", color=[0.1, 0.2, 0.3]), densify=dict(enabled=False), prune=dict(enabled=False))
    g = torch.Generator().manual_seed(200)
    N = 200
    init = dict(mean=(torch.randn(N, 3, generator=g) * 0.3).clamp(-0.7, 0.7), qvec=torch.randn(N, 4, generator=g),
                svec=0.1 + 0.1 * torch.rand(N, 3, generator=g), color=torch.rand(N, 3, generator=g), alpha=torch.full((N,), 0.88))
    m = GaussianSplattingRenderer(mcfg, {k: v.to(DEV) for k, v in init.items()})
    verts, tris, normals, colors, L = m.to_mesh(reso=32, L=1.5)
    assert tris.shape[0] > 200
    iv = mesh_initialize(cfg(num_points=1000, mean_std=0.5, svec_val=0.03, random_color=False), verts, tris, colors, generator=gen())
    assert iv["mean"].shape == (1000, 3) and 0 <= float(iv["color"].min()) and float(iv["color"].max()) <= 1
    m2 = GaussianSplattingRenderer(mcfg, iv)
    cams = [S.Camera(64, 64, fx=70.0, c2w=S.orbit(3.0, 20.0, az)) for az in (30.0, 140.0)]
    out = m2({"c2w": torch.tensor(np.stack([c.c2w for c in cams])), "camera_info": [CameraInfo(*c.intr) for c in cams]})
    assert out["rgb"].shape == (2, 64, 64, 3) and bool(torch.isfinite(out["rgb"]).all())
    assert float(out["opacity"].detach().max()) > 0.5 and float(out["rgb"].detach().std()) > 0.02  # an image, not a background
