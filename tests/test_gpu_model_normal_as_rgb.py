"""cfg.normal_as_rgb of gsgen_amd.model.GaussianSplattingRenderer on the MI355X (conf/renderer/normal_as_rgb.yaml: neighbourhood 30,
disambiguated): forward(batch) renders the estimated normals as colours through the fused batched path and normalises every pixel,
gs/gaussian_splatting.py:1424-1427, :1463-1464.  A 600-Gaussian noisy shell, two 64 x 64 cameras."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import normals_cases as NC
import scenes as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
NORMAL = dict(neighborhood_size=30, disambiguate_directions=True)


def shell_model(**extra):
    from gsgen_amd.model import GaussianSplattingRenderer
    from gsgen_amd.renderer import CameraInfo
    cfg = dict(device=DEV, svec_act="exp", alpha_act="sigmoid", color_act="sigmoid", tile_size=16, T_thresh=1e-4, depth_detach=True,
               background=dict(type="fixed", color=[0.1, 0.2, 0.3]), densify=dict(enabled=False), prune=dict(enabled=False), **extra)
    rng = np.random.default_rng(12)
    N = 600
    init = dict(mean=NC.shell(N, 11) * np.float32(0.5), qvec=rng.normal(size=(N, 4)).astype(np.float32),
                svec=np.full((N, 3), 0.04, np.float32), color=rng.uniform(0.1, 0.9, (N, 3)).astype(np.float32),
                alpha=rng.uniform(0.3, 0.9, N).astype(np.float32))
    cams = [S.Camera(64, 64, fx=70.0, c2w=S.orbit(3.0, 20.0, az)) for az in (30.0, 140.0)]
    m = GaussianSplattingRenderer(cfg, {k: torch.tensor(v, device=DEV) for k, v in init.items()})
    batch = {"c2w": torch.tensor(np.stack([c.c2w for c in cams])), "camera_info": [CameraInfo(*c.intr) for c in cams]}
    return m, batch


@pytest.mark.parametrize("rgb_only", [True, False])
def test_forward_renders_the_estimated_normals(rgb_only):
    from gsgen_amd.normals import estimate_normal
    m, batch = shell_model(normal_as_rgb=True, normal=NORMAL)
    out = m(batch, rgb_only=rgb_only)
    assert set(out) == ({"rgb"} if rgb_only else {"rgb", "depth", "opacity", "z_var"}) and out["rgb"].shape == (2, 64, 64, 3)
    got = {k: v.detach().clone() for k, v in out.items()}
    out["rgb"].sum().backward()  # (before the next render: a batch's backward needs its own forward's lists)
    g = m.mean.grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert m.color_before_activation.grad is None  # (the model's colours take no part; the override is a constant)
    with torch.no_grad():
        r = m._render(batch, rgb_only=rgb_only, color=(estimate_normal(m.mean, 30, True) + 1) / 2)
        want = (F.normalize(r["rgb"], dim=-1, eps=1e-6) + 1) / 2
    assert torch.equal(got["rgb"].view(torch.int32), want.view(torch.int32))
    assert float(got["rgb"].std()) > 0.02  # (an image, not a background)
    for k in set(got) - {"rgb"}:
        assert torch.equal(got[k], r[k]), k
    m.render_one(batch["c2w"][0], batch["camera_info"][0])  # render_one does not apply the view: plain colours


def test_normal_property_and_update_normal():
    from gsgen_amd.normals import estimate_normal
    m, _ = shell_model(normal_as_rgb=True, normal=NORMAL)
    n = m.update_normal()
    assert n.shape == (600, 3) and not n.requires_grad
    assert torch.equal(n, m.normal) and torch.equal(n, estimate_normal(m.mean, **NORMAL)) and torch.equal(n, m._normal)
    # a shell's normals are radial: the disambiguated ones point inwards, where the neighbours lie
    rad = F.normalize(m.mean.detach(), dim=-1)
    assert float(((n * rad).sum(-1) < -0.9).float().mean()) > 0.95


def test_what_is_still_refused():
    with pytest.raises(NotImplementedError, match="pbr"):
        shell_model(pbr=True)
    with pytest.raises(NotImplementedError, match="pbr"):
        shell_model(pbr=True, normal_as_rgb=True, normal=NORMAL)
    m, batch = shell_model(normal_as_rgb=True, normal=NORMAL, normal_type="learned")
    with pytest.raises(NotImplementedError, match="learned"):
        m.normal
    with pytest.raises(NotImplementedError, match="learned"):
        m(batch)


def test_without_normal_as_rgb_nothing_changes():
    plain, batch = shell_model()
    off, _ = shell_model(normal_as_rgb=False)
    a, b = plain(batch), off(batch)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert off._normal is None
