"""render_one(overrides={"color": t}) of gsgen_amd.model.GaussianSplattingRenderer on the MI355X: an already-activated colour tensor
rendered in place of the model's -- the same render as the plain forward when it holds the model's own colours, another image when it
does not, with gradients to the tensor -- on the heads path (activation "nothing") and with rgb_only."""
import pytest
import torch

import scenes as S

pytestmark = pytest.mark.gpu
DEV = "cuda"


def small_model():
    from gsgen_amd.model import GaussianSplattingRenderer
    from gsgen_amd.renderer import CameraInfo
    cfg = dict(device=DEV, svec_act="exp", alpha_act="sigmoid", color_act="sigmoid", tile_size=16, T_thresh=1e-4, depth_detach=True,
               background=dict(type="fixed", color=[0.1, 0.2, 0.3]), densify=dict(enabled=False), prune=dict(enabled=False))
    sc = S.pointe_scene(2000, seed=3, svec=0.03, C=1)
    init = {k: torch.tensor(sc[k], device=DEV) for k in ("mean", "qvec", "svec", "color", "alpha")}
    cam = S.Camera(64, 64, fx=70.0, c2w=S.orbit(3.0, 20.0, 30.0))
    m = GaussianSplattingRenderer(cfg, init)
    return m, {"c2w": torch.tensor(cam.c2w)[None], "camera_info": [CameraInfo(*cam.intr)]}, torch.tensor(cam.c2w), CameraInfo(*cam.intr)


@pytest.mark.parametrize("rgb_only", [True, False])
def test_colour_override_with_the_models_colours_is_the_plain_render(rgb_only):
    m, batch, c2w, ci = small_model()
    plain = m(batch, rgb_only=rgb_only)
    col = m.color.detach().clone().requires_grad_(True)
    one = m.render_one(c2w, ci, rgb_only=rgb_only, overrides={"color": col})
    assert set(one) == set(plain) == ({"rgb"} if rgb_only else {"rgb", "depth", "opacity", "z_var"})
    for k in plain:
        assert one[k].shape == plain[k].shape[1:]
        assert float((plain[k][0] - one[k]).abs().max()) <= 1e-6, k
    assert float(plain["rgb"].std()) > 0.02  # (an image, not a background)
    one["rgb"].sum().backward()
    assert col.grad is not None and float(col.grad.abs().max()) > 0 and m.mean.grad is not None
    assert m.color_before_activation.grad is None  # (the model's own colours took no part)


@pytest.mark.parametrize("rgb_only", [True, False])
def test_colour_override_is_what_gets_rendered(rgb_only):
    m, batch, c2w, ci = small_model()
    plain = m.render_one(c2w, ci, rgb_only=rgb_only)
    red = torch.zeros(m.N, 3, device=DEV)
    red[:, 0] = 1.0
    one = m.render_one(c2w, ci, rgb_only=rgb_only, overrides={"color": red})
    again = m.render_one(c2w, ci, rgb_only=rgb_only, overrides={"color": red.clone()})
    assert torch.equal(one["rgb"], again["rgb"])
    assert float((one["rgb"] - plain["rgb"]).abs().max()) > 0.05
    # every pixel is background * T + red * (1 - T): green and blue are the background's share alone
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    T = one["rgb"][..., 1] / bg[1]
    assert float((one["rgb"][..., 2] - T * bg[2]).abs().max()) <= 1e-6
    assert float((one["rgb"][..., 0] - (T * bg[0] + (1 - T))).abs().max()) <= 2e-6
    if not rgb_only:
        for k in ("depth", "opacity", "z_var"):
            assert torch.equal(one[k], plain[k]), k  # (the colour plays no part in the other heads)


def test_other_overrides_and_wrong_shapes_are_refused():
    m, batch, c2w, ci = small_model()
    with pytest.raises(NotImplementedError, match="mean"):
        m.render_one(c2w, ci, overrides={"mean": m.mean.detach()})
    with pytest.raises(ValueError):
        m.render_one(c2w, ci, overrides={"color": m.color.detach()[:10]})
    out = m.render_one(c2w, ci, overrides={})
    assert torch.equal(out["rgb"], m.render_one(c2w, ci, overrides=None)["rgb"])
