"""gsgen_amd.background on the MI355X against the torch restatement of tests/background_cases.py, to the bound that restatement's own
fp32 error sets (no fixed tolerance), and the properties a trainer relies on: the upstream gradient passed through to rgb bit for bit,
bit equality from run to run, linearity in the upstream gradient, the reference's state-dict key, a captured forward + backward whose
replay reads new parameters AND new cameras, and the model class with background.type "mlp" on both of its render paths."""
import numpy as np
import pytest
import torch

import background_cases as BC
import scenes
from refpy_cases import rel_rows

pytestmark = pytest.mark.gpu

from gsgen_amd import background as GB  # noqa: E402

DEV = "cuda"


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def on_device(name, stride_floats=68):
    """the case's tensors on the GPU: params (a leaf), cams [B, stride] as the renderer holds them, rgb and opacity (leaves), grad"""
    c = BC.case(name)
    t = dict(params=c["params"].to(DEV).requires_grad_(True), cams=BC.cam_blocks(c, stride_floats).to(DEV),
             rgb=c["rgb"].to(DEV).requires_grad_(True), opacity=c["opacity"].to(DEV).requires_grad_(True), grad=c["grad"].to(DEV))
    return c, t


def run_over(t, scale=1.0):
    """-> (out, d params, d rgb, d opacity) of <scale * grad, over(rgb, opacity)>"""
    for k in ("params", "rgb", "opacity"):
        t[k].grad = None
    out = GB.mlp_background_over(t["params"], t["rgb"], t["opacity"], t["cams"])
    out.backward(scale * t["grad"])
    return out.detach(), t["params"].grad.clone(), t["rgb"].grad.clone(), t["opacity"].grad.clone()


@pytest.mark.parametrize("name", BC.NAMES)
def test_background_meets_the_restatements_own_error(name):
    c, t = on_device(name)
    B, H, W = c["shape"]
    bg = GB.mlp_background_images(t["params"], t["cams"], H, W)
    assert bg.shape == (B, H, W, 3) and bg.dtype == torch.float32 and bg.requires_grad
    bg.backward(t["grad"])
    BC.check(name, "bg", bg)
    BC.check(name, "gp_plain", t["params"].grad)
    out, gp, g_rgb, g_op = run_over(t)
    BC.check(name, "out", out)
    BC.check(name, "gp_over", gp)
    BC.check(name, "g_opacity", g_op)
    assert torch.equal(bits(g_rgb), bits(t["grad"]))            # d out / d rgb = 1: the upstream gradient itself
    assert not gp[512 + 48:].any() and gp[:512 + 48].any()      # W2's padding rows: exactly zero
    # the reference's call, bg(rays_d), on the fp32 restatement's rays: one camera, [H, W, 3]
    dirs = c["r32"]["dirs"].to(DEV)
    p2 = t["params"].detach().clone().requires_grad_(True)
    per_view = torch.stack([GB.mlp_background(p2, dirs[b]) for b in range(B)])
    assert per_view.shape == (B, H, W, 3)
    per_view.backward(t["grad"])
    BC.check(name, "bg", per_view)
    BC.check(name, "gp_plain", p2.grad)


def test_bit_identical_from_run_to_run_and_an_upstream_scale_of_two_doubles_the_gradients():
    c, t = on_device("views-3x64x64")
    a, b, two = run_over(t), run_over(t), run_over(t, 2.0)
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y))
    assert torch.equal(bits(two[0]), bits(a[0]))
    for x, y in zip(two[1:], a[1:]):
        assert torch.equal(bits(x), bits(2.0 * y)) and y.abs().max() > 0
    # 16-float camera blocks (a stand-alone caller's) give the same bits as the renderer's 68-float rows
    _, t16 = on_device("views-3x64x64", stride_floats=16)
    for x, y in zip(a, run_over(t16)):
        assert torch.equal(bits(x), bits(y))


def test_state_dict_round_trip_under_the_references_key():
    torch.manual_seed(3)
    a = GB.MLPBackground({"type": "mlp", "device": DEV})
    assert list(a.state_dict()) == ["mlp.params"] and a.mlp.params.is_cuda and a.mlp.params.shape == (768,)
    saved = {k: v.cpu().clone() for k, v in a.state_dict().items()}
    b = GB.MLPBackground({"type": "mlp", "device": DEV})
    assert not torch.equal(a.mlp.params, b.mlp.params)
    b.load_state_dict(saved)
    assert torch.equal(bits(a.mlp.params), bits(b.mlp.params))
    c = BC.case("one-1x16x16")
    cams = BC.cam_blocks(c).to(DEV)
    assert torch.equal(bits(a.images(cams, 1, 16, 16)), bits(b.images(cams, 1, 16, 16)))
    dirs = c["r32"]["dirs"][0].to(DEV)
    assert torch.equal(bits(a(dirs)), bits(b(dirs))) and a(dirs).shape == (16, 16, 3)
    rgb, op = c["rgb"].to(DEV), c["opacity"].to(DEV)
    assert torch.equal(bits(a.over(rgb, op, cams)), bits(rgb + (1 - op) * a.images(cams, 1, 16, 16)))  # (unfused: mul, then add)


def test_forward_and_backward_replay_in_a_captured_graph_on_new_parameters_and_new_cameras():
    name, other = "tail-2x37x53", BC.make_inputs((2, 37, 53), 1.0, 777)
    c, t = on_device(name)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run_over(t)  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    for k in ("params", "rgb", "opacity"):
        t[k].grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = GB.mlp_background_over(t["params"], t["rgb"], t["opacity"], t["cams"])
        out.backward(t["grad"])
    new_cams = BC.cam_blocks(dict(c2w=other["c2w"], intr=other["intr"]), 68).to(DEV)
    with torch.no_grad():
        t["params"].copy_(other["params"].to(DEV))
        t["cams"].copy_(new_cams)
        t["grad"].mul_(-0.5)
    graph.replay()
    torch.cuda.synchronize()
    got = [x.clone() for x in (out, t["params"].grad, t["rgb"].grad, t["opacity"].grad)]
    e = dict(params=other["params"].to(DEV).requires_grad_(True), cams=new_cams.clone(), rgb=t["rgb"].detach().clone().requires_grad_(True),
             opacity=t["opacity"].detach().clone().requires_grad_(True), grad=t["grad"].clone())
    want = run_over(e)
    for a, b in zip(got, want):
        assert torch.equal(bits(a), bits(b))
    first = run_over(on_device(name)[1])
    assert not torch.equal(bits(got[0]), bits(first[0])) and not torch.equal(bits(got[1]), bits(first[1]))  # (it did read the new ones)


# --- the model class with background.type "mlp" --------------------------------------------------------------------------
W_, H_ = 48, 40


@pytest.fixture(scope="module")
def tiny():
    """about 200 Gaussians, 2 views of 48 x 40 with fx != fy and off-centre principal points; the model and what the tests compare it
    with: its parameters' names, the cameras and the restatement's background in fp64 and fp32 (CPU)"""
    from gsgen_amd.model import GaussianSplattingRenderer
    from gsgen_amd.renderer import CameraInfo
    sc = scenes.random_scene(200, seed=7, svec=0.12)
    cfg = dict(device=DEV, svec_act="exp", alpha_act="sigmoid", color_act="sigmoid", tile_size=16, T_thresh=1e-4, depth_detach=True,
               background=dict(type="mlp"), densify=dict(enabled=False), prune=dict(enabled=False))
    init = {k: torch.tensor(sc[k], device=DEV) for k in ("mean", "qvec", "svec", "color", "alpha")}
    cams = [scenes.Camera(W_, H_, fx=52.0 + 9 * i, fy=47.0 - 4 * i, cx=22.5 + 3 * i, cy=21.0 - 2 * i, c2w=scenes.orbit(2.6, 15 + 10 * i, 40.0 + 80 * i))
            for i in range(2)]
    torch.manual_seed(5)
    m = GaussianSplattingRenderer(cfg, init)
    m.train()
    batch = {"c2w": torch.tensor(np.stack([cam.c2w for cam in cams])), "camera_info": [CameraInfo(*cam.intr) for cam in cams]}
    c2w = torch.tensor(np.stack([cam.c2w[:3, :4] for cam in cams]), dtype=torch.float32)
    intr = torch.tensor([[cam.fx, cam.fy, cam.cx, cam.cy] for cam in cams], dtype=torch.float32)
    p = m.bg.mlp.params.detach().cpu()
    bg64 = BC.background_torch(p.double(), BC.rays_torch(c2w.double(), intr.double(), H_, W_))
    bg32 = BC.background_torch(p, BC.rays_torch(c2w, intr, H_, W_))
    gen = torch.Generator().manual_seed(9)
    return dict(m=m, batch=batch, c2w=c2w, intr=intr, bg64=bg64, bg32=bg32, grad=torch.randn(2, H_, W_, 3, generator=gen).to(DEV))


def model_grads(m):
    names = ("mean", "qvec", "svec_before_activation", "color_before_activation", "alpha_before_activation")
    out = {k: getattr(m, k).grad.cpu().numpy().copy() for k in names if getattr(m, k).grad is not None}
    if m.bg.mlp.params.grad is not None:
        out["bg"] = m.bg.mlp.params.grad.cpu().numpy().copy()
    for k in names:
        getattr(m, k).grad = None
    m.bg.mlp.params.grad = None
    return out


def free_render(s, rgb_only, bg_rgb=None):
    """the model's Gaussians through its own BatchRenderer without the model's background: -> (rgb, T or opacity)"""
    m, b = s["m"], s["batch"]
    br = m.batch_renderer(b)
    c2ws = b["c2w"].numpy().astype(np.float32)
    kw = dict(thresh=m.T_thresh, frustum_radius=m.frustum_culling_radius, tile_radius=m.tile_culling_radius, detach_depth=m.depth_detach)
    if rgb_only:
        return br.render(m.mean, m.qvec, m.svec, m.alpha, m.color, b["camera_info"], c2ws, C=0, bg_rgb=bg_rgb, **kw)
    out = br.render_heads(m.mean, m.qvec, m.svec, m.alpha, m.color, b["camera_info"], c2ws, bg_rgb=None, **kw)
    return out[0], out[2]


@pytest.mark.parametrize("rgb_only", [True, False])
def test_model_with_an_mlp_background_renders_and_differentiates_as_the_torch_composition(tiny, rgb_only):
    s = tiny
    m = s["m"]
    out = m(s["batch"], rgb_only=rgb_only)
    assert set(out) == ({"rgb"} if rgb_only else {"rgb", "depth", "opacity", "z_var"}) and out["rgb"].shape == (2, H_, W_, 3)
    out["rgb"].backward(s["grad"])
    got = model_grads(m)
    # the image: the background-free render composited in torch with the restatement's background, to the restatement's own error
    with torch.no_grad():
        rgb_free, w = free_render(s, rgb_only)
    w = (w if rgb_only else 1 - w).cpu()      # T, or 1 - opacity
    assert 0.2 < float(w.mean()) < 0.95       # (Gaussians and background both show)
    want64 = rgb_free.cpu().double() + w.double() * s["bg64"]
    want32 = rgb_free.cpu() + w * s["bg32"]
    bound, e32 = BC.tensor_bound(want64, want32)
    err = float((out["rgb"].detach().cpu().double() - want64).abs().max())
    print(f"model image rgb_only={rgb_only}: err {err:.3e} (fp32 torch {e32:.3e}, bound {bound:.3e})")
    assert err <= bound
    # the gradients: the same composition differentiated by torch on the device, at the suite's rtol 1e-3 per Gaussian
    p_ref = m.bg.mlp.params.detach().clone().requires_grad_(True)
    bg_ref = BC.background_torch(p_ref, BC.rays_torch(s["c2w"].to(DEV), s["intr"].to(DEV), H_, W_))
    if rgb_only:
        ref, _ = free_render(s, True, bg_rgb=bg_ref)  # (T carries no graph: the compositing entry differentiates rgb + T bg itself)
    else:
        rgb_free, opacity = free_render(s, False)
        ref = rgb_free + (1 - opacity) * bg_ref
    ref.backward(s["grad"])
    want = model_grads(m)
    want["bg"] = p_ref.grad.cpu().numpy()
    assert set(got) == set(want)
    for k in want:
        assert np.isfinite(got[k]).all() and np.abs(want[k]).max() > 0, k
        g, w_ = (got[k][None], want[k][None]) if k == "bg" else (got[k], want[k])
        r = rel_rows(g, w_)
        print(f"model gradient {k} rgb_only={rgb_only}: worst row at {r:.3f} of its tolerance")
        assert r <= 1.0, k


@pytest.mark.parametrize("rgb_only", [True, False])
def test_a_captured_step_draws_the_background_of_the_replays_cameras(tiny, rgb_only):
    """model.device_cameras: the background reads the renderer's device camera blocks, so a replay for other cameras (uploaded by
    CapturedStep, nothing else) equals an eager step of a second model on those cameras"""
    from gsgen_amd.graph import CapturedStep
    from gsgen_amd.model import GaussianSplattingRenderer
    from gsgen_amd.renderer import CameraInfo
    src, grad = tiny["m"], tiny["grad"]
    saved = src.get_params_for_save()
    other = [scenes.Camera(W_, H_, fx=44.0 + 12 * i, fy=58.0 - 7 * i, cx=25.0 - 2 * i, cy=18.5 + 2 * i, c2w=scenes.orbit(2.3, 40 - 30 * i, 200.0 + 70 * i))
             for i in range(2)]
    sets = {"first": (tiny["batch"]["camera_info"], tiny["batch"]["c2w"].numpy().astype(np.float32)),
            "other": ([CameraInfo(*cam.intr) for cam in other], np.stack([cam.c2w for cam in other]).astype(np.float32))}

    def make(device_cameras):
        m = GaussianSplattingRenderer(src.cfg, {"raw": True, "mean": saved["mean"].clone(), "qvec": saved["qvec"].clone(),
                                                "svec": saved["svec_before_activation"].clone(), "color": saved["color_before_activation"].clone(),
                                                "alpha": saved["alpha_before_activation"].clone()})
        m.bg.load_state_dict(saved["bg"])
        m.train()
        m.device_cameras = device_cameras
        params = [m.mean, m.alpha_before_activation, m.bg.mlp.params]

        def step(cis, c2ws):
            for q in params:
                q.grad = None
            rgb = m({"c2w": c2ws, "camera_info": cis}, rgb_only=rgb_only)["rgb"]
            rgb.backward(grad)
            m.post_backward()
            return rgb, [q.grad for q in params]
        return m, step

    def snap(res):
        torch.cuda.synchronize()
        return [res[0].detach().cpu().numpy().copy()] + [g.detach().cpu().numpy().copy() for g in res[1]]

    _, step_e = make(False)
    eager = {k: snap(step_e(*sets[k])) for k in sets}
    cs = CapturedStep(*make(True), *sets["first"])
    for k in ("other", "first", "other"):
        got = snap(cs(*sets[k]))
        assert np.abs(got[0] - eager[k][0]).max() <= 1e-5, k
        for a, b in zip(got[1:], eager[k][1:]):
            assert rel_rows(a.reshape(1, -1), b.reshape(1, -1)) <= 1.0, k
    assert cs.captures == 1 and cs.replays == 3
    assert np.abs(eager["first"][0] - eager["other"][0]).mean() > 0.02  # (the two camera sets really differ)


def test_model_optimiser_and_saved_parameters_carry_the_background(tiny):
    m, s = tiny["m"], tiny
    m.setup_lr(dict(mean=1e-3, qvec=1e-3, svec=1e-3, color=1e-2, alpha=1e-2, bg=1e-2))
    m.set_optimizer(dict(type="Adam", opt_args=dict(eps=1e-15)))
    groups = {g["name"]: g for g in m.optimizer.param_groups}
    assert "bg" in groups and groups["bg"]["lr"] == 1e-2 and groups["bg"]["params"][0] is m.bg.mlp.params
    before = m.bg.mlp.params.detach().clone()
    m.optimizer.zero_grad()
    m(s["batch"])["rgb"].square().mean().backward()
    m.optimizer.step()
    moved = (m.bg.mlp.params.detach() - before).abs()
    assert float(moved[:560].min()) >= 0 and float(moved.max()) > 1e-3 and not moved[560:].any()  # (Adam leaves a zero gradient's entry)
    with torch.no_grad():
        m.bg.mlp.params.copy_(before)
    m.optimizer = None
    saved = m.get_params_for_save()
    assert list(saved["bg"]) == ["mlp.params"] and torch.equal(saved["bg"]["mlp.params"], m.bg.mlp.params)
    from gsgen_amd.model import GaussianSplattingRenderer
    cfg = dict(m.cfg, background=dict(type="fixed", color=[0.1, 0.2, 0.3]))
    other = GaussianSplattingRenderer(cfg, {"raw": True, **{k: saved[k].clone() for k in ("mean", "qvec")},
                                            "svec": saved["svec_before_activation"].clone(), "color": saved["color_before_activation"].clone(),
                                            "alpha": saved["alpha_before_activation"].clone()})
    assert "bg" not in other.get_params_for_save()  # (every other type saves what it saved before)
