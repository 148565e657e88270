"""The trainer's default outputs -- rgb with a background, depth, opacity, depth^2 or z_var (gs/gaussian_splatting.py:1304-1403) --
and their backward held to central differences of the independent fp64 model (tests/fd_model.py, forward_heads), per ENTRY of every
parameter tensor: |analytic - fd| <= 1e-3 |fd| + 1e-5 max|fd| (test_fd_gradcheck._assert_entrywise), on scenes of 8 Gaussians kept
away from the skip, stop and 0.99-clamp discontinuities, on a 37 x 27 image (partial tiles on both axes).

CPU: the oracle's four-pass chain (render_rgb_bwd + 3 x render_scalar_bwd + project_bwd with the folded depth gradient -- the
composition the oracle tests rely on), and the batched C-ABI pair on the emulator in both backward forms (plain and moments) with the
in-launch densify statistics (tests/heads_chain.py).  GPU (-m gpu): BatchRenderer.render_heads through the C++ node and the Python
Functions, with raw parameters, the statistics, the per-camera path, the C-ABI pair, plain against moments on a mid-size scene, and the
parameter activations at their edges."""
import os
import subprocess

import numpy as np
import pytest
import torch

import fd_model as FD
import heads_chain
import scenes
from oracle import oracle as O
from test_fd_gradcheck import _assert_entrywise

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
KEYS = ("mean", "qvec", "svec", "alpha", "color")
W, H = 37, 27  # 3 x 2 tiles, the last column and row partial


def _cams(B, seed=0):
    return [scenes.Camera(W, H, fx=600.0 + 70 * i, c2w=scenes.orbit(2.5, 15.0 + 7 * seed + 25 * i, 40.0 + 50 * seed + 80 * i))
            for i in range(B)]


def _gos(B, seed):
    rng = np.random.default_rng(200 + seed)
    return [(rng.normal(size=(H, W, 3)), rng.normal(size=(H, W)), rng.normal(size=(H, W)), rng.normal(size=(H, W)))
            for _ in range(B)]


def _logit(x):
    return np.log(x / (1 - x))


def _scene(seed, cams, raw=False):
    """-> (post-activation scene [fp32], fp64 FD parameters: raw fields under exp / sigmoid / sigmoid when raw)"""
    sc = FD.tiny_scene(8, seed, 0, cams[0])
    P = {k: np.asarray(sc[k], np.float64) for k in KEYS}
    if raw:
        rawf = {"svec": np.log(sc["svec"]), "alpha": _logit(sc["alpha"].astype(np.float64)), "color": _logit(sc["color"].astype(np.float64))}
        for k, v in rawf.items():
            P[k] = v.astype(np.float32).astype(np.float64)
        act = FD.ACTIVATIONS
        sc["svec"], sc["alpha"], sc["color"] = (act[a](P[k]).astype(np.float32) for a, k in
                                                 (("exp", "svec"), ("sigmoid", "alpha"), ("sigmoid", "color")))
    return sc, P


def _fd_heads(sc, P, cams, gos, bg, detach, z_var, act=None, dm2=False):
    """-> (images per view, summed FD gradients of KEYS + bg, per-view FD d L / d mean2d when dm2)"""
    P = dict(P, bg=np.asarray(bg, np.float64))
    names = KEYS + ("bg",)
    want = {k: 0.0 for k in names}
    imgs, m2 = [], []
    for cam, go in zip(cams, gos):
        g = scenes.oracle_geometry(sc, cam)
        assert g["mask"].all() and g["D"] >= len(sc["mean"])  # every Gaussian is visible and lands in a tile list
        kw = dict(heads=dict(zip(FD.HEADS, go[1:])), z_var=z_var, act=act)
        _, img, frozen = FD.forward_heads(P, cam, 0, go[0], None, 1e-4, detach, None, (g["start"], g["end"], g["ids"]), **kw)
        # the same decisions in fp32 as in fp64 (test_fd_gradcheck._fd), and well away from the 0.99 clamp
        assert frozen.margins["skip"] > 1e-5 and frozen.margins["stop"] > 0.5 and frozen.margins["clamp"] > 1e-2, frozen.margins
        fd = FD.fd_gradients(P, cam, 0, go[0], frozen, names, detach_depth=detach, **kw)
        want = {k: want[k] + fd[k] for k in names}
        imgs.append(img)
        if dm2:
            Q = dict(P, dm2=np.zeros((len(sc["mean"]), 2)))
            m2.append(FD.fd_gradients(Q, cam, 0, go[0], frozen, ("dm2",), detach_depth=detach, **kw)["dm2"])
    return imgs, want, m2


def _assert_images(got, want, tol=1e-5):
    for k in ("rgb", "depth", "opacity", "depth2"):
        a, b = np.asarray(got[k], np.float64).reshape(want[k].shape), want[k]
        assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()), (k, float(np.abs(a - b).max()))


# ---- CPU: the oracle's four-pass chain ---------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,detach,z_var", [(0, False, True), (1, True, True), (2, True, False)])
def test_oracle_heads_chain_against_finite_differences(seed, detach, z_var):
    """render_rgb_bwd (final = rgb + T bg) + render_scalar_bwd for depth, opacity, depth^2 + project_bwd with
    g_depth = ss_depth + 2 depth ss_depth2 -- z_var's chain rule d/d depth -= 2 depth g_zvar by hand, d bg = sum g_rgb T"""
    cams = _cams(1, seed)
    cam = cams[0]
    sc, P = _scene(seed, cams)
    gos = _gos(1, seed)
    bg = np.array([0.3, 0.6, 0.15], np.float32)
    (img,), want, _ = _fd_heads(sc, P, cams, gos, bg, detach, z_var)
    g_rgb, g_d, g_o, g_z = (np.asarray(x, np.float32) for x in gos[0])
    g = scenes.oracle_geometry(sc, cam)
    geo = (g["start"], g["end"], g["ids"], cam.topleft, 1 / cam.fx, 1 / cam.fy, H, W)
    dv = np.ascontiguousarray(g["depth"].ravel())
    o_rgb, o_T = O.render_rgb_fwd(g["mean2d"], g["cov2d"], sc["color"], sc["alpha"], *geo)
    final = (o_rgb + o_T.reshape(H, W, 1) * bg).astype(np.float32)
    vals = (dv, np.ones_like(dv), dv * dv)
    outs = [O.render_scalar_fwd(g["mean2d"], g["cov2d"], v, sc["alpha"], *geo)[0] for v in vals]
    z2img = outs[2] - outs[0] * outs[0] if z_var else outs[2]
    _assert_images(dict(rgb=final, depth=outs[0], opacity=outs[1], depth2=z2img), img)
    r = O.render_rgb_bwd(g["mean2d"], g["cov2d"], sc["color"], sc["alpha"], g["start"], g["end"], g["ids"], final, g_rgb, *geo[3:])
    sgo = (g_d - 2.0 * outs[0] * g_z if z_var else g_d, g_o, g_z)
    ss = [O.render_scalar_bwd(g["mean2d"], g["cov2d"], v, sc["alpha"], g["start"], g["end"], g["ids"], o_,
                              np.ascontiguousarray(s_, np.float32), *geo[3:]) for v, o_, s_ in zip(vals, outs, sgo)]
    gm2 = r[0] + sum(x[0] for x in ss); gc2 = r[1] + sum(x[1] for x in ss); ga = r[3] + sum(x[3] for x in ss)
    gdepth = ss[0][2] + 2.0 * dv * ss[2][2]
    gm, gq, gs = O.project_bwd(sc["mean"], sc["qvec"], sc["svec"], cam.c2w, gm2, gc2, gdepth.reshape(-1, 1), detach)
    gbg = (g_rgb.astype(np.float64) * o_T.reshape(H, W, 1)).sum((0, 1))
    _assert_entrywise({"mean": gm, "qvec": gq, "svec": gs, "alpha": ga, "color": r[2], "bg": gbg}, want, ("oracle heads", seed, detach))


# ---- the batched C-ABI pair: emulator and device ---------------------------------------------------------------------------
def _check_pair(L, form, detach, seed=3, sync=lambda: None):
    """two views, background, z_var, statistics: every gradient, d L / d mean2d per view, grad_accum and cnt against the FD model"""
    cams = _cams(2, seed)
    sc, P = _scene(seed, cams)
    gos = _gos(2, seed)
    bg = np.array([0.25, 0.5, 0.7], np.float32)
    imgs, want, m2 = _fd_heads(sc, P, cams, gos, bg, detach, True, dm2=True)
    res = heads_chain.batched_heads(L, sc, cams, gos, bg, form, detach, True, sync=sync)
    for got, img in zip(res["images"], imgs):
        _assert_images(got, img)
        assert np.abs(got["T"] - img["T"]).max() <= 1e-5
    _assert_entrywise(res["grads"], want, ("C ABI", form, detach))
    for v, fd in enumerate(m2):
        _assert_entrywise({"gm2d": res["gm2d"][v]}, {"gm2d": fd}, ("d mean2d", form, v))
    norms = sum(np.linalg.norm(x, axis=1) for x in m2)
    _assert_entrywise({"grad_accum": res["grad_accum"]}, {"grad_accum": norms}, ("grad_accum", form))
    assert np.array_equal(res["cnt"], np.full(len(sc["mean"]), 2.0, np.float32)), res["cnt"]


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "emu"])
    from gsgen_amd import _capi
    return _capi.Lib(os.path.join(ROOT, "oracle", "_build", "libgsgen_emu.so"))


class _HostArrays:
    """the emulator works on host memory: "device" arrays are numpy arrays"""

    class Arr:
        def __init__(self, a):
            self.a = np.ascontiguousarray(a).copy(); self.p = self.a.ctypes.data; self.n = self.a.size

        def get(self):
            return self.a

    def __init__(self, lib):
        self.lib, self.stream = lib, None

    def to_dev(self, a):
        return self.Arr(a)


@pytest.mark.parametrize("form,detach", [("plain", False), ("moments", False), ("moments", True)])
def test_emulated_batched_heads_pair_against_finite_differences(emu, form, detach):
    _check_pair(_HostArrays(emu), form, detach)


# ---- the HIP path ------------------------------------------------------------------------------------------------------------
def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda:0")


class _DeviceArrays:
    """heads_chain on the GPU: arrays are torch tensors on the device"""

    class Arr:
        def __init__(self, a):
            self.t = torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0"); self.p = self.t.data_ptr(); self.n = self.t.numel()

        def get(self):
            return self.t.cpu().numpy()

    def __init__(self):
        from gsgen_amd import _capi
        self.lib, self.stream = _capi.load(), torch.cuda.current_stream().cuda_stream

    def to_dev(self, a):
        return self.Arr(a)


@pytest.mark.gpu
@pytest.mark.parametrize("form,detach", [("plain", False), ("moments", False), ("moments", True)])
def test_hip_batched_heads_pair_against_finite_differences(form, detach):
    """what the emulator test above runs, on the device"""
    _check_pair(_DeviceArrays(), form, detach, sync=torch.cuda.synchronize)


@pytest.mark.gpu
@pytest.mark.parametrize("B,detach,z_var,use_ext,raw", [(1, False, False, True, False), (2, False, True, True, False),
                                                        (2, True, True, True, False), (2, True, False, False, False),
                                                        (1, True, True, False, False), (2, False, True, True, True),
                                                        (2, True, True, False, True)])
def test_hip_render_heads_against_finite_differences(B, detach, z_var, use_ext, raw):
    """BatchRenderer.render_heads (the moment form) through the C++ node (use_ext) or the Python Function, a trainable background,
    raw parameters under ("exp", "sigmoid", "sigmoid") when raw: the gradients of mean, qvec, svec, alpha, colour and bg; the densify
    statistics against the FD norm of d L / d mean2d per view and the visit count"""
    from gsgen_amd import renderer as R
    from gsgen_amd.batch import BatchRenderer
    seed = 4 + B + 2 * int(detach) + int(raw)
    cams = _cams(B, seed)
    sc, P64 = _scene(seed, cams, raw=raw)
    act = ("exp", "sigmoid", "sigmoid") if raw else None
    gos = _gos(B, seed)
    bg0 = np.array([0.35, 0.2, 0.65], np.float32)
    imgs, want, m2 = _fd_heads(sc, P64, cams, gos, bg0, detach, z_var, act=act, dm2=True)
    n = len(sc["mean"])
    P = {k: _T(P64[k]).requires_grad_(True) for k in KEYS}
    bg = _T(bg0).requires_grad_(True)
    stats = R.DensifyStats(n, torch.device("cuda:0"))
    br = BatchRenderer(n, W, H, torch.device("cuda:0"), max_batch=B)
    br.use_ext = use_ext
    cis, c2ws = [R.CameraInfo(*c.intr) for c in cams], [c.c2w for c in cams]
    run = lambda: br.render_heads(P["mean"], P["qvec"], P["svec"], P["alpha"], P["color"], cis, c2ws, bg_rgb=bg,  # noqa: E731
                                  detach_depth=detach, stats=stats, z_var=z_var, activations=act)
    with torch.no_grad():
        run()  # (sizes the pair lists: the C++ node takes the batches after the first)
    assert br.ensure_capacity(B)
    outs = run()
    assert ("HeadsFn" in outs[0].grad_fn.name()) == use_ext, outs[0].grad_fn.name()  # which autograd node rendered it
    gos_t = [_T(np.stack([go[k] for go in gos])) for k in range(4)]
    (sum((o.reshape(x.shape) * x).sum() for o, x in zip(outs[:4], gos_t))).backward()
    torch.cuda.synchronize()
    for i, img in enumerate(imgs):
        _assert_images({k: o[i].detach().cpu().numpy() for k, o in zip(("rgb", "depth", "opacity", "depth2"), outs)}, img)
    got = {k: P[k].grad.cpu().numpy() for k in KEYS}
    got["bg"] = bg.grad.cpu().numpy()
    _assert_entrywise(got, want, ("render_heads", B, detach, z_var, use_ext, raw))
    norms = sum(np.linalg.norm(x, axis=1) for x in m2)
    _assert_entrywise({"grad_accum": stats.grad_accum.cpu().numpy()}, {"grad_accum": norms}, "grad_accum")
    assert np.array_equal(stats.cnt.cpu().numpy(), np.full(n, float(B), np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("seed,detach,z_var", [(5, False, True), (6, True, False)])
def test_hip_per_camera_rgb_heads_against_finite_differences(seed, detach, z_var):
    """the per-camera plain path: renderer.project_gaussians -> the frame's lists -> renderer.render_rgb_heads
    (gsgen_vol_render_rgbd_backward per pixel), z_var formed in torch, d L / d mean2d through mean2d.grad"""
    from gsgen_amd import renderer as R
    cams = _cams(1, seed)
    cam = cams[0]
    sc, P64 = _scene(seed, cams)
    gos = _gos(1, seed)
    bg0 = np.array([0.1, 0.45, 0.8], np.float32)
    (img,), want, (m2,) = _fd_heads(sc, P64, cams, gos, bg0, detach, z_var, dm2=True)
    g = scenes.oracle_geometry(sc, cam)
    P = {k: _T(P64[k]).requires_grad_(True) for k in KEYS}
    bg = _T(bg0).requires_grad_(True)
    mean2d, cov2d, _, depth = R.project_gaussians(P["mean"], P["qvec"], P["svec"], _T(cam.c2w), detach)
    mean2d.retain_grad()
    assert np.abs(mean2d.detach().cpu().numpy() - g["mean2d"]).max() <= 1e-6 * np.abs(g["mean2d"]).max()
    nth, ntw = cam.tiles
    ids = torch.from_numpy(g["ids"]).to("cuda:0")
    rgb, dimg, opac, z2, T = R.render_rgb_heads(mean2d, cov2d, P["color"], depth, P["alpha"], torch.from_numpy(g["start"]).to("cuda:0"),
                                                torch.from_numpy(g["end"]).to("cuda:0"), ids, _T(cam.topleft), nth, ntw, 1 / cam.fx,
                                                1 / cam.fy, H, W, 1e-4, bg)
    zz = z2 - dimg * dimg if z_var else z2
    go = [_T(x) for x in gos[0]]
    ((rgb * go[0]).sum() + (dimg[..., 0] * go[1]).sum() + (opac[..., 0] * go[2]).sum() + (zz[..., 0] * go[3]).sum()).backward()
    _assert_images({"rgb": rgb.detach().cpu().numpy(), "depth": dimg[..., 0].detach().cpu().numpy(),
                    "opacity": opac[..., 0].detach().cpu().numpy(), "depth2": zz[..., 0].detach().cpu().numpy()}, img)
    got = {k: P[k].grad.cpu().numpy() for k in KEYS}
    got["bg"] = bg.grad.cpu().numpy()
    _assert_entrywise(got, want, ("per camera", seed, detach, z_var))
    _assert_entrywise({"gm2d": mean2d.grad.cpu().numpy()}, {"gm2d": m2}, "per camera d mean2d")


@pytest.mark.gpu
def test_hip_heads_moment_form_equals_the_plain_form():
    """plain against moments on the device, one mid-size scene (3 000 Gaussians, 3 cameras of 101 x 75): every gradient row within
    1e-4 of its own largest entry + 1e-6 of the tensor's largest (scenes.per_gaussian_grad_error), d L / d mean2d per view and the
    statistics alike, cnt exactly"""
    sc = scenes.random_scene(3000, seed=17, svec=0.04)
    Wm, Hm = 101, 75
    cams = [scenes.Camera(Wm, Hm, fx=95.0 + 10 * i, c2w=scenes.orbit(2.4 + 0.1 * i, 10 + 15 * i, 30.0 + 110 * i)) for i in range(3)]
    rng = np.random.default_rng(8)
    gos = [(rng.normal(size=(Hm, Wm, 3)), rng.normal(size=(Hm, Wm)), rng.normal(size=(Hm, Wm)), rng.normal(size=(Hm, Wm)))
           for _ in cams]
    bg = np.array([0.2, 0.3, 0.9], np.float32)
    L = _DeviceArrays()
    res = {f: heads_chain.batched_heads(L, sc, cams, gos, bg, f, False, True, sync=torch.cuda.synchronize) for f in ("plain", "moments")}
    a, b = res["plain"], res["moments"]
    report = {}
    for k in KEYS:
        assert np.abs(a["grads"][k]).max() > 0, k
        report[k] = scenes.per_gaussian_grad_error(b["grads"][k], a["grads"][k], rtol=1e-4, atol=1e-6)
    for v in range(len(cams)):
        report[f"gm2d{v}"] = scenes.per_gaussian_grad_error(b["gm2d"][v], a["gm2d"][v], rtol=1e-4, atol=1e-6)
    report["grad_accum"] = scenes.per_gaussian_grad_error(b["grad_accum"], a["grad_accum"], rtol=1e-4, atol=1e-6)
    print("plain vs moments, per-row error in units of the tolerance (worst row):", report)
    assert all(r <= 1.0 for r, _ in report.values()), report
    assert np.abs(a["grads"]["bg"] - b["grads"]["bg"]).max() <= 1e-5 * np.abs(a["grads"]["bg"]).max()
    assert np.array_equal(a["cnt"], b["cnt"]) and a["cnt"].max() == 3


# the edges of the activations: (code name, raw values); fp64 torch is the accuracy reference, fp32 torch decides inf, 0 and the
# subgradients.  Budget: 4 fp32 ulps of the fp64 value (relative 4 x 2^-23; the GPU's expf / log1pf are within 1-2 ulps, the sigmoid's
# 1 / (1 + e) adds two roundings) plus 1e-37 absolute where the result is sub-normal and the device flushes it to zero.
_EDGE = np.array([-100.0, -88.8, -88.7, -30.0, -20.5, -20.0, -19.5, -1.0, -1e-7, 0.0, 1e-7, 1.0, 19.5, 20.0, 20.0001, 20.5, 30.0,
                  88.7, 88.72, 88.8, 100.0], np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["nothing", "exp", "sigmoid", "abs", "relu", "softplus", "biased_relu", "biased_abs"])
def test_hip_activations_at_their_edges(name):
    from gsgen_amd import _capi
    from gsgen_amd.batch import ACTIVATION_CODES, TORCH_ACTIVATIONS
    lib = _capi.load()
    x = np.concatenate([_EDGE, -_EDGE[::-1]])  # (-0.0 as well)
    raw = [np.ascontiguousarray(np.stack([x, x[::-1], x], 1)), x.copy(), np.ascontiguousarray(np.stack([x[::-1], x, x[::-1]], 1))]
    N = x.size
    code = ACTIVATION_CODES[name]
    d = [_T(r) for r in raw]
    out = [torch.full_like(t, 7.0) for t in d]
    lib.activate_fields(N, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), code, code, code, *(t.data_ptr() for t in out),
                        torch.cuda.current_stream().cuda_stream)
    gin = [np.random.default_rng(i).normal(size=r.shape).astype(np.float32) for i, r in enumerate(raw)]
    g = [_T(x_) for x_ in gin]
    lib.activate_fields_backward(N, *(t.data_ptr() for t in d), *(t.data_ptr() for t in out), code, code, code,
                                 *(t.data_ptr() for t in g), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    f = TORCH_ACTIVATIONS[name]
    ulp4 = 4 * 2.0 ** -23
    for r, o, gi, go in zip(raw, out, gin, g):
        o, go = o.cpu().numpy().astype(np.float64), go.cpu().numpy().astype(np.float64)
        x32 = torch.tensor(r, requires_grad=True)
        y32 = f(x32)
        y32.backward(torch.tensor(gi))
        x64 = torch.tensor(r.astype(np.float64), requires_grad=True)
        y64 = f(x64)
        y64.backward(torch.tensor(gi.astype(np.float64)))
        for what, got, w32, w64 in (("value", o, y32.detach().numpy(), y64.detach().numpy()),
                                    ("gradient", go, x32.grad.numpy(), x64.grad.numpy())):
            assert not np.isnan(got).any(), (name, what, r[np.isnan(got)])
            inf32 = np.isinf(w32)
            assert np.array_equal(np.isinf(got), inf32), (name, what, r[np.isinf(got) != inf32])
            assert np.array_equal(got[inf32], w32[inf32].astype(np.float64)), (name, what)
            zero32 = (w32 == 0) & ~inf32  # (0, or a sub-normal the device flushes: the subgradients at 0 among them)
            assert (np.abs(got[zero32]) <= 1e-37).all(), (name, what, r[zero32], got[zero32])
            fin = ~inf32 & ~zero32
            err = np.abs(got[fin] - w64[fin])
            assert (err <= ulp4 * np.abs(w64[fin]) + 1e-37).all(), (name, what, r[fin][err > ulp4 * np.abs(w64[fin]) + 1e-37],
                                                                   got[fin][err > ulp4 * np.abs(w64[fin]) + 1e-37])
