"""gsgen_amd/csrc/background.hip on the CPU SIMT emulator (oracle/emu) against the torch restatement of tests/background_cases.py, and
the argument checks of gsgen_amd.background that need no GPU.  The file is compiled without contraction and carries its own stand-in
for the fp32 MFMA (four products per output gathered with __shfl, chained with fmaf in k order), so the emulated kernels perform the
GPU's operations in the GPU's order; only expf differs (libm here, the device library there)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import background_cases as BC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSGEN_EUNSUPPORTED, GSGEN_EINVAL, GSGEN_EWORKSPACE = -2, -3, -4


@pytest.fixture(scope="module")
def bg_emu(tmp_path_factory):
    """background.hip compiled with g++ on the emulator headers, with the flags tests/test_depth_loss_host.py uses (into tmp: nothing
    under oracle/ changes)"""
    out = tmp_path_factory.mktemp("background_emu") / "libbackground_emu.so"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                           "-Wno-unknown-pragmas", "-DGSGEN_EMU_KNOBS=1", "-I", os.path.join(ROOT, "oracle", "emu"), "-x", "c++",
                           os.path.join(ROOT, "gsgen_amd", "csrc", "background.hip"), "-o", str(out), "-lm"])
    lib = C.CDLL(str(out))
    u32, vp, i32, sz = C.c_uint32, C.c_void_p, C.c_int, C.c_size_t
    lib.gsgen_mlp_background_workspace_bytes.argtypes = [u32, u32, u32]
    lib.gsgen_mlp_background_workspace_bytes.restype = sz
    lib.gsgen_mlp_background_forward.argtypes = [vp, vp, sz, vp, u32, u32, u32, vp, vp, vp, vp]
    lib.gsgen_mlp_background_forward.restype = i32
    lib.gsgen_mlp_background_backward.argtypes = [vp, vp, sz, vp, u32, u32, u32, vp, vp, vp, vp, vp, sz, vp]
    lib.gsgen_mlp_background_backward.restype = i32
    lib.gsgen_mlp_background_emu_constants.argtypes = [vp]
    return lib


def ptr(a):
    return None if a is None else a.ctypes.data


def f32(t):
    return np.ascontiguousarray(t.numpy() if isinstance(t, torch.Tensor) else t, np.float32)


def run(lib, params, shape, cams=None, stride=0, dirs=None, rgb=None, opacity=None, grad=None, want_opacity=True):
    """-> (out [B,H,W,3], grad_params [768] or None, grad_opacity [B,H,W,1] or None); the backward only with `grad`.  The workspace
    starts dirty and unaligned, the outputs start as NaN."""
    B, H, W = shape
    out = np.full((B, H, W, 3), np.nan, np.float32)
    rc = lib.gsgen_mlp_background_forward(ptr(params), ptr(cams), stride, ptr(dirs), B, H, W, ptr(rgb), ptr(opacity), ptr(out), None)
    assert rc == 0, rc
    if grad is None:
        return out, None, None
    nbytes = lib.gsgen_mlp_background_workspace_bytes(B, H, W)
    assert nbytes > 0
    wsb = np.full(nbytes + 3, 0xA5, np.uint8)[3:]  # (an unaligned, dirty base: the kernels align it and assume nothing zero)
    gp = np.full(BC.N_PARAMS, np.nan, np.float32)
    go = np.full((B, H, W, 1), np.nan, np.float32) if (opacity is not None and want_opacity) else None
    rc = lib.gsgen_mlp_background_backward(ptr(params), ptr(cams), stride, ptr(dirs), B, H, W, ptr(opacity), ptr(grad), ptr(gp), ptr(go),
                                           ptr(wsb), wsb.size, None)
    assert rc == 0, rc
    return out, gp, go


def arrays(name, stride_floats=16):
    c = BC.case(name)
    return c, dict(params=f32(c["params"]), cams=f32(BC.cam_blocks(c, stride_floats)), stride=4 * stride_floats, rgb=f32(c["rgb"]),
                   opacity=f32(c["opacity"]), grad=f32(c["grad"]))


def test_the_constants_the_cases_assume(bg_emu):
    k = np.zeros(4, np.uint32)
    bg_emu.gsgen_mlp_background_emu_constants(k.ctypes.data)
    threads, min_iters, max_groups, slices = (int(v) for v in k)
    run_len = threads * min_iters
    groups = {n: -(-int(np.prod(BC.CASES[n][0])) // run_len) for n in BC.NAMES}
    assert groups["one-1x16x16"] == 1 and 16 * 16 < run_len                      # one partial workgroup
    assert (2 * 37 * 53) % 64 != 0 and (37 * 53) % run_len != 0                  # tail lanes; a run crosses the views
    assert 64 * 64 // run_len > 1                                                # several workgroups per view
    assert slices < groups["passes-1x160x200"] <= max_groups                     # more than one pass of the final reduction


@pytest.mark.parametrize("name", BC.NAMES)
def test_emulated_background_meets_the_restatements_own_error(bg_emu, name):
    c, a = arrays(name, stride_floats=68)  # (the renderer's row stride)
    shape = c["shape"]
    # the plain form: the image and its parameter gradient
    bg, gp, none = run(bg_emu, a["params"], shape, a["cams"], a["stride"], grad=a["grad"])
    assert none is None
    BC.check(name, "bg", bg)
    BC.check(name, "gp_plain", gp)
    # the composite form
    out, gpo, go = run(bg_emu, a["params"], shape, a["cams"], a["stride"], rgb=a["rgb"], opacity=a["opacity"], grad=a["grad"])
    BC.check(name, "out", out)
    BC.check(name, "gp_over", gpo)
    BC.check(name, "g_opacity", go)
    # the gradient of W2's padding rows is exactly zero, not merely small
    for g in (gp, gpo):
        assert not g[512 + 3 * 16:].any() and g[:512 + 3 * 16].any()


@pytest.mark.parametrize("name", ["one-1x16x16", "tail-2x37x53"])
def test_explicit_directions_agree_with_the_camera_form(bg_emu, name):
    """bg(rays_d) on the fp32 restatement's rays: within the bound of the truth, as the camera form is; another row stride of the
    camera blocks changes no bit"""
    c, a = arrays(name)
    shape = c["shape"]
    dirs = f32(c["r32"]["dirs"])
    bg_d, gp_d, _ = run(bg_emu, a["params"], shape, dirs=dirs, grad=a["grad"])
    BC.check(name, "bg", bg_d)
    BC.check(name, "gp_plain", gp_d)
    out_d, gpo_d, go_d = run(bg_emu, a["params"], shape, dirs=dirs, rgb=a["rgb"], opacity=a["opacity"], grad=a["grad"])
    BC.check(name, "out", out_d)
    BC.check(name, "gp_over", gpo_d)
    BC.check(name, "g_opacity", go_d)
    if name == "one-1x16x16":
        bg16, gp16, _ = run(bg_emu, a["params"], shape, a["cams"], a["stride"], grad=a["grad"])
        _, a68 = arrays(name, stride_floats=68)
        bg68, gp68, _ = run(bg_emu, a["params"], shape, a68["cams"], a68["stride"], grad=a["grad"])
        assert bg16.tobytes() == bg68.tobytes() and gp16.tobytes() == gp68.tobytes()


def test_bit_identical_from_run_to_run_and_linear_in_the_upstream_gradient(bg_emu):
    name = "tail-2x37x53"
    c, a = arrays(name)
    kw = dict(rgb=a["rgb"], opacity=a["opacity"])
    o0, p0, g0 = run(bg_emu, a["params"], c["shape"], a["cams"], a["stride"], grad=a["grad"], **kw)
    o1, p1, g1 = run(bg_emu, a["params"], c["shape"], a["cams"], a["stride"], grad=a["grad"], **kw)
    assert o0.tobytes() == o1.tobytes() and p0.tobytes() == p1.tobytes() and g0.tobytes() == g1.tobytes()
    _, p2, g2 = run(bg_emu, a["params"], c["shape"], a["cams"], a["stride"], grad=2.0 * a["grad"], **kw)
    assert p2.tobytes() == (2.0 * p0).astype(np.float32).tobytes() and g2.tobytes() == (2.0 * g0).astype(np.float32).tobytes()
    # grad_opacity is optional, and asking for it changes nothing else
    o3, p3, none = run(bg_emu, a["params"], c["shape"], a["cams"], a["stride"], grad=a["grad"], want_opacity=False, **kw)
    assert none is None and o3.tobytes() == o0.tobytes() and p3.tobytes() == p0.tobytes()


def test_a_pixel_with_a_non_finite_output_is_black_and_takes_no_gradient(bg_emu):
    """explicit directions: one pixel's direction is NaN, one is +Inf; every other pixel is unchanged and so is the gradient they sum to"""
    name = "one-1x16x16"
    c, a = arrays(name)
    shape = c["shape"]
    dirs = f32(c["r32"]["dirs"]).copy()
    bad = [(0, 3, 5), (0, 9, 0)]
    good_grad = a["grad"].copy()
    for b in bad:
        good_grad[b] = 0.0
    # the truth: the same pixels with a zero upstream gradient, at finite directions
    out_ref, gp_ref, go_ref = run(bg_emu, a["params"], shape, dirs=dirs, rgb=a["rgb"], opacity=a["opacity"], grad=good_grad)
    dirs[bad[0]] = np.nan
    dirs[bad[1]] = np.inf
    out, gp, go = run(bg_emu, a["params"], shape, dirs=dirs, rgb=a["rgb"], opacity=a["opacity"], grad=a["grad"])
    assert np.isfinite(out).all() and np.isfinite(gp).all() and np.isfinite(go).all()
    for b in bad:
        assert out[b].tobytes() == a["rgb"][b].tobytes() and go[b] == 0.0  # bg = 0: the composite leaves rgb, opacity gets nothing
        out[b], out_ref[b], go[b], go_ref[b] = 0.0, 0.0, 0.0, 0.0
    assert out.tobytes() == out_ref.tobytes() and go.tobytes() == go_ref.tobytes() and gp.tobytes() == gp_ref.tobytes()
    # NaN parameters: a black image, zero gradients
    nan_params = np.full(BC.N_PARAMS, np.nan, np.float32)
    img, gpn, _ = run(bg_emu, nan_params, shape, a["cams"], a["stride"], grad=a["grad"])
    assert not img.any() and not gpn.any()


def test_emulated_background_argument_checks(bg_emu):
    lib = bg_emu
    B, H, W = 2, 5, 7
    rng = np.random.default_rng(0)
    params = rng.random(BC.N_PARAMS).astype(np.float32)
    cams = rng.random((B, 16)).astype(np.float32) + 1.0
    dirs = rng.random((B, H, W, 3)).astype(np.float32)
    rgb, op, g = dirs.copy(), rng.random((B, H, W)).astype(np.float32), dirs.copy()
    out, gp, go = np.full((B, H, W, 3), 7.0, np.float32), np.full(BC.N_PARAMS, 7.0, np.float32), np.full((B, H, W), 7.0, np.float32)
    wsb = np.zeros(1 << 16, np.uint8)

    def fwd(B=B, H=H, params=params, cams=cams, stride=64, dirs=None, rgb=rgb, op=op, out=out):
        return lib.gsgen_mlp_background_forward(ptr(params), ptr(cams), stride, ptr(dirs), B, H, W, ptr(rgb), ptr(op), ptr(out), None)

    def bwd(B=B, H=H, params=params, cams=cams, stride=64, dirs=None, op=op, g=g, gp=gp, go=go, ws=wsb, nbytes=wsb.size):
        return lib.gsgen_mlp_background_backward(ptr(params), ptr(cams), stride, ptr(dirs), B, H, W, ptr(op), ptr(g), ptr(gp), ptr(go), ptr(ws),
                                                 nbytes, None)
    for call in (fwd, bwd):
        assert call(B=0) == 0 and call(H=0) == 0                      # empty: clean, nothing written
        assert call(B=70000, H=70000) == GSGEN_EUNSUPPORTED           # more than 2^31 pixels
        assert call(params=None) == GSGEN_EINVAL
        assert call(cams=None) == GSGEN_EINVAL                        # no source of directions
        assert call(dirs=dirs) == GSGEN_EINVAL                        # two of them
        assert call(stride=62) == GSGEN_EINVAL and call(stride=32) == GSGEN_EINVAL
    assert fwd(out=None) == GSGEN_EINVAL
    assert fwd(rgb=None) == GSGEN_EINVAL and fwd(op=None) == GSGEN_EINVAL       # rgb_in and opacity: both or neither
    assert bwd(g=None) == GSGEN_EINVAL and bwd(gp=None) == GSGEN_EINVAL and bwd(ws=None) == GSGEN_EINVAL
    assert bwd(op=None) == GSGEN_EINVAL                                        # grad_opacity without opacity
    assert lib.gsgen_mlp_background_workspace_bytes(70000, 70000, W) == 0 and lib.gsgen_mlp_background_workspace_bytes(0, H, W) == 0
    need = lib.gsgen_mlp_background_workspace_bytes(B, H, W)
    assert 0 < need <= wsb.size
    assert need < lib.gsgen_mlp_background_workspace_bytes(B, 64, 64) < lib.gsgen_mlp_background_workspace_bytes(2 * B, 64, 64)
    assert lib.gsgen_mlp_background_workspace_bytes(8, 800, 800) <= 768 * 4 * 1024 + 512   # at most 1024 partials
    assert bwd(nbytes=need - 1) == GSGEN_EWORKSPACE
    assert (out == 7.0).all() and (gp == 7.0).all() and (go == 7.0).all() and not wsb.any()  # a refused call enqueues nothing
    assert fwd() == 0 and bwd(nbytes=need) == 0
    assert np.isfinite(out).all() and np.isfinite(gp).all() and np.isfinite(go).all() and (go != 7.0).all()
    assert fwd(cams=None, dirs=dirs) == 0 and bwd(cams=None, dirs=dirs) == 0 and fwd(rgb=None, op=None) == 0
    assert bwd(op=None, go=None) == 0 and bwd(go=None) == 0


# --- gsgen_amd.background: the refusals, which need neither a GPU nor the library -------------------------------------------
def test_python_refusals():
    """every check comes before the device check, so CPU tensors reach each of them; a well-formed CPU call is refused last"""
    from gsgen_amd import background as GB
    d = lambda *s, **k: torch.rand(*s, **k)  # noqa: E731
    p, cams = d(768), d(2, 16)
    for call in (lambda: GB.mlp_background(p, d(8, 9, 3)), lambda: GB.mlp_background_images(p, cams, 8, 9),
                 lambda: GB.mlp_background_over(p, d(2, 8, 9, 3), d(2, 8, 9, 1), cams),
                 lambda: GB.mlp_background_over(p, d(2, 8, 9, 3), d(2, 8, 9), d(4, 68)[:2])):
        with pytest.raises(ValueError, match="no CPU implementation"):
            call()
    with pytest.raises(ValueError, match=r"\[768\]"):
        GB.mlp_background(d(767), d(8, 9, 3))
    with pytest.raises(ValueError, match=r"\[768\]"):
        GB.mlp_background_images(d(16, 48), cams, 8, 9)
    with pytest.raises(ValueError, match=r"\[\.\.\., 3\]"):
        GB.mlp_background(p, d(8, 9, 4))
    with pytest.raises(ValueError, match="camera blocks"):
        GB.mlp_background_images(p, d(2, 12), 8, 9)
    with pytest.raises(ValueError, match="camera blocks"):
        GB.mlp_background_images(p, d(16), 8, 9)
    with pytest.raises(ValueError, match="contiguous rows"):
        GB.mlp_background_images(p, d(32, 2).t(), 8, 9)
    with pytest.raises(ValueError, match=r"\[B, H, W, 3\]"):
        GB.mlp_background_over(p, d(8, 9, 3), d(8, 9, 1), cams)
    with pytest.raises(ValueError, match="opacity must be"):
        GB.mlp_background_over(p, d(2, 8, 9, 3), d(2, 9, 8, 1), cams)
    with pytest.raises(ValueError, match="opacity must be"):
        GB.mlp_background_over(p, d(2, 8, 9, 3), d(2, 8, 9, 3), cams)
    with pytest.raises(ValueError, match="3 camera blocks for a batch of 2"):
        GB.mlp_background_over(p, d(2, 8, 9, 3), d(2, 8, 9, 1), d(3, 16))
    with pytest.raises(ValueError, match="empty"):
        GB.mlp_background(p, d(0, 9, 3))
    with pytest.raises(ValueError, match="empty"):
        GB.mlp_background_images(p, cams, 0, 9)
    with pytest.raises(ValueError, match="empty"):
        GB.mlp_background_over(p, d(0, 8, 9, 3), d(0, 8, 9, 1), d(0, 16))
    with pytest.raises(NotImplementedError, match="float32"):
        GB.mlp_background(p.double(), d(8, 9, 3))
    with pytest.raises(NotImplementedError, match="float32"):
        GB.mlp_background_over(p, d(2, 8, 9, 3), d(2, 8, 9, 1).half(), cams)
    with pytest.raises(NotImplementedError, match="requires a gradient"):
        GB.mlp_background(p, d(8, 9, 3, requires_grad=True))
    with pytest.raises(NotImplementedError, match="random_aug"):
        GB.MLPBackground({"type": "mlp", "random_aug": True})


def test_module_parameters_initialisation_and_state_dict():
    from gsgen_amd import background as GB
    torch.manual_seed(11)
    a = GB.MLPBackground({"type": "mlp"})
    torch.manual_seed(11)
    b = GB.MLPBackground({"type": "mlp"})
    c = GB.MLPBackground({"type": "mlp"}, generator=torch.Generator().manual_seed(12))
    assert list(a.state_dict()) == ["mlp.params"] and a.mlp.params.shape == (768,) and a.mlp.params.dtype == torch.float32
    assert torch.equal(a.mlp.params, b.mlp.params) and not torch.equal(a.mlp.params, c.mlp.params)      # seedable
    w = a.mlp.params.detach()
    assert float(w.abs().max()) <= BC.INIT_BOUND and float(w.abs().max()) > 0.95 * BC.INIT_BOUND
    assert abs(float(w.mean())) < 0.05 and abs(float(w.std()) - BC.INIT_BOUND / 3 ** 0.5) < 0.02  # uniform
    c.load_state_dict(a.state_dict())
    assert torch.equal(c.mlp.params, a.mlp.params)
    blocks = GB.camera_blocks(torch.arange(32.0).view(2, 4, 4), torch.tensor([[1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 8.0]]))
    assert blocks.shape == (2, 16) and blocks[1].tolist() == [*range(16, 28), 5.0, 6.0, 7.0, 8.0]


def test_model_accepts_the_mlp_background_type():
    """the part that needs no GPU: the type is taken and holds the reference's `mlp.params`, random_aug with it is refused, an unknown
    type still raises, and the per-camera call form is refused for a per-pixel background"""
    from gsgen_amd.model import _Background
    bg = _Background({"type": "mlp"})
    assert list(bg.state_dict()) == ["mlp.params"] and [tuple(p.shape) for p in bg.parameters()] == [(768,)]
    with pytest.raises(NotImplementedError, match="random_aug"):
        _Background({"type": "mlp", "random_aug": True})
    with pytest.raises(NotImplementedError, match="background type 'tcnn'"):
        _Background({"type": "tcnn"})
    with pytest.raises(TypeError, match="colour per pixel"):
        bg(2, "cpu")
    with pytest.raises(ValueError, match="no CPU implementation"):
        bg(torch.rand(8, 9, 3))


def test_package_exports_the_background_names():
    import gsgen_amd
    from gsgen_amd import background as GB
    for name in ("MLPBackground", "mlp_background", "mlp_background_images", "mlp_background_over"):
        assert getattr(gsgen_amd, name) is getattr(GB, name)
