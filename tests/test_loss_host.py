"""gsgen_amd/csrc/loss.hip on the CPU SIMT emulator (oracle/emu) against the torch restatement of tests/loss_cases.py, and the
argument checks of gsgen_amd.loss that need no GPU.  The file is compiled without contraction and spells its multiply-adds as
fmaf, so the emulated kernels perform the GPU's fp32 operations in the GPU's order: the errors printed here are the GPU's."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import loss_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSGEN_EUNSUPPORTED, GSGEN_EINVAL, GSGEN_EWORKSPACE = -2, -3, -4
BASE = {"l2": 0, "l1": 1}


@pytest.fixture(scope="module")
def loss_emu(tmp_path_factory):
    """loss.hip compiled with g++ on the emulator headers, with the flags of oracle/Makefile's `emu` rule (into tmp: nothing under
    oracle/ changes)"""
    out = tmp_path_factory.mktemp("loss_emu") / "libloss_emu.so"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                           "-Wno-unknown-pragmas", "-DGSGEN_EMU_KNOBS=1", "-I", os.path.join(ROOT, "oracle", "emu"), "-x", "c++",
                           os.path.join(ROOT, "gsgen_amd", "csrc", "loss.hip"), "-o", str(out), "-lm"])
    lib = C.CDLL(str(out))
    u32, vp, f32, i32, sz = C.c_uint32, C.c_void_p, C.c_float, C.c_int, C.c_size_t
    lib.gsgen_image_loss_workspace_bytes.argtypes = [u32, u32, u32, u32, u32, i32]
    lib.gsgen_image_loss_workspace_bytes.restype = sz
    lib.gsgen_image_loss_forward.argtypes = [vp, vp, u32, u32, u32, u32, u32, f32, i32, i32, vp, vp, sz, vp]
    lib.gsgen_image_loss_forward.restype = i32
    lib.gsgen_image_loss_backward.argtypes = [vp, vp, u32, u32, u32, u32, u32, f32, i32, vp, vp, vp, sz, vp]
    lib.gsgen_image_loss_backward.restype = i32
    lib.gsgen_image_loss_emu_filt_adjoint.argtypes = [vp, u32, u32, u32, u32, vp, vp]
    lib.gsgen_image_loss_emu_filt_adjoint.restype = i32
    return lib


def run_loss(lib, out, gt, w, base, ws, scale=1.0, want_grad=True):
    """-> (loss float32[3] = total, ssim term, base term; d total / d out float32 [B,H,W,C] or None)"""
    out, gt = np.ascontiguousarray(out, np.float32), np.ascontiguousarray(gt, np.float32)
    B, H, W, Ch = out.shape
    nbytes = lib.gsgen_image_loss_workspace_bytes(B, H, W, Ch, ws, int(want_grad))
    assert nbytes > 0
    wsb = np.full(nbytes + 3, 0xA5, np.uint8)[3:]  # (an unaligned, dirty base: the carve aligns it and nothing is assumed zero)
    loss = np.full(3, np.nan, np.float32)
    rc = lib.gsgen_image_loss_forward(out.ctypes.data, gt.ctypes.data, B, H, W, Ch, ws, w, BASE[base], int(want_grad), loss.ctypes.data,
                                      wsb.ctypes.data, wsb.size, None)
    assert rc == 0, rc
    if not want_grad:
        return loss, None
    grad = np.full(out.shape, np.nan, np.float32)
    s = np.array([scale], np.float32)
    rc = lib.gsgen_image_loss_backward(out.ctypes.data, gt.ctypes.data, B, H, W, Ch, ws, w, BASE[base], s.ctypes.data, grad.ctypes.data,
                                       wsb.ctypes.data, wsb.size, None)
    assert rc == 0, rc
    return loss, grad


@pytest.mark.parametrize("name", LC.NAMES)
def test_emulated_image_loss_meets_the_restatements_own_error(loss_emu, name):
    c = LC.case(name)
    loss, grad = run_loss(loss_emu, c["out"], c["gt"], c["w"], c["base"], c["ws"])
    if c["kind"] == "same":
        LC.check_same(name, loss[0], grad)
    else:
        LC.check_bound(name, loss[0], grad)
    # the two terms the total is made of, and the forward alone
    assert abs(c["w"] * float(loss[1]) + (1 - c["w"]) * float(loss[2]) - float(loss[0])) <= 2.0 ** -22 * max(abs(float(loss[0])), 1e-30)
    only, _ = run_loss(loss_emu, c["out"], c["gt"], c["w"], c["base"], c["ws"], want_grad=False)
    assert only.tobytes() == loss.tobytes()


@pytest.mark.parametrize("C_", [1, 3])
@pytest.mark.parametrize("ws", [3, 5, 7, 9, 11])
def test_emulated_filter_adjoint_alone_against_autograd(loss_emu, ws, C_):
    """filtT of a random map on a 6 x 9 image (both folds hit the same rows at ws = 11) = autograd of sum(filt(x) * map)"""
    H, W = 6, 9
    gen = torch.Generator().manual_seed(ws * 10 + C_)
    m = torch.randn(H, W, C_, generator=gen, dtype=torch.float64).float()
    x = torch.zeros(1, C_, H, W, dtype=torch.float64, requires_grad=True)
    (LC.filt(x, ws) * m.double().moveaxis(-1, 0)[None]).sum().backward()
    want = x.grad[0].moveaxis(0, -1).numpy()
    mm = np.ascontiguousarray(m.numpy())
    got, scratch = np.full((H, W, C_), np.nan, np.float32), np.zeros(2 * H * W * C_, np.float32)
    assert loss_emu.gsgen_image_loss_emu_filt_adjoint(mm.ctypes.data, H, W, C_, ws, got.ctypes.data, scratch.ctypes.data) == 0
    np.testing.assert_allclose(got, want, rtol=0, atol=2.0 ** -20 * np.abs(want).max())  # (<= 2 ws fp32 roundings of O(1) sums)


def test_emulated_filter_adjoint_across_tiles(loss_emu):
    """the same on 70 x 41: interior tile borders (zero-extended halo, no fold) and partial tiles"""
    H, W, ws = 70, 41, 11
    m = torch.randn(H, W, 3, generator=torch.Generator().manual_seed(7), dtype=torch.float64).float()
    x = torch.zeros(1, 3, H, W, dtype=torch.float64, requires_grad=True)
    (LC.filt(x, ws) * m.double().moveaxis(-1, 0)[None]).sum().backward()
    want = x.grad[0].moveaxis(0, -1).numpy()
    mm = np.ascontiguousarray(m.numpy())
    got, scratch = np.full((H, W, 3), np.nan, np.float32), np.zeros(2 * H * W * 3, np.float32)
    assert loss_emu.gsgen_image_loss_emu_filt_adjoint(mm.ctypes.data, H, W, 3, ws, got.ctypes.data, scratch.ctypes.data) == 0
    np.testing.assert_allclose(got, want, rtol=0, atol=2.0 ** -20 * np.abs(want).max())


def test_emulated_image_loss_is_bit_identical_from_run_to_run_and_scales_with_the_upstream_scalar(loss_emu):
    c = LC.case("noise-2x37x53x3-ws11-l2")
    l0, g0 = run_loss(loss_emu, c["out"], c["gt"], 0.2, "l2", 11)
    l1, g1 = run_loss(loss_emu, c["out"], c["gt"], 0.2, "l2", 11)
    assert l0.tobytes() == l1.tobytes() and g0.tobytes() == g1.tobytes()
    _, g3 = run_loss(loss_emu, c["out"], c["gt"], 0.2, "l2", 11, scale=3.0)
    assert np.abs(g3 - 3.0 * g0).max() <= np.spacing(np.abs(3.0 * g0).max())
    _, g2 = run_loss(loss_emu, c["out"], c["gt"], 0.2, "l2", 11, scale=2.0)
    assert g2.tobytes() == (2.0 * g0).astype(np.float32).tobytes()  # (a power of two scales every product exactly)


def test_emulated_image_loss_argument_checks(loss_emu):
    lib = loss_emu
    img = np.random.default_rng(0).random((2, 12, 12, 3)).astype(np.float32)
    loss, grad, one = np.zeros(3, np.float32), np.full(img.shape, 7.0, np.float32), np.ones(1, np.float32)
    wsb = np.zeros(1 << 20, np.uint8)

    def fwd(B, H, W, Ch, ws, base=0, nbytes=wsb.size, out=img.ctypes.data):
        return lib.gsgen_image_loss_forward(out, img.ctypes.data, B, H, W, Ch, ws, 0.2, base, 1, loss.ctypes.data, wsb.ctypes.data, nbytes, None)

    def bwd(B, H, W, Ch, ws, base=0, nbytes=wsb.size, scale=one.ctypes.data):
        return lib.gsgen_image_loss_backward(img.ctypes.data, img.ctypes.data, B, H, W, Ch, ws, 0.2, base, scale, grad.ctypes.data,
                                             wsb.ctypes.data, nbytes, None)
    for call in (fwd, bwd):
        assert call(2, 12, 12, 3, 13) == GSGEN_EUNSUPPORTED      # window > 11
        assert call(2, 12, 12, 2, 11) == GSGEN_EUNSUPPORTED      # C not in {1, 3}
        assert call(2, 12, 12, 4, 11) == GSGEN_EUNSUPPORTED
        assert call(2, 12, 12, 3, 11, base=2) == GSGEN_EUNSUPPORTED
        assert call(2, 12, 12, 3, 10) == GSGEN_EINVAL            # even window
        assert call(2, 12, 12, 3, 1) == GSGEN_EINVAL             # below 3
        assert call(2, 5, 12, 3, 11) == GSGEN_EINVAL             # H <= p: torch's reflect limit
        assert call(2, 12, 5, 3, 11) == GSGEN_EINVAL
        assert call(0, 12, 12, 3, 11) == 0                       # empty: clean, nothing written
    assert (grad == 7.0).all() and (loss == 0).all()
    assert fwd(2, 12, 12, 3, 11, out=None) == GSGEN_EINVAL
    assert bwd(2, 12, 12, 3, 11, scale=None) == GSGEN_EINVAL
    assert lib.gsgen_image_loss_workspace_bytes(2, 12, 12, 2, 11, 1) == 0 and lib.gsgen_image_loss_workspace_bytes(2, 12, 12, 3, 10, 1) == 0
    assert lib.gsgen_image_loss_workspace_bytes(2, 5, 12, 3, 11, 1) == 0
    need = lib.gsgen_image_loss_workspace_bytes(2, 12, 12, 3, 11, 1)
    small = lib.gsgen_image_loss_workspace_bytes(2, 12, 12, 3, 11, 0)
    assert 0 < small < need <= wsb.size and need - small >= 3 * img.size * 4
    assert fwd(2, 12, 12, 3, 11, nbytes=need - 1) == GSGEN_EWORKSPACE and bwd(2, 12, 12, 3, 11, nbytes=need - 1) == GSGEN_EWORKSPACE
    assert (grad == 7.0).all() and (loss == 0).all()             # a refused call enqueues nothing
    assert fwd(2, 6, 6, 3, 11, nbytes=need) == 0 and fwd(2, 12, 12, 3, 11, nbytes=need) == 0 and bwd(2, 12, 12, 3, 11, nbytes=need) == 0
    assert np.isfinite(grad).all() and loss[0] == 0  # (out == gt here)


# --- gsgen_amd.loss: the refusals, which need neither a GPU nor the library ------------------------------------------------
def test_python_refusals():
    """every check comes before the device check, so CPU tensors reach each of them; a well-formed CPU call is refused last"""
    from gsgen_amd import loss as GL
    img = lambda *s, **k: torch.rand(*s, **k)  # noqa: E731
    with pytest.raises(ValueError, match="no CPU implementation"):
        GL.image_loss(img(2, 16, 16, 3), img(2, 16, 16, 3))
    with pytest.raises(ValueError, match="no CPU implementation"):
        GL.ssim_loss(img(16, 16, 1), img(16, 16, 1), 7)
    with pytest.raises(ValueError, match="no CPU implementation"):
        GL.image_loss(img(2, 16, 16, 3, requires_grad=True), img(2, 16, 16, 3), 0.5, "l2", 3)
    with pytest.raises(NotImplementedError, match="float32"):
        GL.image_loss(img(2, 16, 16, 3).half(), img(2, 16, 16, 3).half())
    with pytest.raises(NotImplementedError, match="float32"):
        GL.image_loss(img(2, 16, 16, 3), img(2, 16, 16, 3).double())
    with pytest.raises(NotImplementedError, match="gt requires"):
        GL.image_loss(img(2, 16, 16, 3), img(2, 16, 16, 3, requires_grad=True))
    with pytest.raises(ValueError, match="differ in shape"):
        GL.image_loss(img(2, 16, 16, 3), img(2, 16, 15, 3))
    with pytest.raises(ValueError, match=r"\[B, H, W, C\]"):
        GL.image_loss(img(16, 3), img(16, 3))
    with pytest.raises(ValueError, match="window_size"):
        GL.image_loss(img(2, 16, 16, 3), img(2, 16, 16, 3), window_size=10)
    with pytest.raises(ValueError, match="window_size"):
        GL.ssim_loss(img(2, 16, 16, 3), img(2, 16, 16, 3), window_size=1)
    with pytest.raises(ValueError, match="reflect"):
        GL.image_loss(img(2, 5, 16, 3), img(2, 5, 16, 3))
    with pytest.raises(ValueError, match="reflect"):
        GL.image_loss(img(16, 3, 3), img(16, 3, 3), window_size=7)
    with pytest.raises(ValueError, match="empty batch"):
        GL.image_loss(img(0, 16, 16, 3), img(0, 16, 16, 3))
    with pytest.raises(NotImplementedError, match="channels"):
        GL.image_loss(img(2, 16, 16, 4), img(2, 16, 16, 4))
    with pytest.raises(NotImplementedError, match="window_size 13"):
        GL.image_loss(img(2, 16, 16, 3), img(2, 16, 16, 3), window_size=13)
    for bad in (lambda: GL.image_loss(img(2, 16, 16, 3), img(2, 16, 16, 3), type="huber"), lambda: GL.get_image_loss(0.2, "huber"),
                lambda: GL.get_loss_fn(types.SimpleNamespace(loss_fn="huber", ssim_loss_mult=0.2, ssim_loss_win_size=11))):
        with pytest.raises(NotImplementedError, match="huber"):
            bad()
    fn = GL.get_loss_fn(types.SimpleNamespace(loss_fn="l2", ssim_loss_mult=0.2, ssim_loss_win_size=11))
    with pytest.raises(ValueError, match="no CPU implementation"):
        fn(img(16, 16, 3), img(16, 16, 3))
    with pytest.raises(ValueError, match="no CPU implementation"):
        GL.get_image_loss(0.2, "l1")(img(1, 16, 16, 3), img(1, 16, 16, 3))


def test_package_exports_the_loss_names():
    import gsgen_amd
    from gsgen_amd import loss as GL
    for name in ("ssim_loss", "image_loss", "get_image_loss", "get_loss_fn"):
        assert getattr(gsgen_amd, name) is getattr(GL, name)
