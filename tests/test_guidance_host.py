"""gsgen_amd/csrc/guidance_seam.hip on the CPU SIMT emulator (oracle/emu) against the torch restatements of tests/guidance_cases.py, the
file's bit-level fp16 routines against numpy's float16 casts, and the argument checks of gsgen_amd.guidance that need no GPU.  The file
is compiled without contraction, so the emulated kernels perform the GPU's operations in the GPU's order: the errors printed here
are the GPU's, up to the fp16 conversions, which are the hardware's there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import guidance_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSGEN_EUNSUPPORTED, GSGEN_EINVAL, GSGEN_EWORKSPACE = -2, -3, -4
GUARD = 8  # sentinel elements on either side of every output buffer


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """guidance_seam.hip compiled with g++ on the emulator headers, with the flags tests/test_depth_loss_host.py uses (into tmp:
    nothing under oracle/ changes)"""
    out = tmp_path_factory.mktemp("guidance_emu") / "libguidance_emu.so"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                           "-Wno-unknown-pragmas", "-DGSGEN_EMU_KNOBS=1", "-I", os.path.join(ROOT, "oracle", "emu"), "-x", "c++",
                           os.path.join(ROOT, "gsgen_amd", "csrc", "guidance_seam.hip"), "-o", str(out), "-lm"])
    lib = C.CDLL(str(out))
    u32, vp, i32, sz, f32 = C.c_uint32, C.c_void_p, C.c_int, C.c_size_t, C.c_float
    lib.gsgen_guidance_input_workspace_bytes.argtypes = [u32, u32, u32, u32]
    lib.gsgen_guidance_input_workspace_bytes.restype = sz
    lib.gsgen_guidance_input_forward.argtypes = [vp, u32, u32, u32, u32, u32, u32, f32, f32, i32, i32, vp, i32, vp, sz, vp]
    lib.gsgen_guidance_input_forward.restype = i32
    lib.gsgen_guidance_input_backward.argtypes = [vp, i32, i32, u32, u32, u32, u32, u32, u32, f32, vp, vp, sz, vp]
    lib.gsgen_guidance_input_backward.restype = i32
    lib.gsgen_sds_loss_workspace_bytes.argtypes = [u32, u32]
    lib.gsgen_sds_loss_workspace_bytes.restype = sz
    lib.gsgen_sds_loss_forward.argtypes = [vp, u32, u32, i32, f32, vp, vp, sz, vp]
    lib.gsgen_sds_loss_forward.restype = i32
    lib.gsgen_sds_loss_backward.argtypes = [u32, u32, vp, vp, vp, sz, vp]
    lib.gsgen_sds_loss_backward.restype = i32
    lib.gsgen_guidance_emu_constants.argtypes = [vp]
    lib.gsgen_guidance_emu_f32_to_f16.argtypes = [vp, vp, sz]
    lib.gsgen_guidance_emu_f16_to_f32.argtypes = [vp, vp, sz]
    return lib


def ptr(a):
    return None if a is None else a.ctypes.data


def guarded(count, dtype, sentinel, offset=0):
    """-> (the whole buffer, the `count` elements inside it that a kernel may write), `offset` elements off the aligned position"""
    full = np.full(count + 2 * GUARD + offset, sentinel, dtype)
    return full, full[GUARD + offset:GUARD + offset + count]


def guards_intact(full, inner, sentinel):
    lo = (inner.ctypes.data - full.ctypes.data) // full.itemsize
    edge = np.concatenate([full[:lo], full[lo + inner.size:]])
    return edge.size >= 2 * GUARD and edge.tobytes() == np.full(edge.size, sentinel, full.dtype).tobytes()


def dirty_workspace(nbytes):
    return np.full(nbytes + 3, 0xA5, np.uint8)[3:]  # (an unaligned, dirty base: the carve aligns it and nothing is assumed zero)


def resize_forward(lib, x, OH, OW, scale, shift, half, planar, wsb=None, offset=0):
    """x [B,H,W,C] -> (out as float32 [B,OH,OW,C], the raw bits, the workspace with its tables)"""
    x = np.ascontiguousarray(x, np.float32)
    B, H, W, Cc = x.shape
    build = wsb is None
    if build:
        nbytes = lib.gsgen_guidance_input_workspace_bytes(H, W, OH, OW)
        assert nbytes > 0
        wsb = dirty_workspace(nbytes)
    sentinel = 0x7bff if half else 7.0
    full, out = guarded(B * Cc * OH * OW, np.uint16 if half else np.float32, sentinel, offset)
    rc = lib.gsgen_guidance_input_forward(ptr(x), B, H, W, Cc, OH, OW, scale, shift, int(half), int(planar), ptr(out), int(build), ptr(wsb),
                                          wsb.size, None)
    assert rc == 0, rc
    assert guards_intact(full, out, sentinel)
    vals = out.view(np.float16).astype(np.float32) if half else out
    vals = vals.reshape((B, Cc, OH, OW) if planar else (B, OH, OW, Cc))
    return GC.from_layout(vals, planar), out.copy(), wsb


def resize_backward(lib, g, shape, scale, g_half, planar, wsb):
    """g [B,OH,OW,C] float32 -> d / d x [B,H,W,C] float32, through the tables a forward left in wsb"""
    B, H, W, Cc = shape
    OH, OW = g.shape[1:3]
    gl = GC.to_layout(np.asarray(g, np.float32), planar)
    if g_half:
        assert (gl.astype(np.float16).astype(np.float32) == gl).all()  # (exactly representable)
        gl = gl.astype(np.float16)
    full, gx = guarded(B * H * W * Cc, np.float32, 7.0)
    rc = lib.gsgen_guidance_input_backward(ptr(gl), int(g_half), int(planar), B, H, W, Cc, OH, OW, scale, ptr(gx), ptr(wsb), wsb.size, None)
    assert rc == 0, rc
    assert guards_intact(full, gx, 7.0)
    return gx.reshape(shape).copy()


def test_the_constants_the_cases_assume(emu):
    k = np.zeros(3, np.uint32)
    emu.gsgen_guidance_emu_constants(k.ctypes.data)
    assert k[0] == GC.KPIX and k[2] == GC.KCHUNK
    assert 4 * 5 * 7 < GC.KCHUNK < 4 * 64 * 64 and (4 * 5 * 7) % k[1] != 0  # the SDS shapes: under one chunk, and sixteen


@pytest.mark.parametrize("case", GC.RESIZE_CASES, ids=GC.resize_id)
def test_emulated_resize_meets_the_restatements_own_error(emu, case):
    H, W, OH, OW, Cc, B = case
    d = GC.resize_case(case)
    name = GC.resize_id(case)
    dead_y, dead_x = GC.untouched(H, OH), GC.untouched(W, OW)
    for planar in (True, False):
        wsb = None
        for half in (False, True):
            out, bits, wsb = resize_forward(emu, d["x"], OH, OW, GC.SCALE, GC.SHIFT, half, planar)
            GC.check(f"{name} out planar={planar} half={half}", out, d["out64"], d["out32"], half)
            # a base one element off the aligned position, and the tables read back instead of rebuilt: the same bits
            _, bits1, _ = resize_forward(emu, d["x"], OH, OW, GC.SCALE, GC.SHIFT, half, planar, wsb=wsb, offset=1)
            assert bits1.tobytes() == bits.tobytes()
        for g_half, which in ((False, "32"), (True, "16")):
            gx = resize_backward(emu, d["g" + which], d["x"].shape, GC.SCALE, g_half, planar, wsb)
            GC.check(f"{name} grad planar={planar} g_half={g_half}", gx, d[f"gx{which}64"], d[f"gx{which}32"])
            # an input row or column no output reads: exact zeros
            assert not gx[:, dead_y].any() and not gx[:, :, dead_x].any()
    if H in (67, 23):
        assert dead_y.sum() == {67: 51, 23: 10}[H]
    if OH >= H or (H, OH) == (25, 16):
        assert not dead_y.any()


def test_identity_is_bit_exact(emu):
    """16 x 16 -> 16 x 16: every l1 is 0, so the fp32 forward is x * 2 - 1 in fp32 and the backward 2 * g, bit for bit"""
    for case in ((16, 16, 16, 16, 3, 3), (16, 16, 16, 16, 1, 3)):
        d = GC.resize_case(case)
        want = (torch.as_tensor(d["x"].copy()) * 2.0 - 1.0).numpy()
        for planar in (True, False):
            out, _, wsb = resize_forward(emu, d["x"], 16, 16, 2.0, -1.0, False, planar)
            assert np.ascontiguousarray(out).tobytes() == want.tobytes()
            plain, _, _ = resize_forward(emu, d["x"], 16, 16, 1.0, 0.0, False, planar)
            assert np.ascontiguousarray(plain).tobytes() == d["x"].tobytes()
            for g_half, g in ((False, d["g32"]), (True, d["g16"])):
                gx = resize_backward(emu, g, d["x"].shape, 2.0, g_half, planar, wsb)
                assert gx.tobytes() == (2.0 * g).astype(np.float32).tobytes()


@pytest.mark.parametrize("case", [c for c in GC.RESIZE_CASES if c[5] == 3], ids=GC.resize_id)
def test_backward_is_the_adjoint_of_the_forward(emu, case):
    """<forward(x), g> = <x, backward(g)> for the fp32, no-affine form.  Both sums are taken in fp64 from fp32 factors, so they differ
    by the factors' rounding alone: each term of either sum carries a relative error of a few 2^-24, the sums differ by at most that
    times the sum of the terms' magnitudes.  The bound is the rule of guidance_cases.check on that scale: 4 x max(what the fp32
    restatement's two sums differ by, 2^-22 sum |terms|)."""
    H, W, OH, OW, Cc, B = case
    d = GC.resize_case(case)
    out, _, wsb = resize_forward(emu, d["x"], OH, OW, 1.0, 0.0, False, True)
    gx = resize_backward(emu, d["g32"], d["x"].shape, 1.0, False, True, wsb)
    g, x = d["g32"].astype(np.float64), d["x"].astype(np.float64)
    lhs, rhs = (out.astype(np.float64) * g).sum(), (x * gx.astype(np.float64)).sum()
    e32 = abs((d["out_plain32"] * g).sum() - (x * d["gx32_plain32"]).sum())
    bound = 4 * max(e32, GC.FLOOR * np.abs(d["out_plain64"] * g).sum())
    print(f"{GC.resize_id(case)}: <f(x), g> {lhs:.9e} <x, b(g)> {rhs:.9e} differ by {abs(lhs - rhs):.3e} bound {bound:.3e} (fp32 torch {e32:.3e})")
    assert abs(lhs - rhs) <= bound
    GC.check("plain out", out, d["out_plain64"], d["out_plain32"])
    GC.check("plain grad", gx, d["gx32_plain64"], d["gx32_plain32"])


def run_sds(lib, grad, clip, scale=1.0, backward=True):
    grad = np.ascontiguousarray(grad, np.float32)
    B, n = grad.shape[0], grad[0].size
    nbytes = lib.gsgen_sds_loss_workspace_bytes(B, n)
    assert nbytes > 0
    wsb = dirty_workspace(nbytes)
    full, out = guarded(2 + B, np.float32, 7.0)
    rc = lib.gsgen_sds_loss_forward(ptr(grad), B, n, int(clip is not None), 0.0 if clip is None else clip, ptr(out), ptr(wsb), wsb.size, None)
    assert rc == 0, rc
    assert guards_intact(full, out, 7.0)
    g = None
    if backward:
        s = np.array([scale], np.float32)
        gfull, g = guarded(B * n, np.float32, 7.0)
        rc = lib.gsgen_sds_loss_backward(B, n, ptr(s), ptr(g), ptr(wsb), wsb.size, None)
        assert rc == 0, rc
        assert guards_intact(gfull, g, 7.0)
        g = g.reshape(grad.shape).copy()
    return out[0].copy(), out[2:].copy(), out[1].copy(), g


@pytest.mark.parametrize("case", GC.SDS_CASES, ids=GC.sds_id)
def test_emulated_sds_loss_meets_the_restatements_own_error(emu, case):
    d = GC.sds_case(case)
    loss, each, norm, g = run_sds(emu, d["grad"], case[1])
    GC.check_sds(case, loss, each, norm, g)
    assert np.isfinite(loss) and np.isfinite(each).all() and np.isfinite(norm) and np.isfinite(g).all()
    if case[2] == "zeros":
        assert loss == 0.0 and norm == 0.0 and not each.any() and not g.any()
    if case[2] == "nonfinite":
        assert np.isnan(d["grad"]).sum() >= 3 and np.isinf(d["grad"]).sum() == 6
        assert (np.abs(g[np.isinf(d["grad"])]) == np.float32(case[1]) / np.float32(case[0][0])).all()  # +-inf: clipped
    # bit-identical from run to run, and the forward alone
    again = run_sds(emu, d["grad"], case[1])
    assert all(a.tobytes() == b.tobytes() for a, b in zip((loss, each, norm, g), again))
    only = run_sds(emu, d["grad"], case[1], backward=False)
    assert only[0].tobytes() == loss.tobytes() and only[1].tobytes() == each.tobytes()
    # the upstream scalar
    _, _, _, g3 = run_sds(emu, d["grad"], case[1], scale=3.0)
    GC.check_sds(case, loss, each, norm, g3, scale=3.0)
    _, _, _, g2 = run_sds(emu, d["grad"], case[1], scale=2.0)
    assert g2.tobytes() == (2.0 * g).astype(np.float32).tobytes()


def test_sds_without_a_clip_keeps_infinities_at_flt_max(emu):
    grad = np.zeros((1, 4, 2, 2), np.float32)
    grad[0, 0, 0, 0], grad[0, 1, 0, 0], grad[0, 2, 0, 0] = np.inf, -np.inf, np.nan
    loss, each, norm, g = run_sds(emu, grad, None)
    fmax = np.finfo(np.float32).max
    assert g[0, 0, 0, 0] == fmax and g[0, 1, 0, 0] == -fmax and g[0, 2, 0, 0] == 0.0
    assert np.isinf(loss) and np.isinf(norm)  # (2 FLT_MAX^2 is past fp32, as it is in torch)


def test_half_conversions_against_numpy(emu):
    """float16 -> float32: all 65 536 patterns, bit for bit.  float32 -> float16, round to nearest even: a seeded million of random
    bit patterns, every tie between two neighbouring halves (both signs), the subnormal range, the overflow threshold and the
    specials"""
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    f = np.zeros(65536, np.float32)
    emu.gsgen_guidance_emu_f16_to_f32(ptr(h), ptr(f), h.size)
    assert f.view(np.uint32).tobytes() == h.view(np.float16).astype(np.float32).view(np.uint32).tobytes()

    rng = np.random.default_rng(16)
    finite = h[(h & 0x7c00) != 0x7c00].view(np.float16).astype(np.float32)
    pos = np.sort(finite[finite >= 0])
    ties = ((pos[:-1].astype(np.float64) + pos[1:].astype(np.float64)) / 2).astype(np.float32)  # (exact in fp32)
    assert (ties.astype(np.float64) * 2 == pos[:-1].astype(np.float64) + pos[1:]).all()
    near = np.concatenate([np.nextafter(ties, np.float32(0)), np.nextafter(ties, np.float32(np.inf))])
    edge = np.array([65504.0, 65519.996, 65520.0, 65520.004, 65536.0, 1e30, np.inf, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 2.0 ** -26,
                     np.nextafter(np.float32(2.0 ** -25), np.float32(1)), 1e-45, 0.0], np.float32)
    sub = (rng.random(100000) * 2.0 ** -13).astype(np.float32)
    rand = rng.integers(0, 2 ** 32, 1000000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    vals = np.concatenate([rand, ties, -ties, near, -near, edge, -edge, sub, -sub, finite, np.array([np.nan, -np.nan], np.float32)])
    got = np.zeros(vals.size, np.uint16)
    emu.gsgen_guidance_emu_f32_to_f16(ptr(np.ascontiguousarray(vals)), ptr(got), vals.size)
    with np.errstate(over="ignore"):
        want = vals.astype(np.float16).view(np.uint16)
    nan = np.isnan(vals)
    assert nan.sum() > 1000 and (got[~nan] == want[~nan]).all()
    assert np.isnan(got[nan].view(np.float16)).all() and ((got[nan] ^ want[nan]) & 0x8000 == 0).all()  # a NaN stays one, sign kept


def test_emulated_argument_checks(emu):
    lib = emu
    B, H, W, Cc, OH, OW = 2, 5, 7, 3, 4, 6
    x = np.random.default_rng(0).random((B, H, W, Cc)).astype(np.float32)
    out, g, gx = np.full((B, Cc, OH, OW), 7.0, np.float32), np.ones((B, Cc, OH, OW), np.float32), np.full(x.shape, 7.0, np.float32)
    wsb = np.zeros(1 << 14, np.uint8)

    def fwd(B=B, H=H, W=W, Cc=Cc, OH=OH, OW=OW, x=x, out=out, ws=wsb, nbytes=wsb.size):
        return lib.gsgen_guidance_input_forward(ptr(x), B, H, W, Cc, OH, OW, 2.0, -1.0, 0, 1, ptr(out), 1, ptr(ws), nbytes, None)

    def bwd(B=B, H=H, W=W, Cc=Cc, OH=OH, OW=OW, g=g, gx=gx, ws=wsb, nbytes=wsb.size):
        return lib.gsgen_guidance_input_backward(ptr(g), 0, 1, B, H, W, Cc, OH, OW, 2.0, ptr(gx), ptr(ws), nbytes, None)
    for call in (fwd, bwd):
        for zero in ("B", "H", "W", "Cc", "OH", "OW"):
            assert call(**{zero: 0}) == GSGEN_EINVAL, zero
        assert call(ws=None) == GSGEN_EINVAL
        for Cbad in (2, 4):
            assert call(Cc=Cbad) == GSGEN_EUNSUPPORTED
        assert call(H=70000) == GSGEN_EUNSUPPORTED and call(OW=70000) == GSGEN_EUNSUPPORTED
    assert fwd(x=None) == GSGEN_EINVAL and fwd(out=None) == GSGEN_EINVAL
    assert bwd(g=None) == GSGEN_EINVAL and bwd(gx=None) == GSGEN_EINVAL
    assert lib.gsgen_guidance_input_workspace_bytes(0, W, OH, OW) == 0 and lib.gsgen_guidance_input_workspace_bytes(H, W, OH, 70000) == 0
    need = lib.gsgen_guidance_input_workspace_bytes(H, W, OH, OW)
    assert 0 < need <= wsb.size and need < lib.gsgen_guidance_input_workspace_bytes(H, W, 800, OW)
    assert fwd(nbytes=need - 1) == GSGEN_EWORKSPACE and bwd(nbytes=need - 1) == GSGEN_EWORKSPACE
    assert (out == 7.0).all() and (gx == 7.0).all() and not wsb.any()  # a refused call enqueues nothing
    assert fwd(nbytes=need) == 0 and bwd(nbytes=need) == 0
    assert (out != 7.0).all() and (gx != 7.0).all()

    n = 4 * 5 * 7
    grad, loss, one, gl = np.ones((B, n), np.float32), np.full(2 + B, 7.0, np.float32), np.ones(1, np.float32), np.full((B, n), 7.0, np.float32)

    def sfwd(B=B, n=n, grad=grad, loss=loss, ws=wsb, nbytes=wsb.size, use_clip=1, clip=1.0):
        return lib.gsgen_sds_loss_forward(ptr(grad), B, n, use_clip, clip, ptr(loss), ptr(ws), nbytes, None)

    def sbwd(B=B, n=n, scale=one, gl=gl, ws=wsb, nbytes=wsb.size):
        return lib.gsgen_sds_loss_backward(B, n, ptr(scale), ptr(gl), ptr(ws), nbytes, None)
    wsb[:] = 0
    for call in (sfwd, sbwd):
        assert call(B=0) == GSGEN_EINVAL and call(n=0) == GSGEN_EINVAL and call(ws=None) == GSGEN_EINVAL
        assert call(B=70000) == GSGEN_EUNSUPPORTED
    assert sfwd(grad=None) == GSGEN_EINVAL and sfwd(loss=None) == GSGEN_EINVAL
    assert sfwd(clip=-1.0) == GSGEN_EINVAL and sfwd(clip=float("nan")) == GSGEN_EINVAL and sfwd(use_clip=0, clip=-1.0) == 0
    assert sbwd(scale=None) == GSGEN_EINVAL and sbwd(gl=None) == GSGEN_EINVAL
    assert lib.gsgen_sds_loss_workspace_bytes(0, n) == 0 and lib.gsgen_sds_loss_workspace_bytes(70000, n) == 0
    need = lib.gsgen_sds_loss_workspace_bytes(B, n)
    assert 0 < need <= wsb.size and need < lib.gsgen_sds_loss_workspace_bytes(B, 4 * 64 * 64)
    loss[:] = 7.0
    wsb[:] = 0
    assert sfwd(nbytes=need - 1) == GSGEN_EWORKSPACE and sbwd(nbytes=need - 1) == GSGEN_EWORKSPACE
    assert (loss == 7.0).all() and (gl == 7.0).all() and not wsb.any()
    assert sfwd(nbytes=need) == 0 and sbwd(nbytes=need) == 0
    assert loss[0] == 0.5 * n and loss[1] == np.float32(np.sqrt(B * n)) and (loss[2:] == 0.5 * n).all() and (gl == 0.5).all()


# --- gsgen_amd.guidance: the refusals, which need neither a GPU nor the library ------------------------------------------------
def test_python_refusals():
    """every check comes before the device check, so CPU tensors reach each of them; a well-formed CPU call is refused last"""
    from gsgen_amd import guidance as GG
    d = lambda *s, **k: torch.rand(*s, **k)  # noqa: E731
    for img in (d(2, 8, 9, 3), d(8, 9, 3), d(2, 8, 9, 1), d(2, 8, 9, 3, requires_grad=True)):
        for fn in (GG.to_guidance, GG.vae_input, GG.if_input, GG.rgb_as_latents, lambda t: GG.resize(t, (4, 5)),
                   lambda t: GG.to_guidance(t, 7, 1.0, 0.0, torch.float32, "BHWC")):
            with pytest.raises(ValueError, match="no CPU implementation"):
                fn(img)
    with pytest.raises(ValueError, match=r"\[B, H, W, C\]"):
        GG.to_guidance(d(8, 9))
    with pytest.raises(ValueError, match=r"\[B, H, W, C\]"):
        GG.vae_input([1.0])
    with pytest.raises(NotImplementedError, match="1 or 3"):
        GG.to_guidance(d(2, 8, 9, 4))
    with pytest.raises(NotImplementedError, match="1 or 3"):
        GG.resize(d(8, 9, 2), 4)
    with pytest.raises(ValueError, match="size must be"):
        GG.to_guidance(d(2, 8, 9, 3), (4, 5, 6))
    with pytest.raises(ValueError, match="size must be"):
        GG.to_guidance(d(2, 8, 9, 3), 0)
    with pytest.raises(ValueError, match="size must be"):
        GG.resize(d(2, 8, 9, 3), (4, 2.5))
    with pytest.raises(ValueError, match="layout"):
        GG.to_guidance(d(2, 8, 9, 3), layout="CHW")
    with pytest.raises(NotImplementedError, match="float16 or float32"):
        GG.to_guidance(d(2, 8, 9, 3), dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="must be float32"):
        GG.to_guidance(d(2, 8, 9, 3).double())
    with pytest.raises(ValueError, match="empty"):
        GG.to_guidance(d(0, 8, 9, 3))
    with pytest.raises(ValueError, match="empty"):
        GG.to_guidance(d(2, 0, 9, 3))
    lat = d(2, 4, 8, 8)
    with pytest.raises(ValueError, match="no CPU implementation"):
        GG.sds_loss(lat, d(2, 4, 8, 8))
    with pytest.raises(ValueError, match="no CPU implementation"):
        GG.sds_loss(lat.clone().requires_grad_(True), d(2, 4, 8, 8), 1.0)
    with pytest.raises(ValueError, match=r"\[B, \.\.\.\]"):
        GG.sds_loss(d(8), d(8))
    with pytest.raises(ValueError, match=r"\[B, \.\.\.\]"):
        GG.sds_loss(lat, None)
    with pytest.raises(ValueError, match="differ in shape"):
        GG.sds_loss(lat, d(2, 4, 8, 7))
    with pytest.raises(ValueError, match="grad_clip_val"):
        GG.sds_loss(lat, d(2, 4, 8, 8), -1.0)
    with pytest.raises(ValueError, match="grad_clip_val"):
        GG.sds_loss(lat, d(2, 4, 8, 8), float("nan"))
    with pytest.raises(ValueError, match="empty"):
        GG.sds_loss(d(0, 4, 8, 8), d(0, 4, 8, 8))
    with pytest.raises(NotImplementedError, match="float32"):
        GG.sds_loss(lat.half(), d(2, 4, 8, 8).half())


def test_package_exports_the_guidance_names():
    import gsgen_amd
    from gsgen_amd import guidance as GG
    assert gsgen_amd.guidance is GG
    for name in ("to_guidance", "vae_input", "if_input", "rgb_as_latents", "sds_loss"):
        assert getattr(gsgen_amd, name) is getattr(GG, name)
    assert callable(GG.resize)
