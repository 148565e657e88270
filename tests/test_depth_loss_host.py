"""gsgen_amd/csrc/depth_loss.hip on the CPU SIMT emulator (oracle/emu) against the torch restatement of tests/depth_loss_cases.py,
and the argument checks of gsgen_amd.loss's depth functions that need no GPU.  The file is compiled without contraction, so the
emulated kernels perform the GPU's operations in the GPU's order: the errors printed here are the GPU's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import depth_loss_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSGEN_EUNSUPPORTED, GSGEN_EINVAL, GSGEN_EWORKSPACE = -2, -3, -4


@pytest.fixture(scope="module")
def depth_emu(tmp_path_factory):
    """depth_loss.hip compiled with g++ on the emulator headers, with the flags tests/test_loss_host.py uses (into tmp: nothing under
    oracle/ changes)"""
    out = tmp_path_factory.mktemp("depth_loss_emu") / "libdepth_loss_emu.so"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                           "-Wno-unknown-pragmas", "-DGSGEN_EMU_KNOBS=1", "-I", os.path.join(ROOT, "oracle", "emu"), "-x", "c++",
                           os.path.join(ROOT, "gsgen_amd", "csrc", "depth_loss.hip"), "-o", str(out), "-lm"])
    lib = C.CDLL(str(out))
    u32, vp, i32, sz = C.c_uint32, C.c_void_p, C.c_int, C.c_size_t
    lib.gsgen_depth_loss_workspace_bytes.argtypes = [u32, u32]
    lib.gsgen_depth_loss_workspace_bytes.restype = sz
    lib.gsgen_depth_loss_forward.argtypes = [vp, vp, sz, vp, sz, u32, u32, vp, vp, sz, vp]
    lib.gsgen_depth_loss_forward.restype = i32
    lib.gsgen_depth_loss_backward.argtypes = [vp, vp, sz, vp, sz, u32, u32, vp, vp, vp, vp, sz, vp]
    lib.gsgen_depth_loss_backward.restype = i32
    lib.gsgen_depth_loss_emu_constants.argtypes = [vp]
    return lib


def ptr(a):
    return None if a is None else a.ctypes.data


def run_depth(lib, pred, gt, mask=None, scale=1.0, want=("pred", "gt")):
    """pred [B,H,W], gt [B,H,W] or [1,H,W] (shared by an image stride of 0), mask bool [B,H,W] or [1,H,W] or None
    -> (loss_out float32 [1 + B], grad_pred or None, grad_gt or None); want = (): the forward alone"""
    pred, gt = np.ascontiguousarray(pred, np.float32), np.ascontiguousarray(gt, np.float32)
    B, P = pred.shape[0], pred.shape[1] * pred.shape[2]
    m8 = None if mask is None else np.ascontiguousarray(mask).astype(np.uint8)
    gstride = P if gt.shape[0] == B else 0
    mstride = 0 if m8 is None or m8.shape[0] != B else P
    nbytes = lib.gsgen_depth_loss_workspace_bytes(B, P)
    assert nbytes > 0
    wsb = np.full(nbytes + 3, 0xA5, np.uint8)[3:]  # (an unaligned, dirty base: the carve aligns it and nothing is assumed zero)
    loss = np.full(1 + B, 7.0, np.float32)
    rc = lib.gsgen_depth_loss_forward(ptr(pred), ptr(gt), gstride, ptr(m8), mstride, B, P, ptr(loss), ptr(wsb), wsb.size, None)
    assert rc == 0, rc
    if not want:
        return loss, None, None
    gp = np.full(pred.shape, np.nan, np.float32) if "pred" in want else None
    gg = np.full(gt.shape, np.nan, np.float32) if "gt" in want else None
    s = np.array([scale], np.float32)
    rc = lib.gsgen_depth_loss_backward(ptr(pred), ptr(gt), gstride, ptr(m8), mstride, B, P, ptr(s), ptr(gp), ptr(gg), ptr(wsb), wsb.size, None)
    assert rc == 0, rc
    return loss, gp, gg


def run_case(lib, name, scale=1.0):
    """-> (loss_out, grad_pred, grad_gt in the shape of the case's gt).  A shared gt takes its gradient as gsgen_amd.loss does it:
    from a run on the materialised repeat, summed over the batch in fp32; that run's forward must equal the strided one's bit
    for bit."""
    c = DC.case(name)
    B = c["pred"].shape[0]
    if c["gt"].shape[0] == B:
        return run_depth(lib, c["pred"], c["gt"], c["mask"], scale)
    loss, gp, _ = run_depth(lib, c["pred"], c["gt"], c["mask"], scale, want=("pred",))
    loss_r, gp_r, gg_r = run_depth(lib, c["pred"], np.repeat(c["gt"], B, axis=0), c["mask"], scale)
    assert loss_r.tobytes() == loss.tobytes() and gp_r.tobytes() == gp.tobytes()
    return loss, gp, torch.as_tensor(gg_r).sum(0, keepdim=True).numpy()


def test_the_chunk_the_cases_assume(depth_emu):
    k = np.zeros(4, np.uint32)
    depth_emu.gsgen_depth_loss_emu_constants(k.ctypes.data)
    assert k[0] == DC.KCHUNK and 160 * 200 > 2 * DC.KCHUNK and 64 * 64 == DC.KCHUNK


@pytest.mark.parametrize("name", DC.NAMES)
def test_emulated_depth_loss_meets_the_restatements_own_error(depth_emu, name):
    c = DC.case(name)
    loss, gp, gg = run_case(depth_emu, name)
    DC.check_bound(name, loss[0], gp, gg)
    DC.check_corr(name, loss[1:])
    # the forward alone, and each gradient alone
    only, _, _ = run_depth(depth_emu, c["pred"], c["gt"], c["mask"], want=())
    assert only.tobytes() == loss.tobytes()
    _, gp1, none = run_depth(depth_emu, c["pred"], c["gt"], c["mask"], want=("pred",))
    assert none is None and gp1.tobytes() == gp.tobytes()
    if c["gt"].shape[0] == c["pred"].shape[0]:
        _, none, gg1 = run_depth(depth_emu, c["pred"], c["gt"], c["mask"], want=("gt",))
        assert none is None and gg1.tobytes() == gg.tobytes()
    # outside the mask both gradients are exact zeros
    if c["mask"] is not None:
        out = ~np.broadcast_to(c["mask"], c["pred"].shape)
        assert not gp[out].any()
        if gg.shape == gp.shape:
            assert not gg[out].any()


@pytest.mark.parametrize("name", [n for n in DC.NAMES if np.isnan(DC.case(n)["c64"]).any()])
def test_a_degenerate_image_contributes_exactly_one_and_exact_zeros(depth_emu, name):
    c = DC.case(name)
    loss, gp, gg = run_case(depth_emu, name)
    dead = np.isnan(c["c64"])
    assert (np.isnan(loss[1:]) == dead).all()
    assert not gp[dead].any()
    if gg.shape == gp.shape:
        assert not gg[dead].any()
    if dead.all():
        assert loss[0] == 1.0 and not gg.any()
    else:  # the loss is the mean of 1 for the dead images and 1 - r for the others, from the reported r
        B = dead.size
        want = (dead.sum() + (1.0 - loss[1:][~dead].astype(np.float64)).sum()) / B
        assert abs(float(loss[0]) - want) <= 2.0 ** -23


def test_degenerate_kinds_named_one_by_one(depth_emu):
    """n = 0, n = 1, constant pred 0.9f at several P, constant gt, all-NaN and all +Inf pred: each is degenerate exactly"""
    rng = np.random.default_rng(3)
    for P in (2, 63, 4096, 4097, 3 * 4096 + 5):
        y = rng.random((1, 1, P)).astype(np.float32)
        for x in (np.full((1, 1, P), 0.9, np.float32), np.full((1, 1, P), np.nan, np.float32), np.full((1, 1, P), np.inf, np.float32)):
            loss, gp, gg = run_depth(depth_emu, x, y)
            assert loss[0] == 1.0 and np.isnan(loss[1]) and not gp.any() and not gg.any(), (P, x[0, 0, 0])
        loss, gp, gg = run_depth(depth_emu, y, np.full((1, 1, P), 0.9, np.float32))
        assert loss[0] == 1.0 and np.isnan(loss[1]) and not gp.any() and not gg.any(), P
        # one value differs by an ulp, in the last workgroup: not degenerate
        x = np.full((1, 1, P), 0.9, np.float32)
        x[0, 0, P - 1] = np.nextafter(np.float32(0.9), np.float32(1))
        loss, _, _ = run_depth(depth_emu, x, y)
        assert not np.isnan(loss[1]), P
    x, y = rng.random((1, 5, 7)).astype(np.float32), rng.random((1, 5, 7)).astype(np.float32)
    for n_true in (0, 1):
        m = np.zeros((1, 5, 7), bool)
        m.reshape(-1)[3:3 + n_true] = True
        loss, gp, gg = run_depth(depth_emu, x, y, m)
        assert loss[0] == 1.0 and np.isnan(loss[1]) and not gp.any() and not gg.any()


def test_exact_two_pixel_correlations(depth_emu):
    for name, r in (("exact2-1x1x2-none", 1.0), ("exact2anti-1x1x2-none", -1.0)):
        loss, gp, gg = run_case(depth_emu, name)
        assert loss[1] == r and loss[0] == 1.0 - r and not gp.any() and not gg.any()


def test_infinities_in_pred_are_clamped_and_take_no_gradient(depth_emu):
    c = DC.case("affine-2x37x53-rand70")
    pred = c["pred"].copy()
    m = c["mask"]
    at = np.argwhere(m)[[5, 40, 900]]
    pred[tuple(at[0])], pred[tuple(at[1])], pred[tuple(at[2])] = np.inf, -np.inf, np.inf
    loss, gp, gg = run_depth(depth_emu, pred, c["gt"], m)
    assert np.isfinite(loss).all() and 0.0 <= loss[0] <= 2.0
    assert np.isfinite(gp).all() and np.isfinite(gg).all()
    for a in at:
        assert gp[tuple(a)] == 0.0
    # an infinity outside the mask changes nothing
    pred2 = c["pred"].copy()
    pred2[tuple(np.argwhere(~m)[7])] = np.inf
    a, b = run_depth(depth_emu, pred2, c["gt"], m), run_depth(depth_emu, c["pred"], c["gt"], m)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


def test_a_nan_in_gt_under_the_mask_makes_the_loss_nan(depth_emu):
    c = DC.case("affine-2x37x53-rand70")
    m = c["mask"]
    gt = c["gt"].copy()
    gt[tuple(np.argwhere(m)[11])] = np.nan  # (image 0)
    loss, _, _ = run_depth(depth_emu, c["pred"], gt, m)
    assert np.isnan(loss[0]) and np.isnan(loss[1]) and np.isfinite(loss[2])
    gt = c["gt"].copy()
    gt[tuple(np.argwhere(~m)[11])] = np.nan  # outside the mask: not read into any sum
    loss, _, _ = run_depth(depth_emu, c["pred"], gt, m)
    assert np.isfinite(loss).all()
    # a constant gt with one NaN is not "all equal"
    gt = np.full(c["gt"].shape, 2.5, np.float32)
    gt[0, 3, 3] = np.nan
    loss, _, _ = run_depth(depth_emu, c["pred"], gt)
    assert np.isnan(loss[0]) and np.isnan(loss[1]) and loss[2] != loss[2]  # (image 1 is constant: degenerate, reported NaN too)
    assert np.isnan(run_depth(depth_emu, c["pred"][:1], gt[:1])[0][0])


def test_bit_identical_from_run_to_run_and_the_upstream_scalar(depth_emu):
    name = "offset100-3x64x64-rand70"
    l0, p0, g0 = run_case(depth_emu, name)
    l1, p1, g1 = run_case(depth_emu, name)
    assert l0.tobytes() == l1.tobytes() and p0.tobytes() == p1.tobytes() and g0.tobytes() == g1.tobytes()
    l3, p3, g3 = run_case(depth_emu, name, scale=3.0)
    assert l3.tobytes() == l0.tobytes()
    DC.check_bound(name, l3[0], p3, g3, scale=3.0)
    _, p2, g2 = run_case(depth_emu, name, scale=2.0)
    assert p2.tobytes() == (2.0 * p0).astype(np.float32).tobytes() and g2.tobytes() == (2.0 * g0).astype(np.float32).tobytes()


def test_the_naive_one_pass_form_misses_the_bound_the_kernel_meets():
    """the trap the kernel avoids: sum x^2 - (sum x)^2 / n in fp32 on the offset-100 case (so the bound can tell the two apart)"""
    name = "offset100-2x37x53-none"
    c = DC.case(name)
    x, y = torch.as_tensor(c["pred"].copy()).reshape(2, -1), torch.as_tensor(c["gt"].copy()).reshape(2, -1)
    n = x.shape[1]
    sxx, syy = (x * x).sum(1) - x.sum(1) ** 2 / n, (y * y).sum(1) - y.sum(1) ** 2 / n
    sxy = (x * y).sum(1) - x.sum(1) * y.sum(1) / n
    naive = float((1 - sxy / torch.sqrt(sxx * syy)).mean())
    rows, _ = DC.bound_report(name, naive)
    assert rows[0][1] > rows[0][2]


def test_emulated_depth_loss_argument_checks(depth_emu):
    lib = depth_emu
    B, P = 2, 35
    x = np.random.default_rng(0).random((B, P)).astype(np.float32)
    y = np.random.default_rng(1).random((B, P)).astype(np.float32)
    m = np.ones((B, P), np.uint8)
    loss, gp, gg, one = np.full(1 + B, 7.0, np.float32), np.full(x.shape, 7.0, np.float32), np.full(x.shape, 7.0, np.float32), np.ones(1, np.float32)
    wsb = np.zeros(1 << 16, np.uint8)

    def fwd(B=B, P=P, pred=x, gt=y, out=loss, ws=wsb, nbytes=wsb.size):
        return lib.gsgen_depth_loss_forward(ptr(pred), ptr(gt), P, ptr(m), P, B, P, ptr(out), ptr(ws), nbytes, None)

    def bwd(B=B, P=P, pred=x, gt=y, scale=one, ws=wsb, nbytes=wsb.size, gstride=None, g_gt=gg):
        return lib.gsgen_depth_loss_backward(ptr(pred), ptr(gt), P if gstride is None else gstride, ptr(m), P, B, P, ptr(scale), ptr(gp),
                                             ptr(g_gt), ptr(ws), nbytes, None)
    for call in (fwd, bwd):
        assert call(B=0) == 0 and call(P=0) == 0                # empty: clean, nothing written
        assert call(B=70000) == GSGEN_EUNSUPPORTED
        assert call(pred=None) == GSGEN_EINVAL and call(gt=None) == GSGEN_EINVAL and call(ws=None) == GSGEN_EINVAL
    assert fwd(out=None) == GSGEN_EINVAL
    assert bwd(scale=None) == GSGEN_EINVAL
    assert bwd(gstride=0) == GSGEN_EINVAL                       # B images' gradients onto one gt
    assert lib.gsgen_depth_loss_workspace_bytes(70000, P) == 0
    need = lib.gsgen_depth_loss_workspace_bytes(B, P)
    assert 0 < need <= wsb.size
    assert need < lib.gsgen_depth_loss_workspace_bytes(B, 3 * DC.KCHUNK) < lib.gsgen_depth_loss_workspace_bytes(2 * B, 3 * DC.KCHUNK)
    assert fwd(nbytes=need - 1) == GSGEN_EWORKSPACE and bwd(nbytes=need - 1) == GSGEN_EWORKSPACE
    assert (loss == 7.0).all() and (gp == 7.0).all() and (gg == 7.0).all() and not wsb.any()  # a refused call enqueues nothing
    assert fwd(nbytes=need) == 0 and bwd(nbytes=need) == 0
    assert np.isfinite(loss).all() and np.isfinite(gp).all() and np.isfinite(gg).all() and (loss != 7.0).all()
    # a shared gt is fine for the forward, for the gradient to pred, and for its own gradient in a batch of one
    assert lib.gsgen_depth_loss_forward(ptr(x), ptr(y), 0, None, 0, B, P, ptr(loss), ptr(wsb), wsb.size, None) == 0
    assert bwd(gstride=0, g_gt=None) == 0
    gp[:] = 7.0
    assert lib.gsgen_depth_loss_backward(ptr(x), ptr(y), 0, None, 0, B, P, ptr(one), None, None, ptr(wsb), wsb.size, None) == 0  # nothing asked
    assert (gp == 7.0).all()
    assert lib.gsgen_depth_loss_forward(ptr(x), ptr(y), 0, None, 0, 1, P, ptr(loss), ptr(wsb), wsb.size, None) == 0
    assert lib.gsgen_depth_loss_backward(ptr(x), ptr(y), 0, None, 0, 1, P, ptr(one), ptr(gp), ptr(gg), ptr(wsb), wsb.size, None) == 0


# --- gsgen_amd.loss: the refusals, which need neither a GPU nor the library ------------------------------------------------
def test_python_refusals():
    """every check comes before the device check, so CPU tensors reach each of them; a well-formed CPU call is refused last"""
    from gsgen_amd import loss as GL
    d = lambda *s, **k: torch.rand(*s, **k)  # noqa: E731
    for pred, gt, mask in ((d(2, 8, 9, 1), d(2, 8, 9, 1), None), (d(2, 8, 9), d(8, 9), None), (d(8, 9, 1), d(8, 9, 1), torch.ones(8, 9, dtype=torch.bool)),
                           (d(2, 8, 9, 1, requires_grad=True), d(1, 8, 9, 1, requires_grad=True), torch.ones(2, 8, 9, dtype=torch.uint8)),
                           (d(8, 9), d(8, 9), torch.ones(1, 8, 9, dtype=torch.bool))):
        with pytest.raises(ValueError, match="no CPU implementation"):
            GL.pearson_depth_loss(pred, gt, mask)
        with pytest.raises(ValueError, match="no CPU implementation"):
            GL.depth_loss(None, pred, gt, mask)
        with pytest.raises(ValueError, match="no CPU implementation"):
            GL.pearson_depth_loss_terms(pred, gt, mask)
    with pytest.raises(ValueError, match=r"\[B, H, W, 1\]"):
        GL.pearson_depth_loss(d(9), d(9))
    with pytest.raises(ValueError, match=r"\[B, H, W, 1\]"):
        GL.pearson_depth_loss(d(2, 8, 9, 1), [1.0])
    with pytest.raises(ValueError, match="one channel"):
        GL.pearson_depth_loss(d(2, 8, 9, 3), d(2, 8, 9, 3))
    with pytest.raises(ValueError, match="differ in shape"):
        GL.pearson_depth_loss(d(2, 8, 9, 1), d(2, 8, 8, 1))
    with pytest.raises(ValueError, match="differ in shape"):
        GL.pearson_depth_loss(d(4, 8, 9, 1), d(2, 8, 9, 1))
    with pytest.raises(ValueError, match="differ in shape"):
        GL.pearson_depth_loss(d(8, 9), d(2, 8, 9))  # (a batched gt against one pred image)
    with pytest.raises(ValueError, match="mask must be"):
        GL.pearson_depth_loss(d(2, 8, 9, 1), d(2, 8, 9, 1), torch.ones(2, 8, 9, 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="does not fit"):
        GL.pearson_depth_loss(d(2, 8, 9, 1), d(2, 8, 9, 1), torch.ones(2, 9, 8, dtype=torch.bool))
    with pytest.raises(ValueError, match="does not fit"):
        GL.pearson_depth_loss(d(4, 8, 9, 1), d(4, 8, 9, 1), torch.ones(2, 8, 9, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="bool or uint8"):
        GL.pearson_depth_loss(d(2, 8, 9, 1), d(2, 8, 9, 1), torch.ones(2, 8, 9))
    with pytest.raises(ValueError, match="empty"):
        GL.pearson_depth_loss(d(0, 8, 9, 1), d(0, 8, 9, 1))
    with pytest.raises(ValueError, match="empty"):
        GL.pearson_depth_loss(d(2, 0, 9), d(2, 0, 9))
    with pytest.raises(NotImplementedError, match="float32"):
        GL.pearson_depth_loss(d(2, 8, 9, 1).double(), d(2, 8, 9, 1))
    with pytest.raises(NotImplementedError, match="float32"):
        GL.depth_loss(None, d(2, 8, 9, 1), d(2, 8, 9, 1).half())


def test_package_exports_the_depth_loss_names():
    import gsgen_amd
    from gsgen_amd import loss as GL
    for name in ("depth_loss", "pearson_depth_loss", "pearson_depth_loss_terms"):
        assert getattr(gsgen_amd, name) is getattr(GL, name)
