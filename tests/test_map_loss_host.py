"""gsgen_amd/csrc/map_loss.hip on the CPU SIMT emulator (oracle/emu) against the torch restatement of tests/map_loss_cases.py, and the
argument checks of gsgen_amd.loss's map functions that need no GPU.  The file is compiled without contraction, so the emulated kernels
perform the GPU's operations in the GPU's order (logf is the platform's own on either side)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import map_loss_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSGEN_EINVAL, GSGEN_EWORKSPACE = -3, -4
ALL = 7


@pytest.fixture(scope="module")
def map_emu(tmp_path_factory):
    """map_loss.hip compiled with g++ on the emulator headers, with the flags tests/test_depth_loss_host.py uses (into tmp: nothing
    under oracle/ changes)"""
    out = tmp_path_factory.mktemp("map_loss_emu") / "libmap_loss_emu.so"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                           "-Wno-unknown-pragmas", "-DGSGEN_EMU_KNOBS=1", "-I", os.path.join(ROOT, "oracle", "emu"), "-x", "c++",
                           os.path.join(ROOT, "gsgen_amd", "csrc", "map_loss.hip"), "-o", str(out), "-lm"])
    lib = C.CDLL(str(out))
    u32, vp, i32, sz = C.c_uint32, C.c_void_p, C.c_int, C.c_size_t
    lib.gsgen_map_loss_workspace_bytes.argtypes = [u32]
    lib.gsgen_map_loss_workspace_bytes.restype = sz
    lib.gsgen_map_loss_forward.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp, sz, vp]
    lib.gsgen_map_loss_forward.restype = i32
    lib.gsgen_map_loss_backward.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.gsgen_map_loss_backward.restype = i32
    lib.gsgen_map_loss_emu_constants.argtypes = [vp]
    return lib


def ptr(a):
    return None if a is None else a.ctypes.data


def at_offset(a, k, fill=None):
    """-> a flat float32 array holding a's values (or `fill`) whose address is 4 k bytes past a 16-byte boundary"""
    n = a.size
    buf = np.empty(n + 8, np.float32)
    s = (k - (buf.ctypes.data // 4) % 4) % 4
    view = buf[s:s + n]
    assert view.ctypes.data % 16 == 4 * k
    view[:] = a.reshape(-1) if fill is None else fill
    return view


def run_map(lib, o, v, terms=ALL, weights=MC.W, dev_weights=False, scale=1.0, want=("o", "v"), offset=0):
    """-> (out float32 [4], grad_opacity or None, grad_z_var or None, in o's shape); want = (): the forward alone.  `weights` go in
    as the host's three floats, or (dev_weights) as float[3] "device" memory with the host's pointer null."""
    shape, P = o.shape, o.size
    o = at_offset(np.asarray(o, np.float32), offset)
    v = None if v is None else at_offset(np.asarray(v, np.float32), offset)
    w = np.array(weights, np.float32)
    wh, wd = (None, w) if dev_weights else (w, None)
    nbytes = lib.gsgen_map_loss_workspace_bytes(P)
    assert nbytes > 0
    wsb = np.full(nbytes + 3, 0xA5, np.uint8)[3:]  # (an unaligned, dirty base: the carve aligns it and nothing is assumed zero)
    out = np.full(4, 7.0, np.float32)
    rc = lib.gsgen_map_loss_forward(ptr(o), ptr(v), P, terms, ptr(wh), ptr(wd), ptr(out), ptr(wsb), wsb.size, None)
    assert rc == 0, rc
    if not want:
        return out, None, None
    go = at_offset(o, offset, fill=np.nan) if "o" in want else None
    gv = at_offset(o, offset, fill=np.nan) if "v" in want else None
    s = np.array([scale], np.float32)
    rc = lib.gsgen_map_loss_backward(ptr(o), ptr(v), P, terms, ptr(wh), ptr(wd), ptr(s), ptr(go), ptr(gv), ptr(wsb), wsb.size, None)
    assert rc == 0, rc
    return out, None if go is None else go.reshape(shape), None if gv is None else gv.reshape(shape)


def same(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_the_constants_the_cases_assume(map_emu):
    k = np.zeros(3, np.uint32)
    map_emu.gsgen_map_loss_emu_constants(k.ctypes.data)
    assert k[0] == MC.KCHUNK and k[1] == MC.KSWEEP
    size = lambda s: s[0] * s[1] * s[2]  # noqa: E731
    assert size(MC.S3) < 4 and -(-size(MC.S70) // 4) < 64 and size(MC.S70) % 4 != 0  # (less than one vector; less than a wave of them)
    assert size(MC.SONE) == MC.KCHUNK and size(MC.SONE1) == MC.KCHUNK + 1
    assert size(MC.S32000) > 2 * MC.KCHUNK and size(MC.S32000) % MC.KCHUNK != 0
    assert -(-size(MC.SSWEEP) // MC.KCHUNK) == MC.KSWEEP + 1


@pytest.mark.parametrize("name", MC.NAMES)
def test_emulated_map_loss_meets_the_restatements_own_error(map_emu, name):
    o, v = MC.inputs(name)
    out, go, gv = run_map(map_emu, o, v)
    MC.check_bound(name, out, go, gv)
    # the forward alone, and each gradient alone
    only, _, _ = run_map(map_emu, o, v, want=())
    assert only.tobytes() == out.tobytes()
    if o.size > 100 * MC.KCHUNK:
        return  # (the final stage's second sweep is the point of this size; the emulator takes a second per pass over it)
    _, go1, none = run_map(map_emu, o, v, want=("o",))
    assert none is None and go1.tobytes() == go.tobytes()
    _, none, gv1 = run_map(map_emu, o, v, want=("v",))
    assert none is None and gv1.tobytes() == gv.tobytes()
    # each term alone: its entry of the three-term run bit for bit, the others 0, and its own bound
    for k in range(3):
        w1 = tuple(1.0 if j == k else 0.0 for j in range(3))
        out1, go1, gv1 = run_map(map_emu, o, v if k == 2 else None, terms=1 << k, weights=w1)
        assert out1[1 + k].tobytes() == out[1 + k].tobytes() and out1[0].tobytes() == out[1 + k].tobytes(), k
        assert not out1[[1 + j for j in range(3) if j != k]].any()
        MC.check_bound(name, out1, go1, gv1, weights=w1)


@pytest.mark.parametrize("name", ["disc-1x160x200", "uniform-1x1x2049", "boundary-2x5x7"])
def test_device_weights_masked_terms_and_offset_bases_keep_the_bits(map_emu, name):
    o, v = MC.inputs(name)
    ref = run_map(map_emu, o, v)
    assert same(run_map(map_emu, o, v, dev_weights=True), ref)
    assert same(run_map(map_emu, o, v), ref)                          # two runs
    for k in (1, 2, 3):                                               # a base 4, 8 and 12 bytes past a 16-byte boundary
        assert same(run_map(map_emu, o, v, offset=k), ref), k
    # a masked-off term reports 0 and leaves the other terms' bits unchanged
    for off in range(3):
        terms = ALL & ~(1 << off)
        out, go, gv = run_map(map_emu, o, v if terms & 4 else None, terms=terms)
        assert out[1 + off] == 0.0
        for k in range(3):
            assert k == off or out[1 + k].tobytes() == ref[0][1 + k].tobytes()
        MC.check_bound(name, out, go, gv, weights=tuple(0.0 if k == off else w for k, w in enumerate(MC.W)))
        if off == 2:
            assert not gv.any()
    # device weights with a zero in them still evaluate the term: its entry stays
    out, _, _ = run_map(map_emu, o, v, weights=(0.5, 0.0, 2.0), dev_weights=True, want=())
    assert out[1:].tobytes() == ref[0][1:].tobytes()


def test_an_upstream_scalar_scales_the_gradients_exactly(map_emu):
    name = "disc-1x160x200"
    o, v = MC.inputs(name)
    out0, go0, gv0 = run_map(map_emu, o, v)
    out2, go2, gv2 = run_map(map_emu, o, v, scale=2.0)
    assert out2.tobytes() == out0.tobytes()
    assert go2.tobytes() == (2.0 * go0).astype(np.float32).tobytes() and gv2.tobytes() == (2.0 * gv0).astype(np.float32).tobytes()
    assert np.abs(go0).max() > 0 and np.abs(gv0).max() > 0
    out3, go3, gv3 = run_map(map_emu, o, v, scale=3.0)
    MC.check_bound(name, out3, go3, gv3, scale=3.0)


@pytest.mark.parametrize("name", [n for n in MC.NAMES if n.startswith("nan_")])
def test_a_nan_pixel_reaches_its_terms_and_no_other_pixels_gradient(map_emu, name):
    o, v = MC.inputs(name)
    out, go, gv = run_map(map_emu, o, v)
    if name.startswith("nan_o"):
        assert np.isnan(out).all()
    else:  # z_var's NaN sits under m == 0: the product with 0 is NaN, as in torch; the other two terms never read it
        assert np.isnan(out[0]) and np.isnan(out[3]) and np.isfinite(out[1]) and np.isfinite(out[2])
    co, cv = MC.clean_of(name)
    _, cgo, cgv = run_map(map_emu, co, cv)
    others = np.ones(o.size, bool)
    others[MC.NAN_AT] = False
    for a, b in ((go, cgo), (gv, cgv)):
        assert a.reshape(-1)[others].tobytes() == b.reshape(-1)[others].tobytes()
        assert np.isfinite(a.reshape(-1)[others]).all()


@pytest.mark.parametrize("name", ["boundary-2x5x7", "boundary-1x1x2049", "zeros-2x5x7", "ones-2x5x7"])
def test_the_clamp_and_the_threshold_are_decided_as_the_restatement_decides_them(map_emu, name):
    """the opague term's gradient is an exact zero exactly where `in` is false, the z_var term's two exactly where `in & m` and `m`
    are: at lo, hi and 0.5 and one ulp to either side this is the restatement's own zero pattern, and numpy's fp32 decision"""
    o, v = MC.inputs(name)
    inside, m = MC.masks(o)
    n = MC.BOUNDARY.size if name.startswith("boundary") else o.size
    if name.startswith("boundary"):
        assert inside.reshape(-1)[:n].tolist() == [False, True, True, True, True, False, True, True, True]
        assert m.reshape(-1)[:n].tolist() == [False, False, False, True, True, True, False, False, True]
    head = lambda a: np.asarray(a).reshape(-1)[:n]  # noqa: E731
    _, go_e, _ = run_map(map_emu, o, None, terms=2, weights=(0.0, 1.0, 0.0), want=("o",))
    _, go_z, gv_z = run_map(map_emu, o, v, terms=4, weights=(0.0, 0.0, 1.0))
    r_e, r_z = MC.reference(name, torch.float32, (0.0, 1.0, 0.0)), MC.reference(name, torch.float32, (0.0, 0.0, 1.0))
    edge = np.abs(head(o) - np.float32(0.5)) > 0.25  # (within an ulp of 0.5 the difference of the two logs may itself round to 0)
    assert ((head(go_e) != 0) == (head(r_e["go"]) != 0))[edge].all()
    assert ((head(go_z) != 0) == (head(r_z["go"]) != 0)).all() and ((head(gv_z) != 0) == (head(r_z["gv"]) != 0)).all()
    assert not head(go_e)[~head(inside)].any()
    assert (head(go_e)[head(inside) & edge] != 0).all()
    assert ((head(gv_z) != 0) == head(m)).all() and ((head(go_z) != 0) == head(inside & m)).all()
    if name.startswith(("zeros", "ones")):  # either side of the clamp: every gradient of the two clamped terms is an exact zero ...
        assert not go_e.any() and not go_z.any() and (gv_z != 0).all() == name.startswith("ones")
        _, go_s, _ = run_map(map_emu, o, None, terms=1, weights=(1.0, 0.0, 0.0), want=("o",))
        assert (go_s != 0).all() == name.startswith("ones")  # ... and the sparsity term's is o / s


def test_emulated_map_loss_argument_checks(map_emu):
    lib = map_emu
    P = 35
    o = np.random.default_rng(0).random(P).astype(np.float32)
    v = np.random.default_rng(1).random(P).astype(np.float32)
    out, go, gv, one = np.full(4, 7.0, np.float32), np.full(P, 7.0, np.float32), np.full(P, 7.0, np.float32), np.ones(1, np.float32)
    w = np.array(MC.W, np.float32)
    wsb = np.zeros(1 << 12, np.uint8)

    def fwd(P=P, o=o, v=v, terms=ALL, wh=w, wd=None, out=out, ws=wsb, nbytes=wsb.size):
        return lib.gsgen_map_loss_forward(ptr(o), ptr(v), P, terms, ptr(wh), ptr(wd), ptr(out), ptr(ws), nbytes, None)

    def bwd(P=P, o=o, v=v, terms=ALL, wh=w, wd=None, scale=one, ws=wsb, nbytes=wsb.size, go=go, gv=gv):
        return lib.gsgen_map_loss_backward(ptr(o), ptr(v), P, terms, ptr(wh), ptr(wd), ptr(scale), ptr(go), ptr(gv), ptr(ws), nbytes, None)
    for call in (fwd, bwd):
        assert call(P=0) == 0                                        # empty: clean, nothing written
        assert call(o=None) == GSGEN_EINVAL and call(ws=None) == GSGEN_EINVAL
        assert call(v=None) == GSGEN_EINVAL                          # the z_var term without z_var
        assert call(wh=None) == GSGEN_EINVAL                         # neither host nor device weights
        assert call(terms=8) == GSGEN_EINVAL
    assert fwd(out=None) == GSGEN_EINVAL
    assert bwd(scale=None) == GSGEN_EINVAL
    need = lib.gsgen_map_loss_workspace_bytes(P)
    assert 0 < need <= wsb.size
    assert need == lib.gsgen_map_loss_workspace_bytes(MC.KCHUNK) < lib.gsgen_map_loss_workspace_bytes(100 * MC.KCHUNK)
    assert fwd(nbytes=need - 1) == GSGEN_EWORKSPACE and bwd(nbytes=need - 1) == GSGEN_EWORKSPACE
    assert (out == 7.0).all() and (go == 7.0).all() and (gv == 7.0).all() and not wsb.any()  # a refused call enqueues nothing
    assert fwd(nbytes=need) == 0 and bwd(nbytes=need) == 0
    assert np.isfinite(out).all() and np.isfinite(go).all() and np.isfinite(gv).all() and (out != 7.0).all() and (go != 7.0).all()
    # without the z_var term z_var may be null; device weights stand in for the host's
    assert fwd(v=None, terms=3) == 0 and bwd(v=None, terms=3, gv=None) == 0
    assert fwd(wh=None, wd=w) == 0 and bwd(wh=None, wd=w) == 0
    go[:] = 7.0
    assert bwd(go=None, gv=None) == 0 and (go == 7.0).all()          # nothing asked


# --- gsgen_amd.loss: the refusals, which need neither a GPU nor the library ------------------------------------------------
def test_python_refusals():
    """every check comes before the device check, so CPU tensors reach each of them; a well-formed CPU call is refused last"""
    from gsgen_amd import loss as GL
    d = lambda *s, **k: torch.rand(*s, **k)  # noqa: E731
    for o, z in ((d(2, 8, 9, 1), d(2, 8, 9, 1)), (d(2, 8, 9), d(2, 8, 9)), (d(8, 9, 1), d(8, 9, 1)), (d(8, 9), d(8, 9)),
                 (d(2, 8, 9, 1, requires_grad=True), d(2, 8, 9, 1, requires_grad=True))):
        with pytest.raises(ValueError, match="no CPU implementation"):
            GL.map_loss(o, z, 1.0, 1.0, 1.0)
        with pytest.raises(ValueError, match="no CPU implementation"):
            GL.map_loss_terms(o, z, weights=torch.ones(3))
        with pytest.raises(ValueError, match="no CPU implementation"):
            GL.map_loss_terms(o, None, 1.0, 1.0)
        for fn in (GL.sparsity_loss, GL.opague_loss, lambda a: GL.z_var_loss(z, a)):
            with pytest.raises(ValueError, match="no CPU implementation"):
                fn(o)
        with pytest.raises(ValueError, match="no CPU implementation"):
            GL.get_map_loss({"sparsity": 1.0, "opague": [0, 1.0, 0.1, 100], "z_var": 0.0})({"opacity": o, "z_var": z}, 10)
    with pytest.raises(ValueError, match=r"\[B, H, W, 1\]"):
        GL.map_loss(d(9), None, 1.0)
    with pytest.raises(ValueError, match=r"\[B, H, W, 1\]"):
        GL.map_loss([1.0], None, 1.0)
    with pytest.raises(ValueError, match="one channel"):
        GL.map_loss(d(2, 8, 9, 3), None, 1.0)
    with pytest.raises(ValueError, match="differ in shape"):
        GL.map_loss(d(2, 8, 9, 1), d(2, 8, 8, 1), 1.0, 0.0, 1.0)
    with pytest.raises(ValueError, match="differ in shape"):
        GL.map_loss(d(2, 8, 9, 1), d(1, 8, 9, 1), 1.0)
    with pytest.raises(ValueError, match="should turn off the `rgb_only` flag"):
        GL.map_loss(d(2, 8, 9, 1), None, 1.0, 1.0, 0.5)
    with pytest.raises(ValueError, match="should turn off the `rgb_only` flag"):
        GL.get_map_loss({"sparsity": 1.0})({"rgb": d(2, 8, 9, 3)}, 0)
    with pytest.raises(ValueError, match=r"float32 \[3\]"):
        GL.map_loss(d(2, 8, 9, 1), None, weights=torch.ones(2))
    with pytest.raises(ValueError, match=r"float32 \[3\]"):
        GL.map_loss(d(2, 8, 9, 1), None, weights=[1.0, 1.0, 1.0])
    with pytest.raises(NotImplementedError, match="float32"):
        GL.map_loss(d(2, 8, 9, 1), None, weights=torch.ones(3, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="require a gradient"):
        GL.map_loss(d(2, 8, 9, 1), None, weights=torch.ones(3, requires_grad=True))
    with pytest.raises(ValueError, match="empty"):
        GL.map_loss(d(0, 8, 9, 1), None, 1.0)
    with pytest.raises(NotImplementedError, match="float32"):
        GL.map_loss(d(2, 8, 9, 1).double(), None, 1.0)
    with pytest.raises(NotImplementedError, match="float32"):
        GL.map_loss(d(2, 8, 9, 1), d(2, 8, 9, 1).half(), 0.0, 0.0, 1.0)
    # every weight 0: nothing to evaluate, and nothing asked of the dict
    total, terms = GL.get_map_loss({"sparsity": 0.0, "opague": 0.0})({"rgb": d(2, 8, 9, 3)}, 0)
    assert total.shape == () and float(total) == 0.0 and set(terms) == {"sparsity", "opague", "z_var"}


def test_package_exports_the_map_loss_names():
    import gsgen_amd
    from gsgen_amd import loss as GL
    for name in ("map_loss", "map_loss_terms", "sparsity_loss", "opague_loss", "z_var_loss", "get_map_loss"):
        assert getattr(gsgen_amd, name) is getattr(GL, name)
