"""gsgen_sh_view::pixel_size_dev on the CPU emulator: the batched SH launches that read their views' pixel sizes from "device" memory
(here: numpy) against the same launches with the pixel sizes in the view table -- the kernels' default instantiations.

Every comparison is bit for bit, gradients included: the emulator runs the workgroups of a launch one after another, so the order of
the atomic additions is that of the launch grid in both runs."""
import os
import subprocess

import numpy as np
import pytest

import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "emu"])
    from gsgen_amd import _capi
    return _capi.Lib(os.path.join(ROOT, "oracle", "_build", "libgsgen_emu.so"))


def P(a):
    return a.ctypes.data if a is not None else None


def _einval():
    """the value of GSGEN_EINVAL as the header states it"""
    import re
    txt = open(os.path.join(ROOT, "include", "gsgen_hip.h")).read()
    return int(re.search(r"#define\s+GSGEN_EINVAL\s+\(?(-?\d+)\)?", txt).group(1))


def _rc(fn, *args):
    """the C function's return code (the ctypes wrappers raise on a non-zero one and name it)"""
    import re
    from gsgen_amd._capi import GsgenError
    try:
        fn(*args)
    except GsgenError as e:
        return int(re.search(r"\(code (-?\d+)\)", str(e)).group(1))
    return 0


class Batch:
    """Two (or more) views of one scene as ONE view table, built once; run() launches forward and backward into fresh images and zeroed
    gradients.  device=True: the table carries pixel_size_dev -> self.pix [B,2] and NaN in the two floats."""

    def __init__(self, emu, sc, cams, device, nseg=0):
        from gsgen_amd._capi import ShView
        self.emu, self.C, self.nseg, self.B = emu, int(sc["C"]), nseg, len(cams)
        self.W, self.H = cams[0].w, cams[0].h
        self.nth, self.ntw = cams[0].tiles
        self.N = N = sc["mean"].shape[0]
        self.sh, self.al = np.ascontiguousarray(sc["sh"]), np.ascontiguousarray(sc["alpha"])
        T = self.nth * self.ntw
        H, W = self.H, self.W
        self.pix = np.array([[1 / c.fx, 1 / c.fy] for c in cams], np.float32)
        self.arr = (ShView * self.B)()
        self.keep = []
        for i, (a, cam) in enumerate(zip(self.arr, cams)):
            g = scenes.oracle_geometry(sc, cam)
            nz = np.nonzero(g["mask"])[0]
            m2 = np.zeros((N, 2), np.float32); c2 = np.zeros((N, 2, 2), np.float32)
            m2[nz] = g["mean2d"]; c2[nz] = g["cov2d"]
            v = dict(m2=m2, c2=c2, st=g["start"], en=g["end"], ids=nz[g["ids"]].astype(np.int32), tlp=cam.topleft,
                     rot=np.ascontiguousarray(cam.c2w[:3, :3].reshape(-1)), bg=np.array([0.3, 0.1, 0.2], np.float32),
                     go=np.random.default_rng(i).normal(size=(H, W, 3)).astype(np.float32),
                     ws=np.zeros(max(1, emu.segment_workspace_bytes(T, nseg)), np.uint8), out=np.empty((H, W, 3), np.float32),
                     T=np.empty((H, W), np.float32), gm=np.empty((N, 2), np.float32), gc=np.empty((N, 4), np.float32))
            self.keep.append(v)
            a.mean, a.cov, a.start, a.end, a.gaussian_ids = P(v["m2"]), P(v["c2"]), P(v["st"]), P(v["en"]), P(v["ids"])
            a.tile_order, a.topleft, a.c2w, a.bg_rgb = None, P(v["tlp"]), P(v["rot"]), P(v["bg"])
            a.out, a.T, a.segment_workspace = P(v["out"]), P(v["T"]), (P(v["ws"]) if nseg else None)
            a.grad_out, a.grad_mean, a.grad_cov = P(v["go"]), P(v["gm"]), P(v["gc"])
            if device:
                a.pixel_size_x = a.pixel_size_y = float("nan")  # ignored: a launch that read them would render NaN
                a.pixel_size_dev = self.pix.ctypes.data + 8 * i
            else:
                a.pixel_size_x, a.pixel_size_y = 1 / cam.fx, 1 / cam.fy
        self.bws = np.empty(emu.sh_batch_workspace_bytes_routed(self.B, T), np.uint8)

    def set_struct_pixel_sizes(self, pix):
        for a, (x, y) in zip(self.arr, pix):
            a.pixel_size_x, a.pixel_size_y = float(x), float(y)

    def run(self, bound=None, rows=None, moments=False, plain=False):
        """-> dict of copies: out [B,H,W,3], T, gm, gc, gsh, ga, flags"""
        emu, B, N, T = self.emu, self.B, self.N, self.nth * self.ntw
        for v in self.keep:
            v["out"].fill(9.0); v["T"].fill(9.0); v["gm"].fill(0.0); v["gc"].fill(0.0)
        self.bws.fill(7)
        geo = (16, self.nth, self.ntw, self.H, self.W, self.C, 1e-4, self.nseg)
        gsh = np.zeros_like(self.sh); ga = np.zeros(N, np.float32)
        if plain:  # the entry points without a bound
            rc = _rc(emu.vol_render_sh_batch, B, self.arr, N, P(self.sh), P(self.al), *geo, P(self.bws), None)
            rc_b = _rc(emu.vol_render_backward_sh_batch, B, self.arr, N, P(self.sh), P(self.al), P(gsh), P(ga), *geo, P(self.bws), None)
        else:
            rc = _rc(emu.vol_render_sh_batch_routed, B, self.arr, N, P(self.sh), P(self.al), *geo, P(bound), P(rows), P(self.bws), None)
            bwd = emu.vol_render_backward_sh_batch_routed_moments if moments else emu.vol_render_backward_sh_batch_routed
            rc_b = _rc(bwd, B, self.arr, N, P(self.sh), P(self.al), P(gsh), P(ga), *geo, P(bound), P(rows), P(self.bws), None)
        flags = self.bws[emu.sh_batch_workspace_bytes(B):][:B * T].reshape(B, T).copy()
        st = lambda k: np.stack([v[k] for v in self.keep]).copy()
        return dict(rc=(rc, rc_b), out=st("out"), T=st("T"), gm=st("gm"), gc=st("gc"), gsh=gsh, ga=ga, flags=flags)


def _same(a, b):
    for k in ("out", "T", "gm", "gc", "gsh", "ga", "flags"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert not np.isnan(a["out"]).any() and not np.isnan(a["gsh"]).any()


def _cams(W, H, fxs):
    return [scenes.Camera(W, H, fx=fx, c2w=scenes.orbit(2.5, 10 + 20 * i, 40.0 + 100 * i)) for i, fx in enumerate(fxs)]


def _run_pair(emu, sc, cams, nseg=0, **kw):
    """the struct-float launch and the pixel_size_dev launch agree bit for bit; then the property a replay of a captured step relies on:
    the device floats rewritten to the OTHER view's focal length, the same view table launched again == that pixel size's struct-float
    launch (the lists stay those of the table: compositing reads the pixel size only for the pixel coordinates and the routing rule)"""
    ref, dev = Batch(emu, sc, cams, False, nseg), Batch(emu, sc, cams, True, nseg)
    a, b = ref.run(**kw), dev.run(**kw)
    assert a["rc"] == (0, 0) and b["rc"] == (0, 0)
    _same(a, b)
    swapped = dev.pix[::-1].copy()
    assert not np.array_equal(swapped, dev.pix)
    dev.pix[:] = swapped             # (in place: the table keeps pointing at these floats)
    ref.set_struct_pixel_sizes(swapped)
    a2, b2 = ref.run(**kw), dev.run(**kw)
    _same(a2, b2)
    assert np.abs(a2["out"] - a["out"]).mean() > 1e-3  # ... and the other focal lengths do render another image
    return a, a2


@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("nseg", [0, 2])
def test_plain_batch_reads_pixel_sizes_from_device_memory(emu, C, nseg):
    sc = scenes.random_scene(300, seed=5 + C, svec=0.05, spread=0.25, C=C)
    _run_pair(emu, sc, _cams(64, 48, (130.0, 175.0)), nseg=nseg, plain=True)


def _routed_scene(outliers):
    """the scene of test_emulated_polynomial_sh_basis_is_routed_per_tile: a bulk within every view's bound and (outliers) a cluster of
    splats far beyond it, which sends its tiles to the exact fallback"""
    C = 4
    sc = scenes.random_scene(300, seed=23, svec=0.048, spread=0.18, C=C)
    sc["sh"][:, :, 1:] *= 0.0078
    sc["alpha"] = (sc["alpha"] * 0.5).astype(np.float32)
    if outliers:
        rng = np.random.default_rng(4)
        centre = sc["mean"][int(rng.integers(300))]
        outl = np.argsort(np.linalg.norm(sc["mean"] - centre, axis=1))[:10]
        sc["sh"][outl, :, 9:] = 3.0
        sc["sh"][outl, :, 0] = 0.0
    return sc


@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("outliers", [False, True])
def test_routed_batch_reads_pixel_sizes_from_device_memory(emu, outliers, moments):
    """per-tile routing on the per-splat bounds (+ the scene's maximum, as BatchRenderer passes both): every tile polynomial, or a
    crowded tile handed to the persistent exact fallback; plain and moment-form backward"""
    sc = _routed_scene(outliers)
    N = sc["mean"].shape[0]
    sh = np.ascontiguousarray(sc["sh"])
    rows = np.zeros(N, np.float32); gmax = np.zeros(1, np.float32)
    emu.sh_l1_bound_rows(N, P(sh), 4, P(gmax), P(rows), None)
    a, a2 = _run_pair(emu, sc, _cams(64, 48, (130.0, 145.0)), bound=gmax, rows=rows, moments=moments)
    for r in (a, a2):
        assert set(np.unique(r["flags"])) <= {0, 1}
        assert bool(r["flags"].any()) == outliers   # (the exact fallback rendered tiles -- or none was handed over)
    # the routing really ran: the same launch on the exact kernels alone leaves other bits
    exact = Batch(emu, sc, _cams(64, 48, (130.0, 145.0)), True).run(moments=moments)
    assert np.abs(exact["out"] - a["out"]).max() > 0 and np.abs(exact["out"] - a["out"]).max() <= 1e-5


def test_per_view_routing_on_the_device_decides_from_the_loaded_pixel_sizes(emu):
    """one device-resident bound, no per-splat rows: the narrow view is the polynomial kernel's, the wide one the persistent fallback's
    -- with the pixel sizes in device memory the host cannot take its "no view can be polynomial" shortcut, and after the swap the two
    views change roles without a new table"""
    sc = _routed_scene(False)
    sh = np.ascontiguousarray(sc["sh"])
    gmax = np.zeros(1, np.float32)
    emu.sh_l1_bound(sc["mean"].shape[0], P(sh), 4, P(gmax), None)
    cams = _cams(64, 48, (560.0, 40.0))
    assert emu.sh_poly_applies(float(gmax[0]), 1 / 560.0, 4) and not emu.sh_poly_applies(float(gmax[0]), 1 / 40.0, 4)
    _run_pair(emu, sc, cams, bound=gmax)
    # both views too wide for any bound: the struct-float launch takes the host's shortcut (exact kernels alone), the device launch
    # cannot -- the same bits all the same
    _run_pair(emu, sc, _cams(64, 48, (20.0, 24.0)), bound=gmax)


def test_mixed_set_and_unset_pointers_are_rejected(emu):
    sc = scenes.random_scene(120, seed=2, svec=0.05, spread=0.25, C=4)
    b = Batch(emu, sc, _cams(64, 48, (130.0, 175.0)), True)
    b.arr[1].pixel_size_dev = None
    b.arr[1].pixel_size_x, b.arr[1].pixel_size_y = 1 / 175.0, 1 / 175.0
    for kw in (dict(plain=True), dict(), dict(moments=True)):
        r = b.run(**kw)
        assert r["rc"] == (_einval(), _einval())
        assert (r["out"] == 9.0).all() and (r["T"] == 9.0).all() and not r["gsh"].any()  # nothing was launched
