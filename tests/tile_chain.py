"""The per-camera chain of `_gs` entry points at a caller-chosen tile size (any side from 1 to 32), against the oracle at that tile size.
Shared by the emulator test (tests/test_cpu_host.py) and the GPU test (tests/test_gpu_parity.py): `L` provides
`lib` (the ctypes binding), `stream`, and `to_dev(array)` -> object with `.p` (address), `.n` (elements), `.get()`."""
import numpy as np
import pytest

import scenes
from oracle import oracle as O


FUZZ_ATOL = 2e-5
# (ts, C, W, H, n, seed, svec, opaque): examples 1 500-example hunts on the MI355X found beyond rtol 1e-3 + 1e-6 (round 5: 8.7e-6) and
# beyond rtol 1e-3 + 1e-5 (round 6: a 194 x 1 image of 2 002 opaque image-sized splats, SH degree 3 -- d cov2d 1.12e-5 beyond the
# relative part, every run alike; 2.3e-6 on the emulator, whose exp and reciprocal are exact where the GPU's are 1 ulp off)
KNOWN_WORST = [(8, 1, 10, 35, 1258, 2, 0.2, True), (8, 4, 194, 1, 2002, 4518, 0.2, True)]


def other_tile_size_chain(L, ts, C, W, H, sync=lambda: None, rtol=1e-4, n=300, seed=None, svec=0.07, opaque=False, atol=0.0, ftol=1e-5):
    """count -> bin / sort -> RGB, scalar and SH forward + backward at tile size `ts` through the library `L`
    against the oracle at the same tile size.  Shared by the emulator and the GPU tests.  n / seed / svec: the random
    scene; opaque: every opacity at 0.999 (above the 0.99 clamp: lists end early, T crosses the stop threshold).
    Gradients: |got - want| <= rtol * max|want| + atol.  atol, for the fuzz, covers the suffix behind near-opaque layers: the
    kernels keep one grad_out-weighted running suffix per pixel, whose rounding residue (fp32 epsilon 6e-8 x the largest
    |sum_c grad_out_c (final_c - prefix_c)| of the walk: an O(1) colour, up to ~3 behind a degree-3 SH sum, more with the depth
    heads) is multiplied by 1 / (1 - a G), up to 100 at the 0.99 clamp, in d L / d (a G).  FUZZ_ATOL = 2e-5 is that term for ONE
    pixel; long random hunts -- 1 500 examples per fuzz, rounds 5 and 6 -- found tiny-gradient scenes where 1e-6 was exceeded by
    exactly it, 8.7e-6 and 1.12e-5 at most: KNOWN_WORST above, rerun by every suite.  It is NOT a floor that every correct fp32
    backward shares: the reference replays the forward's accumulation per channel, so its final_c - prefix_c cancels exactly
    behind the last contributing entry and it has no such term.  On a full 16 x 16 tile behind two taken layers of a = 0.99 the
    kernels' alpha gradient of those layers misses the per-Gaussian bar (rtol 1e-3 of the row, atol 1e-5 of the tensor) by up
    to 2.8 x where the oracle's fp32 chain uses 0.01 of it -- 40 to 280 times tighter; the sum over 256 pixels stays at 0.06 of
    rtol 1e-3 x max|want| + FUZZ_ATOL (tests/chan_cases.py `behind_opaque`; DESIGN.md section 4, "The single suffix behind
    near-opaque layers", has the figures per tensor).
    ftol: forward tolerance (1e-5 on the fixed scenes; the fuzz takes north_star's 1e-4: a transmittance within rounding
    of the stop threshold lets one side composite one splat more, which weighs up to 1e-4).  When the ORACLE's own
    decision margins say that an SH pixel sits within a few ulps of a threshold (oracle.sh_decision_margin), the SH
    gradients of that example are not compared: the flipped splat moves them by up to 1e-4 of an O(1) term.
    (The fuzz keeps svec <= 0.2: with image-sized splats -- svec 0.6 -- the covariance gradient is a heavily cancelling sum
    over every pixel and fp32 atomics against the oracle's fp64 sums reach 1.1e-3 of its largest entry.)"""
    cam = scenes.Camera(W, H, fx=float(max(W, 4)))
    sc = scenes.random_scene(n, seed=C + ts if seed is None else seed, svec=svec, C=C)
    if opaque:
        sc["alpha"][:] = 0.999
    normals, pts = O.frustum(cam.c2w, *cam.intr)
    m = O.cull_bsphere(sc["mean"], sc["svec"], normals, pts, 6.0)
    N = int(m.sum())
    if N == 0:
        return
    m2, c2, _, dep = O.project(sc["mean"][m], sc["qvec"][m], sc["svec"][m], cam.c2w)
    D, otl, obr = O.aabb_count(m2, c2, ts, cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h, 6.0)
    nth, ntw = (H + ts - 1) // ts, (W + ts - 1) // ts
    oids, ost, oen = O.bin_sort(otl, obr, dep, nth, ntw, D)
    c2f = np.ascontiguousarray(c2.reshape(-1, 4))
    tl = np.zeros((N, 2), np.int32); br = np.zeros((N, 2), np.int32); tot = np.zeros(1, np.uint32)
    h = {k: v for k, v in dict(m2=m2, c2=c2f, dep=dep, tl=tl, br=br, tot=tot).items()}
    h = {k: L.to_dev(v) for k, v in h.items()}
    L.lib.tile_culling_aabb_count(N, h["m2"].p, h["c2"].p, ts, cam.fx, cam.fy, cam.cx, cam.cy, cam.w, cam.h, 6.0, h["tl"].p,
                                  h["br"].p, h["tot"].p, L.stream)
    sync()
    assert int(h["tot"].get()[0]) == D and np.array_equal(h["tl"].get(), otl) and np.array_equal(h["br"].get(), obr)
    ws = L.to_dev(np.zeros(L.lib.tile_culling_workspace_bytes(N, D, nth * ntw), np.uint8))
    ids = L.to_dev(np.zeros(D, np.int32)); st = L.to_dev(-np.ones(nth * ntw, np.int32)); en = L.to_dev(-np.ones(nth * ntw, np.int32))
    L.lib.tile_culling_aabb_start_end(N, D, nth, ntw, h["tl"].p, h["br"].p, h["dep"].p, ids.p, st.p, en.p, ws.p, ws.n, L.stream)
    sync()
    assert np.array_equal(st.get(), ost) and np.array_equal(en.get(), oen) and np.array_equal(ids.get(), oids)
    col = np.ascontiguousarray(sc["color"][m]); al = np.ascontiguousarray(sc["alpha"][m])
    tlp = cam.topleft; psx, psy = 1 / cam.fx, 1 / cam.fy
    geo = (ost, oen, oids, tlp, psx, psy, H, W)
    d = {k: L.to_dev(v) for k, v in dict(col=col, al=al, tlp=tlp).items()}
    go = np.random.default_rng(3).normal(size=(H, W, 3)).astype(np.float32)

    def close(a, b):
        assert np.abs(a - b).max() <= rtol * (np.abs(b).max() + 1e-12) + atol
    # RGB
    out = L.to_dev(np.zeros((H, W, 3), np.float32)); T = L.to_dev(np.ones((H, W), np.float32))
    L.lib.vol_render_start_end_with_T(N, D, h["m2"].p, h["c2"].p, d["col"].p, d["al"].p, st.p, en.p, ids.p, out.p, d["tlp"].p, ts,
                                      nth, ntw, psx, psy, H, W, 1e-4, T.p, L.stream)
    sync()
    ref, refT = O.render_rgb_fwd(m2, c2, col, al, *geo, tile_size=ts)
    assert np.abs(out.get() - ref).max() < ftol and np.abs(T.get() - refT.reshape(H, W)).max() < max(ftol, 1.0001e-4 if ftol > 1e-5 else 0)
    bgimg = np.random.default_rng(4).uniform(size=(H, W, 3)).astype(np.float32)
    final = (ref + refT.reshape(H, W, 1) * bgimg).astype(np.float32)
    g = {k: L.to_dev(np.zeros(s_, np.float32)) for k, s_ in dict(gm=(N, 2), gc=(N, 4), gcol=(N, 3), ga=(N,)).items()}
    fin = L.to_dev(final); god = L.to_dev(go)
    L.lib.vol_render_backward_start_end(N, D, h["m2"].p, h["c2"].p, d["col"].p, d["al"].p, st.p, en.p, ids.p, fin.p, g["gm"].p,
                                        g["gc"].p, g["gcol"].p, g["ga"].p, god.p, d["tlp"].p, ts, nth, ntw, psx, psy, H, W,
                                        1e-4, L.stream)
    sync()
    om, oc, ocol, oa = O.render_rgb_bwd(m2, c2, col, al, ost, oen, oids, final, go, tlp, psx, psy, H, W, tile_size=ts)
    for a, b in ((g["gm"], om), (g["gc"], oc.reshape(-1, 4)), (g["gcol"], ocol), (g["ga"], oa)):
        close(a.get(), b)
    # scalar
    sval = np.ascontiguousarray(dep); sv = L.to_dev(sval)
    sout = L.to_dev(np.zeros((H, W), np.float32)); sT = L.to_dev(np.ones((H, W), np.float32))
    L.lib.vol_render_scalar(N, D, h["m2"].p, h["c2"].p, sv.p, d["al"].p, st.p, en.p, ids.p, sout.p, d["tlp"].p, ts, nth, ntw,
                            psx, psy, H, W, 1e-4, sT.p, L.stream)
    sync()
    sref, _ = O.render_scalar_fwd(m2, c2, sval, al, *geo, tile_size=ts)
    assert np.abs(sout.get() - sref).max() < ftol * max(1.0, np.abs(sref).max())
    sgo = np.ascontiguousarray(go[..., 0]); sgod = L.to_dev(sgo); srefd = L.to_dev(sref)
    g = {k: L.to_dev(np.zeros(s_, np.float32)) for k, s_ in dict(gm=(N, 2), gc=(N, 4), gs=(N,), ga=(N,)).items()}
    L.lib.vol_render_scalar_backward(N, D, h["m2"].p, h["c2"].p, sv.p, d["al"].p, st.p, en.p, ids.p, srefd.p, g["gm"].p,
                                     g["gc"].p, g["gs"].p, g["ga"].p, sgod.p, d["tlp"].p, ts, nth, ntw, psx, psy, H, W, 1e-4,
                                     L.stream)
    sync()
    om, oc, os_, oa = O.render_scalar_bwd(m2, c2, sval, al, ost, oen, oids, sref, sgo, tlp, psx, psy, H, W, tile_size=ts)
    for a, b in ((g["gm"], om), (g["gc"], oc.reshape(-1, 4)), (g["gs"], os_), (g["ga"], oa)):
        close(a.get(), b)
    # SH with a background
    sh = np.ascontiguousarray(sc["sh"][m]); rot = np.ascontiguousarray(cam.c2w[:3, :3]).reshape(-1).copy()
    bg = np.array([0.2, 0.5, 0.7], np.float32)
    shd, rotd, bgd = L.to_dev(sh), L.to_dev(rot), L.to_dev(bg)
    out = L.to_dev(np.zeros((H, W, 3), np.float32))
    L.lib.vol_render_sh(N, D, h["m2"].p, h["c2"].p, shd.p, d["al"].p, st.p, en.p, ids.p, out.p, d["tlp"].p, rotd.p, ts, nth, ntw,
                        psx, psy, H, W, C, 1e-4, bgd.p, None, L.stream)
    sync()
    ref = O.render_sh_fwd(m2, c2, sh, al, ost, oen, oids, tlp, rot, C, psx, psy, H, W, bg=bg, tile_size=ts)
    scenes.assert_sh_image_parity(out.get(), ref, m2, c2, al, ost, oen, oids, tlp, psx, psy, tol=ftol, what=f"tile {ts}")
    g = {k: L.to_dev(np.zeros(s_, np.float32)) for k, s_ in dict(gm=(N, 2), gc=(N, 4), gsh=(N, 3, C * C), ga=(N,)).items()}
    L.lib.vol_render_backward_sh(N, D, h["m2"].p, h["c2"].p, shd.p, d["al"].p, st.p, en.p, ids.p, out.p, g["gm"].p, g["gc"].p,
                                 g["gsh"].p, g["ga"].p, god.p, d["tlp"].p, rotd.p, ts, nth, ntw, psx, psy, H, W, C, 1e-4, bgd.p,
                                 L.stream)
    sync()
    om, oc, osh, oa = O.render_sh_bwd(m2, c2, sh, al, ost, oen, oids, ref, go, tlp, rot, C, psx, psy, H, W, tile_size=ts)
    margin = O.sh_decision_margin(m2, c2, al, ost, oen, oids, tlp, psx, psy, H, W, tile_size=ts)
    if atol == 0.0 or margin.min() > 4e-7:
        for a, b in ((g["gm"], om), (g["gc"], oc.reshape(-1, 4)), (g["gsh"], osh), (g["ga"], oa)):
            close(a.get(), b)
    # tile sizes beyond the reference's own limit (tile_size^2 <= 1024 threads per tile) are refused, not misrendered
    for bad in (0, 33):
        with pytest.raises(Exception, match="unsupported"):
            L.lib.vol_render_sh(N, D, h["m2"].p, h["c2"].p, shd.p, d["al"].p, st.p, en.p, ids.p, out.p, d["tlp"].p, rotd.p, bad, nth,
                                ntw, psx, psy, H, W, C, 1e-4, bgd.p, None, L.stream)
