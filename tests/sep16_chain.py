"""Checks of the separable reduce-scatter (wave_reduce_scatter_sep16, gsgen_amd/csrc/common.hpp) and of the polynomial SH backward that
reduces through it, shared by the emulator tests (tests/test_sep16_host.py) and the GPU tests (tests/test_gpu_sep16.py) in the pattern of
tests/tile_chain.py: `A` provides `lib`, `stream` and `to_dev(array) -> object with .p (pointer) and .get() (numpy copy)`."""
import ctypes as Ct

import numpy as np

import scenes

EPS = float(np.finfo(np.float32).eps)


def expanded_slots(x, u):
    """x [64 lanes, 16], u [64] -> fp64 [64 lanes, 8 slots]: what each lane contributes to the slots of its class (lane // 16) -- the
    header's table: classes 0..2 (v0, v1, u v0, v2, u v1, u^2 v0, v3, -), class 3 (v0, v1, 0, v2, 0, 0, v3, -) of the lane's own four
    components of that class (the kernel forms the products on the sums over the four lanes of a column, which share u)"""
    x = x.astype(np.float64)
    u = u.astype(np.float64)
    e = np.zeros((64, 4, 8))
    for lane in range(64):
        for k in range(4):
            v = x[lane, 4 * k:4 * k + 4]
            ue = 0.0 if k == 3 else u[lane]
            e[lane, k] = (v[0], v[1], ue * v[0], v[2], ue * v[1], ue * ue * v[0], v[3], 0.0)
    return e


def helper_check(A, seed, sync=None):
    """64 lanes, 16 random components per lane, u a function of lane & 15: every (class, slot) total against the fp64 sum of the
    expanded per-lane values within 64 fp32 rounding errors of the sum of their magnitudes; `owner` marks each of the 24 live slots
    exactly once; `comp` agrees with where the value landed (every lane, owner or not, holds the total of the slot it names)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(64, 16)).astype(np.float32)
    x[:, rng.integers(0, 16)] *= 1e3   # one component three decades above the rest
    u = np.tile(rng.uniform(-1.0, 1.0, 16).astype(np.float32), 4)
    xd, ud, out = A.to_dev(x), A.to_dev(u), A.to_dev(np.full(192, -7.0, np.float32))
    A.lib.selftest_reduce_scatter_sep16(xd.p, ud.p, out.p, A.stream)
    if sync is not None:
        sync()
    o = out.get()
    e = expanded_slots(x, u)
    tot, mag = e.sum(0).reshape(32), np.abs(e).sum(0).reshape(32)
    live = [8 * k + s for k in range(3) for s in range(7)] + [24, 25, 27]
    owner, comp = o[64:128].astype(int), o[128:192].astype(int)
    assert sorted(owner[owner >= 0].tolist()) == live
    for lane in range(64):
        assert comp[lane] == 8 * (lane // 16) + ((lane >> 1) & 7)
        assert owner[lane] in (-1, comp[lane])
        if comp[lane] in live or comp[lane] == 30:   # (30 = class 3's fourth component: padding in the kernel, summed all the same)
            err = abs(float(o[lane]) - tot[comp[lane]])
            assert err <= 64 * EPS * mag[comp[lane]], (lane, comp[lane], err, mag[comp[lane]])
        elif comp[lane] in (26, 28, 29):             # class 3's products with u = 0
            assert o[lane] == 0.0


# ---- the routed polynomial SH backward against the exact-basis backward -------------------------------------------------------------

# The polynomial form fits the SH basis per tile; its error falls with the tile's angular size (16 pixels / focal length) and is not what
# these tests are about: the views are zoomed in until it lies well inside the tolerance, the scenes shrunk to stay in view.
SHAPES = {  # name -> (W, H, splats, focal lengths of the views, scene spread, splat size)
    "one_full_tile": (16, 16, 40, (800.0,), 0.03, 0.012),
    "partial_tiles": (40, 24, 60, (500.0,), 0.06, 0.02),
    "two_views": (40, 24, 60, (500.0, 540.0), 0.06, 0.02),
}


def _scene(n, seed, spread, svec):
    sc = scenes.random_scene(n, seed=seed, svec=svec, spread=spread, C=4)
    sc["sh"][:, :, 1:] *= 0.0078                      # inside the polynomial form's coefficient bound at these focal lengths
    sc["alpha"] = (sc["alpha"] * 0.3).astype(np.float32)   # no pixel saturates: the whole list reaches the backward
    return sc


def routed_poly_backward_vs_exact(A, shape, moments, sync=None):
    """One batched SH forward + backward (degree 3) per-tile routed -- every tile takes the polynomial form, asserted from the routing flags
    -- against the same launches on the exact kernels alone (no bounds passed).  Tolerance: that of the routed fuzz against the exact
    kernels (tests/test_gpu_sh_bound.py: every gradient within 1e-4 of its largest entry + 1e-6).  Every gradient: mean2d, cov2d (or
    their moments), alpha, sh; grad_cov[1] == grad_cov[2] bit for bit -- in the plain form as the kernel leaves them, in the moment form
    after the projection backward's expansion (geometry.hip, moments_to_grads_sh: repeated here on the kernel's moments, and the
    projection backward's own outputs compared as well)."""
    from gsgen_amd._capi import ShView
    from gsgen_amd import renderer as R
    L = A.lib
    W, H, n, fxs, spread, svec = SHAPES[shape]
    C = 4
    sc = _scene(n, 11, spread, svec)
    cams = [scenes.Camera(W, H, fx=fx, c2w=scenes.orbit(2.5, 10 + 20 * i, 40.0 + 100 * i)) for i, fx in enumerate(fxs)]
    B, N = len(cams), n
    nth, ntw = cams[0].tiles
    T = nth * ntw
    done = sync if sync is not None else (lambda: None)
    sh, al = A.to_dev(sc["sh"]), A.to_dev(sc["alpha"])
    rows, gmax = A.to_dev(np.zeros(N, np.float32)), A.to_dev(np.zeros(1, np.float32))
    L.sh_l1_bound_rows(N, sh.p, C, gmax.p, rows.p, A.stream)
    done()
    assert all(L.sh_poly_applies(float(gmax.get()[0]), 1.0 / c.fx, C) for c in cams)
    views, longest = [], 0
    for i, cam in enumerate(cams):
        g = scenes.oracle_geometry(sc, cam)
        nz = np.nonzero(g["mask"])[0]
        m2 = np.zeros((N, 2), np.float32); c2 = np.zeros((N, 2, 2), np.float32)
        c2[:] = np.eye(2, dtype=np.float32)
        m2[nz] = g["mean2d"]; c2[nz] = g["cov2d"]
        longest = max(longest, int((g["end"] - g["start"]).max()))
        v = dict(m2=m2, c2=c2, st=g["start"], en=g["end"], ids=nz[g["ids"]].astype(np.int32), tlp=cam.topleft,
                 rot=np.ascontiguousarray(cam.c2w[:3, :3].reshape(-1)), bg=np.array([0.3, 0.1, 0.2], np.float32),
                 go=np.random.default_rng(i).normal(size=(H, W, 3)).astype(np.float32), mask=g["mask"].astype(np.uint8),
                 camv=np.ascontiguousarray(R.CameraInfo(*cam.intr).pack(cam.c2w)), out=np.zeros((H, W, 3), np.float32),
                 T=np.zeros((H, W), np.float32))
        views.append({k: A.to_dev(x) for k, x in v.items()})
    assert longest > 32, longest   # a second staging round of the tile's list
    arr = (ShView * B)()
    for a, v, cam in zip(arr, views, cams):
        a.mean, a.cov, a.start, a.end, a.gaussian_ids = v["m2"].p, v["c2"].p, v["st"].p, v["en"].p, v["ids"].p
        a.tile_order, a.topleft, a.c2w, a.bg_rgb = None, v["tlp"].p, v["rot"].p, v["bg"].p
        a.pixel_size_x, a.pixel_size_y = 1 / cam.fx, 1 / cam.fy
        a.out, a.T, a.segment_workspace, a.grad_out = v["out"].p, v["T"].p, None, v["go"].p
    tab = lambda xs: (Ct.c_void_p * B)(*[x.p for x in xs])  # noqa: E731
    geo = (16, nth, ntw, H, W, C, 1e-4, 0)
    res = {}
    for basis in ("exact", "routed"):
        rp = rows.p if basis == "routed" else None
        bws = A.to_dev(np.zeros(L.sh_batch_workspace_bytes_routed(B, T), np.uint8))
        L.vol_render_sh_batch_routed(B, arr, N, sh.p, al.p, *geo, None, rp, bws.p, A.stream)
        gms, gcs = [A.to_dev(np.zeros((N, 2), np.float32)) for _ in views], [A.to_dev(np.zeros((N, 4), np.float32)) for _ in views]
        for a, gm, gc in zip(arr, gms, gcs):
            a.grad_mean, a.grad_cov = gm.p, gc.p
        gsh, ga = A.to_dev(np.zeros((N, 3, 16), np.float32)), A.to_dev(np.zeros(N, np.float32))
        bwd = L.vol_render_backward_sh_batch_routed_moments if moments else L.vol_render_backward_sh_batch_routed
        bwd(B, arr, N, sh.p, al.p, gsh.p, ga.p, *geo, None, rp, bws.p, A.stream)
        done()
        flags = bws.get()[L.sh_batch_workspace_bytes(B):][:B * T]
        if basis == "routed":
            assert not flags.any()   # every tile from the polynomial kernel
        r = dict(gm=[x.get().copy() for x in gms], gc=[x.get().copy() for x in gcs], gsh=gsh.get().copy(), ga=ga.get().copy(),
                 img=[v["out"].get().copy() for v in views])
        if moments:  # the projection backward that consumes the moments (and overwrites grad_mean with d L / d mean2d)
            outs = [A.to_dev(np.zeros((N, k), np.float32)) for k in (3, 4, 3)]
            pm, pq, ps = (A.to_dev(sc[k]) for k in ("mean", "qvec", "svec"))
            L.project_gaussians_backward_batch_moments_sh(B, N, pm.p, pq.p, ps.p, tab([v["camv"] for v in views]), 1,
                                                          tab([v["mask"] for v in views]), tab(gms), tab(gcs), tab([v["c2"] for v in views]),
                                                          *[o.p for o in outs], None, None, A.stream)
            done()
            r["proj"] = [o.get().copy() for o in outs]
            r["gm2d"] = [x.get().copy() for x in gms]
        res[basis] = r

    def close(a, e, what):
        assert np.abs(e).max() > 0, what
        assert np.abs(a - e).max() <= 1e-4 * np.abs(e).max() + 1e-6, (what, float(np.abs(a - e).max()), float(np.abs(e).max()))

    q, e = res["routed"], res["exact"]
    assert max(float(np.abs(a - b).max()) for a, b in zip(q["img"], e["img"])) > 0   # (another basis did render)
    close(q["gsh"], e["gsh"], "sh")
    close(q["ga"], e["ga"], "alpha")
    for i in range(B):
        close(q["gm"][i], e["gm"][i], f"mean2d, view {i}")
        close(q["gc"][i], e["gc"][i], f"cov2d, view {i}")
        if not moments:  # (one value, two holders of its slot, two atomics of one instruction)
            assert np.array_equal(q["gc"][i][:, 1], q["gc"][i][:, 2]) and np.abs(q["gc"][i][:, 1]).max() > 0
        else:
            exp = {}
            for name, r in (("routed", q), ("exact", e)):
                assert not r["gc"][i][:, 3].any()   # (Mxx, Mxy, Myy, untouched)
                c2 = views[i]["c2"].get().reshape(N, 4).astype(np.float32)
                det = c2[:, 0] * c2[:, 3] - c2[:, 1] * c2[:, 2]
                h = 0.5 / det.astype(np.float64) ** 2
                m4 = r["gc"][i].astype(np.float64)
                exp[name] = np.stack([h * m4[:, 0], h * m4[:, 1], h * m4[:, 1], h * m4[:, 2]], 1)
                assert np.array_equal(exp[name][:, 1], exp[name][:, 2]) and np.abs(exp[name][:, 1]).max() > 0
            close(exp["routed"], exp["exact"], f"expanded cov2d, view {i}")
            close(q["gm2d"][i], e["gm2d"][i], f"d L / d mean2d, view {i}")
    if moments:
        for a, b, name in zip(q["proj"], e["proj"], ("mean", "qvec", "svec")):
            close(a, b, name)
