"""The batched RGB + heads pair through the C ABI -- gsgen_vol_render_rgbd_batch, then its backward in the plain form
(gsgen_vol_render_rgbd_backward_batch + gsgen_project_gaussians_backward_batch_heads + gsgen_densify_update_batch) or in the
moment form (gsgen_vol_render_rgbd_backward_batch_moments + gsgen_project_gaussians_backward_batch_heads_moments, statistics
inside the launch) -- with separate head images, a background and optionally z_var, on per-view geometry from the oracle.
Shared by the emulator test and the GPU test (tests/test_fd_heads.py), in the pattern of tests/tile_chain.py: `L` provides
`lib` (the ctypes binding), `stream`, and `to_dev(array)` -> object with `.p` (address), `.n` (elements), `.get()`."""
import ctypes

import numpy as np

import scenes
from gsgen_amd import renderer as R
from gsgen_amd._capi import RgbdView


def batched_heads(L, sc, cams, gos, bg, form, detach_depth, z_var, sync=lambda: None):
    """sc: a scene of post-activation colours; cams: scenes.Camera of one (W, H); gos: per view (g_rgb [H,W,3], g_depth, g_opacity,
    g_depth2 [H,W]); bg [3].  form: "plain" | "moments".  -> dict: "images" (per view rgb, T, depth, opacity, depth2), "grads" (mean,
    qvec, svec, alpha, color, bg), "gm2d" (per view d L / d mean2d), "grad_accum", "cnt", "geo" (the oracle geometry per view)."""
    assert form in ("plain", "moments")
    lib, d = L.lib, L.to_dev
    N = sc["mean"].shape[0]
    W, H, B = cams[0].w, cams[0].h, len(cams)
    nth, ntw = cams[0].tiles
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    mean, qvec, svec, col, al = (d(f32(sc[k])) for k in ("mean", "qvec", "svec", "color", "alpha"))
    bgd = d(f32(bg))
    views = []
    for cam, go in zip(cams, gos):
        g = scenes.oracle_geometry(sc, cam)
        nz = np.nonzero(g["mask"])[0]
        m2 = np.zeros((N, 2), np.float32); c2 = np.zeros((N, 2, 2), np.float32); dv = np.zeros(N, np.float32)
        c2[:] = np.eye(2, dtype=np.float32)
        m2[nz] = g["mean2d"]; c2[nz] = g["cov2d"]; dv[nz] = g["depth"].ravel()
        v = dict(geo=g, m2=d(m2), c2=d(c2), dv=d(dv), st=d(g["start"]), en=d(g["end"]), ids=d(nz[g["ids"]].astype(np.int32)),
                 tlp=d(cam.topleft), mask=d(g["mask"].astype(np.uint8)), cam=d(R.CameraInfo(*cam.intr).pack(cam.c2w)),
                 rgb=d(np.zeros((H, W, 3), np.float32)), T=d(np.zeros((H, W), np.float32)),
                 gm=d(np.zeros((N, 2), np.float32)), gc=d(np.zeros((N, 4), np.float32)), gch=d(np.zeros((N, 6), np.float32)),
                 gbg=d(np.zeros((64, 4), np.float32)), go=[d(f32(x)) for x in go])
        v["heads"] = [d(np.zeros((H, W), np.float32)) for _ in range(3)]
        views.append(v)
    arr = (RgbdView * B)()
    for a, v, cam in zip(arr, views, cams):
        a.mean, a.cov, a.depth, a.start, a.end, a.gaussian_ids = v["m2"].p, v["c2"].p, v["dv"].p, v["st"].p, v["en"].p, v["ids"].p
        a.tile_order, a.topleft, a.pixel_size_x, a.pixel_size_y = None, v["tlp"].p, 1 / cam.fx, 1 / cam.fy
        a.out6, a.T, a.out_rgb = None, v["T"].p, v["rgb"].p
        a.out_depth, a.out_opacity, a.out_depth2 = (x.p for x in v["heads"])
        a.bg_rgb, a.depth_variance = bgd.p, 1 if z_var else 0
    bws = d(np.zeros(lib.sh_batch_workspace_bytes(B), np.uint8))
    lib.vol_render_rgbd_batch(B, arr, N, col.p, al.p, 16, nth, ntw, H, W, 1e-4, bws.p, L.stream)
    for a, v in zip(arr, views):
        a.grad_mean, a.grad_cov, a.grad_chan6, a.grad_out6 = v["gm"].p, v["gc"].p, v["gch"].p, None
        a.grad_rgb, a.grad_depth, a.grad_opacity, a.grad_depth2 = (x.p for x in v["go"])
        a.grad_bg = v["gbg"].p
    ga = d(np.zeros(N, np.float32))
    acc, cnt = d(np.zeros(N, np.float32)), d(np.zeros(N, np.float32))
    out = [d(np.zeros((N, n), np.float32)) for n in (3, 4, 3, 3)]
    tab = lambda k: (ctypes.c_void_p * B)(*[v[k].p for v in views])  # noqa: E731
    common = (B, N, mean.p, qvec.p, svec.p, tab("cam"), int(detach_depth), tab("mask"), tab("gm"), tab("gc"), tab("gch"), tab("dv"))
    if form == "plain":
        lib.vol_render_rgbd_backward_batch(B, arr, N, col.p, al.p, ga.p, 16, nth, ntw, H, W, 1e-4, bws.p, L.stream)
        lib.project_gaussians_backward_batch_heads(*common, *[x.p for x in out], L.stream)
        lib.densify_update_batch(B, N, None, tab("gm"), tab("mask"), None, acc.p, cnt.p, L.stream)
    else:
        lib.vol_render_rgbd_backward_batch_moments(B, arr, N, col.p, al.p, ga.p, 16, nth, ntw, H, W, 1e-4, bws.p, L.stream)
        lib.project_gaussians_backward_batch_heads_moments(*common, tab("c2"), None, *[x.p for x in out], acc.p, cnt.p, L.stream)
    sync()
    grads = dict(zip(("mean", "qvec", "svec", "color"), (x.get() for x in out)))
    grads["alpha"] = ga.get()
    grads["bg"] = sum(v["gbg"].get()[:, :3].astype(np.float64).sum(0) for v in views)
    images = [dict(rgb=v["rgb"].get(), T=v["T"].get(), depth=v["heads"][0].get(), opacity=v["heads"][1].get(),
                   depth2=v["heads"][2].get()) for v in views]
    return dict(images=images, grads=grads, gm2d=[v["gm"].get() for v in views], grad_accum=acc.get(), cnt=cnt.get(),
                geo=[v["geo"] for v in views])
