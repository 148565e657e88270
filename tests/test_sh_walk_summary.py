"""The walk summary of the batched polynomial SH kernels (include/gsgen_hip.h, "the walk summary"; composite_common.hpp, kWalkWords):
the one-wavefront-per-tile polynomial forward of a routed batch leaves, per (view, tile), where its entry loop stopped, which list
entries reached a pixel and on which the threshold guard tripped; the polynomial backward of the same views takes those decisions
instead of voting again.  Every case runs the routed batch forward + backward -- which use the summary -- in both gradient forms and
compares against the per-camera routed pair on the same views (gsgen_vol_render_sh_routed / gsgen_vol_render_backward_sh_routed),
which uses none: images and T bit for bit, gradients up to fp32 summation order.

Each case runs on the CPU host build of the kernels (`emu`) and, marked `gpu`, on the device through the same C API.

Shapes: two views of 48 x 40 pixels (3 x 3 tiles, a partial right column and bottom row), SH degree 3, 500 splats of
scenes.random_scene with higher bands small enough for the polynomial form everywhere, plus the few splats a case adds in the
image plane (2-D mean / covariance / place in the tiles' lists given directly: the compositing kernels take lists as they come).
Every splat is listed in ONE tile per view (Views.__init__): each gradient is then a sum of at most two values, one per view, which
fp32 addition forms alike in either order -- the device's float atomics may land as they like, and every figure is reproducible.

THE GRADIENT BOUND.  What "up to summation order" amounts to was measured on the commit BEFORE the summary existed, with the very
comparisons below (the same scenes, launches and figure: max |a - b| / max |b| per gradient tensor), per comparison, gradient form
and tensor, on the CPU host build and on an MI355X (eight runs, all alike, and 24 more that stayed within them); the figures are
recorded in tests/golden/sh_walk_summary_parent_figures.json, rounded up to three digits, and the kernels with the summary are held
to exactly them -- no factor, no pooling.  Most are 0: the batch adds the same values as the per-camera pair.  Those that are not:
the moment form's mean2d / cov2d, which are expanded on the host here (moment / det, 0.5 moment / det^2, fp64) and differ from the
per-pixel fp32 form by rounding (1e-7 .. 1e-6), and the launches with n_segments = 2, whose segments restart from a stored prefix --
another arithmetic, 2e-3 of the largest entry where a tile saturates behind opaque layers (1 / (1 - a G) = 100 there).

What this file cannot see: the per-camera pair goes through the same gauss_sh_pair, contribution mask and sh_guard_trips as the
batch, so a change of G, a G, the mask or the guard's trips against the PARENT would pass here.  That the `radial < 0` term left
them bit for bit what they were rests on the existing suites (the oracle parity tests of every SH kernel, untouched) and on the
benchmark's images, bit-identical between the parent's build and this one (profiles/r10_notes.md section 6).

A departure from the issue's wording, the flagged tile with no_fallback = 1: there the batch keeps the crowded tile
in the polynomial kernel (per-entry exact tier) while the per-camera kernel, which decides per tile, renders it exactly -- two
different computations by design, within the routing's 1e-5 of each other, so "bit-equal to the per-camera pair" cannot hold
inside that tile.  That run is compared bit for bit against the same
batch launched with n_segments = 2, which walks the same kernels' other path without a summary, and against the per-camera pair
outside the crowded tile (bit for bit) and inside it (1e-5)."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, C, B = 48, 40, 4, 2
NTH, NTW = 3, 3
T = NTH * NTW
FX = (160.0, 176.0)
THRESH = 1e-4
K_MIN = 0.00392156862745098      # 1 / 255, the skip threshold (common.hpp)
GUARD_TOL = 2.0e-4               # kGuardTol
WALK_K, WALK_WORDS = 8, 17       # composite_common.hpp: walked, contributed[8], guarded[8]

# tests/golden/sh_walk_summary_parent_figures.json: [backend]["<comparison>|<form>"] -> the parent's figure per gradient tensor
with open(os.path.join(ROOT, "tests", "golden", "sh_walk_summary_parent_figures.json")) as _f:
    PARENT_FIGURES = json.load(_f)


# ---- where the arrays live -----------------------------------------------------------------------------------------------------------

class HostArrays:
    """the CPU host build works on host memory: "device" arrays are numpy arrays"""
    kind = "cpu"

    class Arr:
        def __init__(self, a):
            self.a = np.ascontiguousarray(a).copy(); self.p = self.a.ctypes.data

        def get(self):
            return self.a.copy()

    def __init__(self, lib):
        self.lib, self.stream = lib, None

    def to_dev(self, a):
        return self.Arr(a)

    def sync(self):
        pass


class DeviceArrays:
    kind = "gpu"

    class Arr:
        def __init__(self, a):
            import torch
            self.t = torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0"); self.p = self.t.data_ptr()

        def get(self):
            return self.t.cpu().numpy()

    def __init__(self, lib=None):
        import torch
        from gsgen_amd import _capi
        self.lib, self.stream = lib or _capi.load(), torch.cuda.current_stream().cuda_stream

    def to_dev(self, a):
        return self.Arr(a)

    def sync(self):
        import torch
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "emu"])
    from gsgen_amd import _capi
    return HostArrays(_capi.Lib(os.path.join(ROOT, "oracle", "_build", "libgsgen_emu.so")))


@pytest.fixture(scope="module")
def gpu():
    return DeviceArrays()


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------

class Views:
    """The two views' compositing inputs: shared sh / alpha, per view the 2-D records and one list of splat ids per tile (front first)."""

    def __init__(self, seed=3, alpha_scale=0.5):
        import scenes
        sc = scenes.random_scene(500, seed=seed, svec=0.06, C=C)
        sc["sh"][:, :, 1:] *= 0.0078   # within the polynomial form's coefficient bound at these focal lengths
        self.sh = [r for r in sc["sh"].astype(np.float32)]
        self.alpha = [np.float32(a * alpha_scale) for a in sc["alpha"]]
        self.cams = [scenes.Camera(W, H, fx=fx, c2w=scenes.orbit(2.5, 10 + 20 * i, 40.0 + 100 * i)) for i, fx in enumerate(FX)]
        self.m2, self.c2, self.lists = [], [], []
        for cam in self.cams:
            assert cam.tiles == (NTH, NTW)
            g = scenes.oracle_geometry(sc, cam)
            nz = np.nonzero(g["mask"])[0]
            m2 = np.zeros((500, 2), np.float32); c2 = np.zeros((500, 2, 2), np.float32)
            c2[:] = np.eye(2, dtype=np.float32)
            m2[nz] = g["mean2d"]; c2[nz] = g["cov2d"]
            ids = nz[g["ids"]]
            self.m2.append([r for r in m2]); self.c2.append([r for r in c2])
            lists = [[int(i) for i in ids[s:e]] if s >= 0 else [] for s, e in zip(g["start"], g["end"])]
            # ONE tile per (view, splat) -- the tile of its centre where that lists it, else the first that does: every gradient is
            # then a sum of at most two values (one per view), which floating-point addition forms alike in either order, so that
            # the device's results do not depend on the order its atomics land in and every figure below is reproducible
            home = {}
            for t, lst in enumerate(lists):
                for i in lst:
                    gx, gy = (m2[i] - cam.topleft) * np.array([cam.fx, cam.fy])
                    own = 0 <= gx < W and 0 <= gy < H and t == int(gy // 16) * NTW + int(gx // 16)
                    if i not in home or own:
                        home[i] = t
            self.lists.append([[i for i in lst if home[i] == t] for t, lst in enumerate(lists)])
        self.go = [np.random.default_rng(10 + i).normal(size=(H, W, 3)).astype(np.float32) for i in range(B)]
        self.bg = np.array([0.3, 0.1, 0.2], np.float32)

    def pixel(self, view, gx, gy):
        """the image-plane position of pixel (gx, gy), formed as the kernels form it (common.hpp, pixel_coord)"""
        cam = self.cams[view]
        ps = np.float32(1.0 / cam.fx), np.float32(1.0 / cam.fy)
        return cam.topleft[0] + np.float32(gx) * ps[0], cam.topleft[1] + np.float32(gy) * ps[1]

    def sigma(self, view, pixels):
        return pixels / self.cams[view].fx

    def add(self, means, covs, alpha, sh=None):
        """one more splat: its 2-D mean and covariance per view; returns its id (it is in no list yet)"""
        row = np.zeros((3, 16), np.float32) if sh is None else np.asarray(sh, np.float32)
        if sh is None:
            row[:, 0] = (0.8, -0.4, 1.5)
        self.sh.append(row); self.alpha.append(np.float32(alpha))
        for v in range(B):
            self.m2[v].append(np.asarray(means[v], np.float32)); self.c2[v].append(np.asarray(covs[v], np.float32).reshape(2, 2))
        return len(self.alpha) - 1

    def arrays(self):
        N = len(self.alpha)
        out = dict(N=N, sh=np.ascontiguousarray(np.stack(self.sh), np.float32), alpha=np.asarray(self.alpha, np.float32), views=[])
        for v in range(B):
            ids = np.asarray([i for lst in self.lists[v] for i in lst] + [0], np.int32)
            lens = np.asarray([len(lst) for lst in self.lists[v]])
            end = np.cumsum(lens).astype(np.int32)
            start = np.where(lens > 0, end - lens, -1).astype(np.int32)
            cam = self.cams[v]
            out["views"].append(dict(m2=np.stack(self.m2[v]).astype(np.float32), c2=np.stack(self.c2[v]).astype(np.float32), st=start, en=end, ids=ids,
                                     D=int(lens.sum()), lens=lens, tlp=cam.topleft, rot=np.ascontiguousarray(cam.c2w[:3, :3].reshape(-1)),
                                     ps=(1.0 / cam.fx, 1.0 / cam.fy), go=self.go[v], bg=self.bg))
        return out


def gauss64(m, c, p):
    """the Gaussian of kernels.h:172-193 in fp64 from the fp32 inputs, and its radial numerator"""
    c = np.asarray(c, np.float64).reshape(4); x, y = float(p[0]) - float(m[0]), float(p[1]) - float(m[1])
    det = c[0] * c[3] - c[1] * c[2]
    q = (x * c[3] - y * c[2]) * x + (y * c[0] - x * c[1]) * y
    return float(np.exp(-0.5 * q / det)), q


def iso(s):
    return np.array([[s * s, 0.0], [0.0, s * s]], np.float32)


def case_mid_batch_saturation():
    """in every tile: 38 thin splats, then three opaque layers (alpha 0.99, G ~ 1 over the tile), then the scene's own entries -- the
    tile saturates at its 41st entry, in the middle of its second batch, with entries left behind it wherever the scene has any"""
    V = Views(alpha_scale=0.1)
    rng = np.random.default_rng(7)
    for t in range(T):
        ty, tx = divmod(t, NTW)
        w, h = min(16, W - 16 * tx), min(16, H - 16 * ty)
        front = []
        for k in range(41):
            gx, gy = 16 * tx + rng.uniform(0, w - 1), 16 * ty + rng.uniform(0, h - 1)
            big = k >= 38
            front.append(V.add([V.pixel(v, gx, gy) for v in range(B)], [iso(V.sigma(v, 4000.0 if big else 4.0)) for v in range(B)],
                               0.99 if big else 0.02))
        for v in range(B):
            V.lists[v][t][0:0] = front
    return V


def case_past_the_cap():
    """320 thin splats (alpha 0.02) over the middle tile, in front of everything else there: the walk passes the summary's 256
    entries and never saturates"""
    V = Views(alpha_scale=0.1)
    rng = np.random.default_rng(5)
    new = []
    for _ in range(320):
        off = rng.uniform(-6.0, 6.0, 2)
        new.append(V.add([V.pixel(v, 23.5 + off[0], 23.5 + off[1]) for v in range(B)], [iso(V.sigma(v, 4.0)) for v in range(B)], 0.02,
                         sh=np.concatenate([rng.normal(0, 1.0, (3, 1)), rng.normal(0, 0.002, (3, 15))], 1)))
    for v in range(B):
        V.lists[v][4][0:0] = new
    return V


def case_non_contributing():
    """splats centred 4 pixels inside the middle tile (sigma 2 pixels, alpha 0.04: a G <= 0.0032 < 1 / 255 from 4.5 pixels on) listed in
    the tile to its LEFT, where nobody sees them, between entries that are seen"""
    V = Views()
    for k in range(12):
        i = V.add([V.pixel(v, 20.0, 17.0 + k) for v in range(B)], [iso(V.sigma(v, 2.0)) for v in range(B)], 0.04)
        for v in range(B):
            V.lists[v][3].insert(min(2 * k + 1, len(V.lists[v][3])), i)
    return V


def case_guard_trip():
    """two splats at the front of the first tile whose a G at a chosen pixel centre lies 5e-5 (relative) above / below 1 / 255 -- a
    quarter of the guard's window, thousands of fp32 roundings of the product: inside the window whichever exponential forms G, and
    on its side of the threshold once the guard has taken the reference's arithmetic"""
    V = Views()
    for k, (gx, gy, side) in enumerate(((5, 6, +1.0), (9, 3, -1.0))):
        means = [V.pixel(v, gx + 2.25, gy - 1.5) for v in range(B)]
        covs = [iso(V.sigma(v, 2.5)) for v in range(B)]
        G, _ = gauss64(means[0], covs[0], V.pixel(0, gx, gy))
        i = V.add(means, covs, K_MIN / G * (1.0 + side * 5e-5))
        a, m, c = float(V.alpha[i]), V.m2[0][i], V.c2[0][i]
        rel = a * gauss64(m, c, V.pixel(0, gx, gy))[0] / K_MIN - 1.0
        assert side * rel > 0 and abs(rel) < 0.5 * GUARD_TOL   # (with the fp32 alpha and the fp32 pixel position)
        for v in range(B):
            V.lists[v][0].insert(k, i)
    return V


def case_non_psd():
    """two splats whose covariance has a positive determinant and an indefinite symmetric part (radial < 0 on a wedge of pixels): an
    opaque one, and a faint one whose RAW a G -- the exponential of the negative radial, beyond 1 -- sits on the skip threshold at
    such a pixel, where the Gaussian is 0 and the guard has nothing to ask"""
    V = Views()
    s2 = [V.sigma(v, 5.0) ** 2 for v in range(B)]
    covs = [np.array([[1.0, 4.0], [0.2, 1.0]], np.float32) * s for s in s2]
    means = [V.pixel(v, 10.0, 9.0) for v in range(B)]
    i0 = V.add(means, covs, 0.8)
    # a pixel of view 0 with radial < 0 and a moderate raw exponential
    cand = [(gx, gy) for gx in range(16) for gy in range(16)]
    raw = [(gauss64(means[0], covs[0], V.pixel(0, gx, gy)), (gx, gy)) for gx, gy in cand]
    neg = [(g, p) for (g, q), p in raw if q < 0 and 1.5 < g < 50.0]
    assert neg and any(q < 0 for (g, q), p in raw) and any(q > 0 for (g, q), p in raw)
    g_raw, _ = neg[0]
    i1 = V.add(means, covs, K_MIN / g_raw * (1.0 + 1e-5))
    for v in range(B):
        V.lists[v][0][0:0] = [i0, i1]
    return V


def case_flagged_tile():
    """twelve splats with large higher bands in the middle of the middle tile (sigma 1 pixel: they reach no other tile), at the front
    of its list: more than a quarter of its first staged batch is beyond the coefficient bound"""
    V = Views()
    rng = np.random.default_rng(9)
    new = []
    for _ in range(12):
        off = rng.uniform(-2.0, 2.0, 2)
        row = rng.normal(0, 0.3, (3, 16)).astype(np.float32); row[:, 9:] = 3.0
        new.append(V.add([V.pixel(v, 23.5 + off[0], 23.5 + off[1]) for v in range(B)], [iso(V.sigma(v, 1.0)) for v in range(B)], 0.3, sh=row))
    for v in range(B):
        V.lists[v][4][0:0] = new
    return V


# ---- launches --------------------------------------------------------------------------------------------------------------------------

def device_inputs(A, V):
    a = V.arrays()
    d = dict(N=a["N"], sh=A.to_dev(a["sh"]), al=A.to_dev(a["alpha"]), rows=A.to_dev(np.zeros(a["N"], np.float32)), views=a["views"])
    A.lib.sh_l1_bound_rows(a["N"], d["sh"].p, C, None, d["rows"].p, A.stream)
    A.sync()
    d["dev"] = [{k: A.to_dev(v[k]) for k in ("m2", "c2", "st", "en", "ids", "tlp", "rot", "go", "bg")} for v in a["views"]]
    return d


def run_batch(A, d, moments, nseg=0, fill=0, no_fallback=0, backwards=1):
    """the routed batch forward + `backwards` backward launches; the workspace starts out as bytes of `fill`"""
    from gsgen_amd._capi import ShView
    L, N = A.lib, d["N"]
    arr = (ShView * B)()
    outs = []
    for a, v, dv in zip(arr, d["views"], d["dev"]):
        o = dict(out=A.to_dev(np.full((H, W, 3), 9.0, np.float32)), T=A.to_dev(np.full((H, W), 9.0, np.float32)))
        a.mean, a.cov, a.start, a.end, a.gaussian_ids = dv["m2"].p, dv["c2"].p, dv["st"].p, dv["en"].p, dv["ids"].p
        a.tile_order, a.topleft, a.c2w, a.bg_rgb = None, dv["tlp"].p, dv["rot"].p, dv["bg"].p
        a.pixel_size_x, a.pixel_size_y = v["ps"]
        a.out, a.T, a.grad_out = o["out"].p, o["T"].p, dv["go"].p
        o["seg"] = A.to_dev(np.zeros(L.segment_workspace_bytes(T, nseg), np.uint8)) if nseg > 1 else None
        a.segment_workspace = o["seg"].p if nseg > 1 else None
        a.route_report, a.no_fallback = None, no_fallback
        outs.append(o)
    bws = A.to_dev(np.full(L.sh_batch_workspace_bytes_routed(B, T), fill, np.uint8))
    geo = (16, NTH, NTW, H, W, C, THRESH, nseg)
    L.vol_render_sh_batch_routed(B, arr, N, d["sh"].p, d["al"].p, *geo, None, d["rows"].p, bws.p, A.stream)
    res = []
    for _ in range(backwards):
        gms, gcs = [A.to_dev(np.zeros((N, 2), np.float32)) for _ in range(B)], [A.to_dev(np.zeros((N, 4), np.float32)) for _ in range(B)]
        for a, gm, gc in zip(arr, gms, gcs):
            a.grad_mean, a.grad_cov = gm.p, gc.p
        gsh, ga = A.to_dev(np.zeros((N, 3, 16), np.float32)), A.to_dev(np.zeros(N, np.float32))
        bwd = L.vol_render_backward_sh_batch_routed_moments if moments else L.vol_render_backward_sh_batch_routed
        bwd(B, arr, N, d["sh"].p, d["al"].p, gsh.p, ga.p, *geo, None, d["rows"].p, bws.p, A.stream)
        A.sync()
        r = dict(img=[o["out"].get() for o in outs], T=[o["T"].get() for o in outs], gm=[x.get() for x in gms], gc=[x.get() for x in gcs],
                 gsh=gsh.get(), ga=ga.get())
        if moments:   # moments -> gradients, as the projection backward expands them (geometry.hip, moments_to_grads_sh), in fp64
            for i, v in enumerate(d["views"]):
                c = v["c2"].reshape(N, 4)
                det = (c[:, 0] * c[:, 3] - c[:, 1] * c[:, 2]).astype(np.float64)
                det = np.where(det > 0, det, 1.0)
                m = r["gc"][i].astype(np.float64); h = 0.5 / det ** 2
                r["gc"][i] = np.stack([h * m[:, 0], h * m[:, 1], h * m[:, 1], h * m[:, 2]], 1)
                r["gm"][i] = r["gm"][i].astype(np.float64) / det[:, None]
        res.append(r)
    res[0]["workspace"] = bws.get()
    return res if backwards > 1 else res[0]


def routing_flags(A, res):
    return res["workspace"][A.lib.sh_batch_workspace_bytes(B):][:B * T].reshape(B, T).copy()


def walk_summary(A, res):
    """[view, tile, word] of the summary records: behind the two parameter tables and the flag bytes (padded to 16)"""
    o = A.lib.sh_batch_workspace_bytes(B) + ((B * T + 15) & ~15)
    return res["workspace"][o:][:B * T * WALK_WORDS * 4].copy().view(np.uint32).reshape(B, T, WALK_WORDS)


def run_per_camera(A, d):
    """the per-camera routed pair on the same views: the reference that knows no summary"""
    L, N = A.lib, d["N"]
    gsh, ga = A.to_dev(np.zeros((N, 3, 16), np.float32)), A.to_dev(np.zeros(N, np.float32))
    r = dict(img=[], T=[], gm=[], gc=[])
    for v, dv in zip(d["views"], d["dev"]):
        geo = (16, NTH, NTW, v["ps"][0], v["ps"][1], H, W, C, THRESH)
        # (the batched forward writes every pixel; the per-camera one leaves the empty tiles to the caller: the background, T = 1)
        img0 = np.zeros((H, W, 3), np.float32); img0[:] = v["bg"]
        out, Tt = A.to_dev(img0), A.to_dev(np.ones((H, W), np.float32))
        L.vol_render_sh_routed(N, v["D"], dv["m2"].p, dv["c2"].p, d["sh"].p, d["al"].p, dv["st"].p, dv["en"].p, dv["ids"].p, out.p, dv["tlp"].p,
                               dv["rot"].p, *geo, dv["bg"].p, Tt.p, None, None, 0, None, d["rows"].p, A.stream)
        gm, gc = A.to_dev(np.zeros((N, 2), np.float32)), A.to_dev(np.zeros((N, 4), np.float32))
        L.vol_render_backward_sh_routed(N, v["D"], dv["m2"].p, dv["c2"].p, d["sh"].p, d["al"].p, dv["st"].p, dv["en"].p, dv["ids"].p, out.p,
                                        gm.p, gc.p, gsh.p, ga.p, dv["go"].p, dv["tlp"].p, dv["rot"].p, *geo, dv["bg"].p, None, None, 0,
                                        None, d["rows"].p, A.stream)
        A.sync()
        r["img"].append(out.get()); r["T"].append(Tt.get()); r["gm"].append(gm.get()); r["gc"].append(gc.get())
    r["gsh"], r["ga"] = gsh.get(), ga.get()
    return r


def grad_figures(got, ref):
    """max |a - b| / max |b| per gradient tensor (the views' mean2d / cov2d: the worse view)"""
    def rel(a, b):
        b = np.asarray(b, np.float64)
        assert np.abs(b).max() > 0
        return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())
    return dict(gsh=rel(got["gsh"], ref["gsh"]), ga=rel(got["ga"], ref["ga"]), gm=max(rel(a, b) for a, b in zip(got["gm"], ref["gm"])),
                gc=max(rel(a, b) for a, b in zip(got["gc"], ref["gc"])))


def same_images(got, ref, skip=None):
    for v in range(B):
        a, b = got["img"][v].copy(), ref["img"][v].copy()
        if skip is not None:
            a[skip] = 0; b[skip] = 0
        assert np.array_equal(a, b), (v, float(np.abs(a - b).max()))
        assert np.array_equal(got["T"][v], ref["T"][v]), v


def check_grads(A, got, ref, moments, what):
    """the comparison `what` of this backend and form, tensor by tensor against the figure the parent commit gave for it"""
    fig = grad_figures(got, ref)
    form = "moments" if moments else "plain"
    print(f"[walk summary] {A.kind} {what}|{form}: " + " ".join(f"{k}={v:.3e}" for k, v in fig.items()))
    bound = PARENT_FIGURES[A.kind][f"{what}|{form}"]
    for k, v in fig.items():
        assert v <= bound[k], (what, form, k, v, bound[k])
    return fig


def bits(words):
    return np.unpackbits(words.astype("<u4").view(np.uint8), bitorder="little")


# ---- the cases -------------------------------------------------------------------------------------------------------------------------

def compare_case(A, name, moments):
    V = CASES[name]()
    d = device_inputs(A, V)
    ref = run_per_camera(A, d)
    got = run_batch(A, d, moments)
    assert not routing_flags(A, got).any()              # every tile from the polynomial kernels
    same_images(got, ref)
    check_grads(A, got, ref, moments, name)
    return got, d


def check_case(A, name, moments):
    got, d = compare_case(A, name, moments)
    walk = walk_summary(A, got)
    walked, lens = walk[:, :, 0].astype(np.int64), np.stack([v["lens"] for v in d["views"]])
    assert (walked[lens > 0] <= lens[lens > 0]).all() and (walked[lens > 0] > 0).all()
    con = [[bits(walk[v, t, 1:1 + WALK_K]) for t in range(T)] for v in range(B)]
    grd = [[bits(walk[v, t, 1 + WALK_K:]) for t in range(T)] for v in range(B)]
    for v in range(B):
        for t in range(T):
            if lens[v, t] > 0:   # bits of entries never reached are 0
                assert not con[v][t][min(walked[v, t], 256):].any() and not grd[v][t][min(walked[v, t], 256):].any()
    # ... and the case is what it says
    if name == "mid_batch_saturation":
        hit = (walked < lens) & (walked % 32 != 0) & (walked > 32)
        assert hit.any(), (walked, lens)
    elif name == "past_the_cap":
        assert (walked[:, 4] > 256).all() and (walked[:, 4] == lens[:, 4]).all()
    elif name == "non_contributing":
        assert all((~con[v][3][:walked[v, 3]].astype(bool)).sum() >= 6 and con[v][3][:walked[v, 3]].sum() >= 6 for v in range(B))
    elif name == "guard_trip":
        assert grd[0][0][0] == 1 and grd[0][0][1] == 1          # both directions tripped in the view they were placed for
        assert con[0][0][0] == 1                                 # (above the threshold: seen; below: by whoever else it reaches)
    elif name == "non_psd":
        assert con[0][0][0] == 1 and not any(g[0] or g[1] for g in (grd[0][0], grd[1][0]))   # no guard trip on radial < 0


CASES = {"mid_batch_saturation": case_mid_batch_saturation, "past_the_cap": case_past_the_cap, "non_contributing": case_non_contributing,
         "guard_trip": case_guard_trip, "non_psd": case_non_psd}


def check_flagged_tile(A, moments):
    V = case_flagged_tile()
    d = device_inputs(A, V)
    ref = run_per_camera(A, d)
    got = run_batch(A, d, moments)                       # the crowded tile goes to the exact fallback
    assert (routing_flags(A, got)[:, 4] == 1).all() and routing_flags(A, got).sum() == B
    same_images(got, ref)
    check_grads(A, got, ref, moments, "flagged_tile")
    kept = run_batch(A, d, moments, no_fallback=1)       # ... or stays, through the per-entry exact tier (see the module's docstring)
    assert not routing_flags(A, kept).any()
    seg = run_batch(A, d, moments, no_fallback=1, nseg=2)
    same_images(kept, seg)
    check_grads(A, kept, seg, moments, "flagged_tile, no_fallback, against the segmented launch")
    crowded = (slice(16, 32), slice(16, 32))
    same_images(kept, ref, skip=crowded)
    for v in range(B):
        assert np.abs(kept["img"][v][crowded] - ref["img"][v][crowded]).max() <= 1e-5


def check_garbage_workspace(A, moments):
    d = device_inputs(A, case_mid_batch_saturation())
    zero = run_batch(A, d, moments, fill=0)
    for fill in (0xFF, 0x07):
        got = run_batch(A, d, moments, fill=fill)
        same_images(got, zero)
        lens = np.stack([v["lens"] for v in d["views"]])
        assert np.array_equal(walk_summary(A, got)[lens > 0], walk_summary(A, zero)[lens > 0])   # every word of a rendered tile was written
        assert np.array_equal(routing_flags(A, got)[lens > 0], routing_flags(A, zero)[lens > 0])
        check_grads(A, got, zero, moments, f"workspace of {fill:#04x}")


def check_repeated_backward(A, moments):
    d = device_inputs(A, case_mid_batch_saturation())
    first, second = run_batch(A, d, moments, backwards=2)
    check_grads(A, second, first, moments, "second backward")
    check_grads(A, second, run_per_camera(A, d), moments, "second backward against the per-camera pair")


def check_segmented(A, moments):
    d = device_inputs(A, case_mid_batch_saturation())
    one = run_batch(A, d, moments)
    two = run_batch(A, d, moments, nseg=2, fill=0x07)
    same_images(two, one)
    assert (walk_summary(A, two) == 0x07070707).all()    # a segmented launch keeps no summary (and reads none)
    check_grads(A, two, one, moments, "two segments")


FORMS = pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])


@FORMS
@pytest.mark.parametrize("name", list(CASES))
def test_emulated_walk_summary_case(emu, name, moments):
    check_case(emu, name, moments)


@FORMS
def test_emulated_walk_summary_flagged_tile(emu, moments):
    check_flagged_tile(emu, moments)


@FORMS
def test_emulated_walk_summary_garbage_workspace(emu, moments):
    check_garbage_workspace(emu, moments)


@FORMS
def test_emulated_walk_summary_repeated_backward(emu, moments):
    check_repeated_backward(emu, moments)


@FORMS
def test_emulated_walk_summary_segmented_launch(emu, moments):
    check_segmented(emu, moments)


@pytest.mark.gpu
@FORMS
@pytest.mark.parametrize("name", list(CASES))
def test_gpu_walk_summary_case(gpu, name, moments):
    check_case(gpu, name, moments)


@pytest.mark.gpu
@FORMS
def test_gpu_walk_summary_flagged_tile(gpu, moments):
    check_flagged_tile(gpu, moments)


@pytest.mark.gpu
@FORMS
def test_gpu_walk_summary_garbage_workspace(gpu, moments):
    check_garbage_workspace(gpu, moments)


@pytest.mark.gpu
@FORMS
def test_gpu_walk_summary_repeated_backward(gpu, moments):
    check_repeated_backward(gpu, moments)


@pytest.mark.gpu
@FORMS
def test_gpu_walk_summary_segmented_launch(gpu, moments):
    check_segmented(gpu, moments)
