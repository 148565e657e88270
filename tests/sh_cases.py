"""Designed tile lists for the SH compositing kernels (gsgen_amd/csrc/composite.hip, MODE_SH: the unpacked k_composite_fwd /
k_composite_bwd_pixel, the packed exact and polynomial kernels and the persistent fallbacks) through the SH entry points of
include/gsgen_hip.h, against an fp64 restatement of the compositing in plain torch (autograd for the gradients) which knows neither
the oracle nor the kernels: the SH counterpart of tests/chan_cases.py.  Shared by tests/test_sh_cases_host.py (the CPU host build)
and tests/test_gpu_sh_cases.py (the device): `L` is HostArrays / DeviceArrays of tests/test_sh_walk_summary.py.

GEOMETRY.  Two views of 48 x 40 pixels (3 x 3 tiles, a partial right column and bottom row, the corner tile 16 x 8 valid), focal
lengths 400 and 440: the polynomial form's basis error is 0.93 delta^3 with delta = 7.5 sqrt 2 / fx (tests/test_poly_fit_bound.py),
2.7e-4 at fx = 160 -- the size of the per-row gradient bar itself (rtol 1e-3 x Y_0 = 0.28) -- and below a tenth of it from fx = 342
on.  The base scene is the 500-splat scenes.random_scene shrunk by 160 / 400 (spread 0.32, svec 0.024: the image-plane layout of
chan_cases at the larger focal lengths, no tile trivially empty), alpha x 0.1, higher SH bands x 0.1 (row sums ~ 0.4, a fifth of the
polynomial form's coefficient bound 1.96 at fx = 400).  Lists are given directly as start / end / ids; every splat is listed in ONE
tile per view, so every gradient is a sum of at most two values and the order the device's atomics land in plays no part.  Thin
splats sit on whole pixels plus ONE fractional offset with one sigma and one alpha (chan_cases.Scene.thin): their a G lattice is
clear of 1 / 255 once and for all.

THE REFERENCE (`reference(case, C)`), per pixel, front to back: dir = normalize(R (qx, qy, 1)) with the nine packed rotation
floats; Y = the real SH basis of bands 1..C; colour_c = 1 / (1 + exp(-sum_k sh[c][k] Y_k)); a = min(alpha, 0.99), straight-through;
G = exp(-0.5 d^T Sigma^-1 d) with the four independent covariance entries (tests/fd_model.py), G = 0 where the form is negative; an
entry is taken iff !(T < thresh) && !(a G < 1 / 255); w = T a G, T *= 1 - a G; image = sum w colour + T bg.  The take masks are
computed first, in numpy fp64 from the fp32 inputs (frozen decisions).  A record with a non-finite mean, covariance entry or alpha
(+-inf included) or det <= 0 contributes nothing.  Unlike the channel kernels, a covariance with det > 0 and an indefinite symmetric
part DOES contribute outside its wedge (non_psd): SH has no `kernel_rule`.

THE BARS.  Images and T of the exact launches: |got - ref| <= 1e-5 max(1, max |ref|), every pixel, every value finite -- admissible
because `build` has seen the oracle's fp32 SH chain meet it with a ratio <= 0.25 on the same lists.  Launches that may take the
polynomial basis (the *_bounded forms with a bound that passes, the *_routed forms): <= 1e-5 against the polynomial model and <= 2e-5
against the exact reference (the routing's 1e-5 promise + 1e-5 arithmetic).  Gradients, per tensor and launch form: scenes.per_gaussian_grad_error(rtol 1e-3, atol
1e-5) <= 1 against the fp64 reference, sh as [N, 3 C^2] rows, after the oracle's chain met it with <= 0.25.  Rows that must be
exactly zero (entries behind a saturated tile, unseen entries, dropped records) are compared with == 0.  Bit equality where the
project documents it: a camera through the batched launch and the per-camera launch of the same form (gsgen_hip.h: the exact batch
against gsgen_vol_render_sh_segmented, the routed batch against gsgen_vol_render_sh_routed), pixel_size_dev set and not, images
and T with n_segments 2 and 0.

WHERE THE REFERENCE GIVES WAY.  An indefinite symmetric part with det > 0 needs an ASYMMETRIC covariance (a symmetric matrix with
det > 0 is definite), which the projection never produces.  The kernels' mean2d / cov2d gradients are the reference's CUDA formula,
derived for a symmetric Sigma (grad_cov carries one value in both off-diagonals); evaluated at an asymmetric matrix that is not the
derivative of G with respect to four independent entries, which autograd forms: the oracle's own rows of the two non_psd records
differ from it by a factor of hundreds.  Those two records' mean2d / cov2d rows are therefore taken from the oracle's fp32 chain
(`build`); their images, T, sh and alpha gradients, and every row of every other record, are held to the fp64 reference.

THE POLYNOMIAL MODEL (`reference(case, basis="poly", mode=...)`): see its docstring.  Launches that may take the polynomial basis are
held to it as well -- images and T within 1e-5, the gradient bar -- after `build` has seen it within 0.25 of the gradient bar and
1e-5 in colour of the exact model, and every tier decision (poly_row_ok per splat, taylor_row_ok per row) at <= 0.8 x or >= 1.25 x
its limit.  taylor_edge puts rows on either side of the Taylor limit, flagged_tile_7 / _9 seven and nine splats of a staged batch
of 32 beyond the coefficient bound (the per-entry exact tier; the tile flag, asserted from the flag bytes the batched launch
leaves; with and without fallback).

WHAT THIS FILE CANNOT SEE (mutations of the kernels that leave every compared output where it was): `stop >=
e_lo` for `>` in the segmented backward; the threshold guard skipped (it changes a decision only within a few ulp of 1 / 255;
guard_trip's pixels sit 5e-5 from it, which every fp32 evaluation decides alike); the 2 f2 w1 w2 term of taylor_convert (a row inside
the Taylor limit bounds it by 5e-6 of colour, half the image bar)."""
import numpy as np

import scenes
from chan_cases import ALPHA_CLAMP, CORNER, FRAC, MARGIN, MID, NON_PSD, NT, ORACLE_SHARE, last_taken, tile_box, tile_pixels
from test_sh_walk_summary import B, GUARD_TOL, H, K_MIN, NTH, NTW, THRESH, W, DeviceArrays, HostArrays, gauss64, iso  # noqa: F401

FX = (400.0, 440.0)
SHRINK = 160.0 / 400.0
BASE_SEED = 10                # chosen for its margins: the least skip margin of the base scene's own entries is 4.9e-4
POLY_BOUND_ROW = 1.96         # 0.25 S delta^3 <= 1e-5 - 8.7e-7 at fx = 400 (composite_common.hpp poly_row_ok)
EXACT_BAR, POLY_BAR = 1e-5, 2e-5
SENT_IMG, SENT_T = 7.0, 5.0   # what the per-camera launches find in out / T (run_camera)


class Scene:
    """the two views' compositing inputs: shared sh [3,16] / alpha, per view the 2-D records and one list of ids per tile"""

    def __init__(self, seed=BASE_SEED, alpha_scale=0.1):
        sc = scenes.random_scene(500, seed=seed, svec=0.06 * SHRINK, spread=0.8 * SHRINK, C=4)
        sc["sh"][:, :, 1:] *= 0.1
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
            lists = [[int(i) for i in ids[s:e]] if s >= 0 else [] for s, e in zip(g["start"], g["end"])]
            home = {}   # ONE tile per (view, splat): the tile of its centre where that lists it, else the first that does
            for t, lst in enumerate(lists):
                for i in lst:
                    gx, gy = (m2[i] - cam.topleft) * np.array([cam.fx, cam.fy])
                    own = 0 <= gx < W and 0 <= gy < H and t == int(gy // 16) * NTW + int(gx // 16)
                    if i not in home or own:
                        home[i] = t
            self.m2.append([r for r in m2]); self.c2.append([r for r in c2])
            self.lists.append([[i for i in lst if home[i] == t] for t, lst in enumerate(lists)])
        self.go = [np.random.default_rng(10 + i).normal(size=(H, W, 3)).astype(np.float32) for i in range(B)]
        self.bg = np.array([0.3, 0.1, 0.2], np.float32)
        self.rng = np.random.default_rng(1000 + seed)
        self.zero = []      # ids whose every gradient must be exactly 0
        self.bad = []       # ids of dropped records (left out of the oracle's lists, which would carry NaN)
        self.note = {}

    def pixel(self, view, gx, gy):
        """the image-plane position of pixel (gx, gy), formed as the kernels form it (common.hpp, pixel_coord)"""
        cam = self.cams[view]
        ps = np.float32(1.0 / cam.fx), np.float32(1.0 / cam.fy)
        return cam.topleft[0] + np.float32(gx) * ps[0], cam.topleft[1] + np.float32(gy) * ps[1]

    def sigma(self, view, pixels):
        return pixels / self.cams[view].fx

    def rand_sh(self, high=0.02):
        row = self.rng.normal(0, high, (3, 16))
        row[:, 0] = self.rng.normal(0, 1.5, 3)
        return row.astype(np.float32)

    def add(self, means, covs, alpha, sh=None):
        self.sh.append(self.rand_sh() if sh is None else np.asarray(sh, np.float32).reshape(3, 16))
        self.alpha.append(np.float32(alpha))
        for v in range(B):
            self.m2[v].append(np.asarray(means[v], np.float32)); self.c2[v].append(np.asarray(covs[v], np.float32).reshape(2, 2))
        return len(self.alpha) - 1

    def add_px(self, gx, gy, sigma_px, alpha, **kw):
        return self.add([self.pixel(v, gx, gy) for v in range(B)], [iso(self.sigma(v, sigma_px)) for v in range(B)], alpha, **kw)

    def thin(self, tile, n, alpha=0.05, sigma_px=4.0, **kw):
        """n thin splats on the valid pixels of `tile`, each at a whole pixel + FRAC"""
        x0, y0, w, h = tile_box(tile)
        return [self.add_px(x0 + int(self.rng.integers(0, w)) + FRAC[0], y0 + int(self.rng.integers(0, h)) + FRAC[1], sigma_px, alpha, **kw)
                for _ in range(n)]

    def front(self, tile, ids, replace=False):
        for v in range(B):
            self.lists[v][tile] = list(ids) + ([] if replace else self.lists[v][tile])

    def arrays(self, C=4, lists=None):
        N = len(self.alpha)
        sh = np.ascontiguousarray(np.stack(self.sh)[:, :, :C * C], np.float32)
        out = dict(N=N, C=C, sh=sh, alpha=np.asarray(self.alpha, np.float32), views=[])
        for v in range(B):
            ls = (lists or self.lists)[v]
            ids = np.asarray([i for lst in ls for i in lst] + [0], np.int32)
            lens = np.asarray([len(lst) for lst in ls])
            end = np.cumsum(lens).astype(np.int32)
            start = np.where(lens > 0, end - lens, -1).astype(np.int32)
            cam = self.cams[v]
            out["views"].append(dict(m2=np.stack(self.m2[v]).astype(np.float32), c2=np.stack(self.c2[v]).astype(np.float32).reshape(N, 4),
                                     st=start, en=end, ids=ids, D=int(lens.sum()), lens=lens, tlp=cam.topleft,
                                     rot=np.ascontiguousarray(cam.c2w[:3, :3].reshape(-1), np.float32), ps=(1.0 / cam.fx, 1.0 / cam.fy),
                                     psd=np.array([1.0 / cam.fx, 1.0 / cam.fy], np.float32), go=self.go[v], bg=self.bg))
        return out


# ---- the reference ---------------------------------------------------------------------------------------------------------------

def sh_basis64(d, C):
    """the real SH basis of bands 1..C at unit vectors d [P,3] -> [P, C^2] (the usual real form with the Condon-Shortley phase)"""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    Y = [np.full_like(x, 0.28209479177387814)]
    if C >= 2:
        Y += [-0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x]
    if C >= 3:
        Y += [1.0925484305920792 * x * y, -1.0925484305920792 * y * z, 0.94617469575755997 * z * z - 0.31539156525251999,
              -1.0925484305920792 * x * z, 0.54627421529603959 * (x * x - y * y)]
    if C >= 4:
        Y += [0.59004358992664352 * y * (3.0 * x * x - y * y) * -1.0, 2.8906114426405538 * x * y * z,
              0.45704579946446572 * y * (1.0 - 5.0 * z * z), 0.3731763325901154 * z * (5.0 * z * z - 3.0),
              0.45704579946446572 * x * (1.0 - 5.0 * z * z), 1.4453057213202769 * z * (x * x - y * y),
              0.59004358992664352 * x * (3.0 * y * y - x * x)]
    return np.stack(Y, 1)


def records_ok(m2, c2, alpha):
    with np.errstate(all="ignore"):
        c = c2.astype(np.float64)
        det = c[:, 0] * c[:, 3] - c[:, 1] * c[:, 2]
        return np.isfinite(m2).all(1) & np.isfinite(c).all(1) & np.isfinite(alpha) & (det > 0)


LOG2E = 1.4426950408889634
_FIT = []


def shipped_fit():
    """kPolyFit [6,9] as composite_common.hpp ships it (tests/test_poly_fit_bound.py parses it)"""
    if not _FIT:
        from test_poly_fit_bound import shipped_fit as parse
        _FIT.append(parse())
    return _FIT[0]


TAYLOR_ERR, POLY_FIT_TOL = 8.7e-7, 1e-5 - 8.7e-7      # composite_common.hpp kTaylorErr, kPolyFitTol (kPolyFitErr = 1)
EDGE_LO, EDGE_HI = 0.8, 1.25                          # every tier decision sits at <= 0.8 x or >= 1.25 x its limit


def poly_tile(view, t):
    """V [6,16] of tile t -- the shipped kPolyFit through the exact basis at the nine nodes (u, v) in {-1, 0, 1}^2,
    node n = 3 (v + 1) + (u + 1) -- and the monomials (1, v, u, v^2, uv, u^2) [P,6] of its valid pixels, u / v = (column / row - 7.5) / 7.5"""
    ty, tx = divmod(t, NTW)
    R = view["rot"].astype(np.float64).reshape(3, 3)
    n = np.arange(9)
    qx = float(view["tlp"][0]) + (16 * tx + 7.5 + 7.5 * (n % 3 - 1)) * float(np.float32(view["ps"][0]))
    qy = float(view["tlp"][1]) + (16 * ty + 7.5 + 7.5 * (n // 3 - 1)) * float(np.float32(view["ps"][1]))
    d = np.stack([qx, qy, np.ones(9)], 1) @ R.T
    V = shipped_fit() @ sh_basis64(d / np.linalg.norm(d, axis=1, keepdims=True), 4)
    ys, xs, _, _ = tile_pixels(view, t)
    u, v = (xs - 16 * tx - 7.5) / 7.5, (ys - 16 * ty - 7.5) / 7.5
    return V, np.stack([np.ones_like(u), v, u, v * v, u * v, u * u], 1)


def bound_ratio(sh, view):
    """per splat: 0.25 S delta^3 / kPolyFitTol, S = the largest per-channel sum of |higher-band coefficients| (<= 1: poly_row_ok)"""
    with np.errstate(all="ignore"):
        S = np.abs(sh.astype(np.float64)[:, :, 1:]).sum(2).max(1)
        delta = 7.5 * 1.41421356 * max(abs(float(np.float32(view["ps"][0]))), abs(float(np.float32(view["ps"][1]))))
        return 0.25 * S * delta ** 3 / POLY_FIT_TOL


def taylor_ratio(Wn):
    """per (splat, channel) row of W [E,3,6]: (0.00694 (l + q)^3 + 0.02312 q (2 l + q)) / kTaylorErr in the kernels' scaled unit"""
    l = LOG2E * (np.abs(Wn[..., 1]) + np.abs(Wn[..., 2])); q = LOG2E * np.abs(Wn[..., 3:]).sum(-1)
    return (0.00694 * (l + q) ** 3 + 0.02312 * q * (2 * l + q)) / TAYLOR_ERR


def reference(case, C=4, basis="exact", mode="entry", fallback=True):
    """basis = "poly" (C = 4): the second fp64 model, restated from DESIGN.md section 3 and the comments of composite_common.hpp --
    w = V . sh per (tile, splat, channel); the Taylor colour quadratic f0 + f' (L + Q) + f'' / 2 L^2 where taylor_row_ok holds for all
    three channels, else the sigmoid of the quadratic logit; splats beyond poly_row_ok through the exact basis; and, by `mode`, what
    is exact as a whole: "view" (the *_bounded launches: the view, unless the largest row sum of ALL splats passes), "tile" (the
    per-camera routed launch: a tile whose list holds a splat beyond the bound), "entry" (the routed batch: a tile one of whose
    staged batches of 32 holds more than a quarter of such splats -- unless fallback is off).  "tiers": per (view, tile) the
    entries' kind (0 Taylor, 1 logit, 2 exact) and the decisions' distances from their edges.
    -> dict: "img" / "T" per view (fp64 [H,W,3] / [H,W], the background included), "grads" (gsh [N,3,C^2], ga, gm / gc per
    view) of sum grad_out . image, "take"[view][tile] (bool [pixels, entries]), "dead"[view][tile], "margins" (skip, stop)"""
    import torch
    a = case.arrays(C)
    N = a["N"]
    f64 = lambda x: torch.tensor(np.nan_to_num(np.asarray(x, np.float64), nan=0.0, posinf=0.0, neginf=0.0), dtype=torch.float64,  # noqa: E731
                                 requires_grad=True)
    alpha, sh = f64(a["alpha"]), f64(a["sh"])
    bg = torch.tensor(case.bg.astype(np.float64))
    a_eff = alpha + (torch.clamp(alpha, max=ALPHA_CLAMP) - alpha).detach()
    leaves = dict(gm=[], gc=[])
    loss = 0.0
    img, Ts, takes, deads = [], [], [], []
    margins = {"skip": np.inf, "stop": np.inf}
    tiers, edges = [[None] * NT for _ in range(B)], dict(bound=[], taylor=[])
    zero = torch.zeros((), dtype=torch.float64)
    for v, view in enumerate(a["views"]):
        ok_all = records_ok(view["m2"], view["c2"], a["alpha"])
        m2, c2 = f64(view["m2"]), f64(view["c2"])
        leaves["gm"].append(m2); leaves["gc"].append(c2)
        go = torch.tensor(view["go"].astype(np.float64))
        R = view["rot"].astype(np.float64).reshape(3, 3)
        im = np.zeros((H, W, 3)); im[:] = case.bg.astype(np.float64)
        Tim = np.ones((H, W))
        takes.append([]); deads.append([])
        for t in range(NT):
            ys, xs, px, py = tile_pixels(view, t)
            ids = np.asarray(case.lists[v][t], np.int64)
            gop = go[ys, xs]
            if len(ids) == 0:                    # an empty tile shows the background, T = 1
                takes[v].append(np.zeros((len(px), 0), bool)); deads[v].append(False)
                continue
            ok = ok_all[ids]
            with np.errstate(all="ignore"):      # -- the decisions, frozen: numpy fp64 from the fp32 inputs
                m = np.where(ok[:, None], view["m2"][ids].astype(np.float64), 0.0)
                c = np.where(ok[:, None], view["c2"][ids].astype(np.float64), np.array([1.0, 0.0, 0.0, 1.0]))
                al = np.where(ok, np.minimum(a["alpha"][ids].astype(np.float64), ALPHA_CLAMP), 0.0)
            x, y = px[:, None] - m[None, :, 0], py[:, None] - m[None, :, 1]
            q = (x * c[:, 3] - y * c[:, 2]) * x + (y * c[:, 0] - x * c[:, 1]) * y
            radial = q / (c[:, 0] * c[:, 3] - c[:, 1] * c[:, 2])
            ag = al * np.where(radial < 0, 0.0, np.exp(-0.5 * np.maximum(radial, 0.0)))
            T = np.ones(len(px)); take = np.zeros(ag.shape, bool)
            alive_any = np.zeros(len(ids), bool)
            for e in range(len(ids)):
                alive = ~(T < THRESH)
                alive_any[e] = alive.any()
                take[:, e] = alive & ~(ag[:, e] < K_MIN) & ok[e]
                if alive.any() and ok[e]:
                    margins["skip"] = min(margins["skip"], float(np.abs(ag[alive, e] / K_MIN - 1).min()))
                    margins["stop"] = min(margins["stop"], float(np.abs(T[alive] / THRESH - 1).min()))
                T = np.where(take[:, e], T * (1 - ag[:, e]), T)
            takes[v].append(take); deads[v].append(bool((T < THRESH).all()))
            # -- the same composite under autograd, the masks given
            d = np.stack([px, py, np.ones_like(px)], 1) @ R.T
            Y = torch.tensor(sh_basis64(d / np.linalg.norm(d, axis=1, keepdims=True), C))          # [P, C^2]
            idt, okt = torch.tensor(ids), torch.tensor(ok)
            mt = torch.where(okt[:, None], m2[idt], zero)
            ct = torch.where(okt[:, None], c2[idt], torch.tensor([1.0, 0.0, 0.0, 1.0], dtype=torch.float64))
            at = torch.where(okt, a_eff[idt], zero)
            xt, yt = torch.tensor(px)[:, None] - mt[None, :, 0], torch.tensor(py)[:, None] - mt[None, :, 1]
            qt = (xt * ct[:, 3] - yt * ct[:, 2]) * xt + (yt * ct[:, 0] - xt * ct[:, 1]) * yt
            rt = qt / (ct[:, 0] * ct[:, 3] - ct[:, 1] * ct[:, 2])
            f = torch.where(torch.tensor(take), at[None] * torch.exp(-0.5 * torch.clamp(rt, min=0.0)), zero)
            cp = torch.cumprod(1 - f, 1)
            Tb = torch.cat([torch.ones((len(px), 1), dtype=torch.float64), cp[:, :-1]], 1)
            colour = torch.sigmoid(torch.einsum("pk,eck->pec", Y, sh[idt]))                        # [P,E,3]
            if basis == "poly":
                assert C == 4
                V, M = poly_tile(view, t)
                ratio = bound_ratio(a["sh"][ids], view)
                beyond = ~(ratio <= 1.0)                                   # (NaN: beyond)
                Wn = np.einsum("rk,eck->ecr", V, np.nan_to_num(a["sh"][ids].astype(np.float64)))
                tr = taylor_ratio(Wn)
                assert (LOG2E * np.abs(Wn).sum(-1)[~beyond] <= 32.0).all()   # (no row near the kernels' |s| <= 40 rescue)
                kind = np.where(beyond, 2, np.where((tr <= 1.0).all(1), 0, 1))
                if mode == "view":
                    whole = not bool(np.nanmax(bound_ratio(a["sh"], view)) <= 1.0) or not np.isfinite(a["sh"]).all()
                elif mode == "tile":
                    whole = bool(beyond.any())
                else:
                    whole = fallback and any(alive_any[b] and 4 * int(beyond[b:b + 32].sum()) > len(beyond[b:b + 32]) for b in range(0, len(ids), 32))
                if whole:
                    kind[:] = 2
                tiers[v][t] = dict(kind=kind, whole=whole)
                edges["bound"] += [float(x) for x in ratio if np.isfinite(x)]
                edges["taylor"] += [float(x) for x in tr[~beyond].reshape(-1)]
                Vt, Mt = torch.tensor(V), torch.tensor(M)
                Wt = torch.einsum("rk,eck->ecr", Vt, sh[idt])                                      # [E,3,6]
                f0 = torch.sigmoid(Wt[..., 0])
                d1 = f0 * (1 - f0)
                Lp = torch.einsum("pr,ecr->pec", Mt[:, 1:3], Wt[..., 1:3]); Qp = torch.einsum("pr,ecr->pec", Mt[:, 3:], Wt[..., 3:])
                taylor = f0[None] + d1[None] * (Lp + Qp) + (0.5 * d1 * (1 - 2 * f0))[None] * Lp * Lp
                logit = torch.sigmoid(torch.einsum("pr,ecr->pec", Mt, Wt))
                kt = torch.tensor(kind)[None, :, None]
                colour = torch.where(kt == 0, taylor, torch.where(kt == 1, logit, colour))
            acc = torch.einsum("pe,pec->pc", Tb * f, colour) + cp[:, -1:] * bg[None]
            loss = loss + (gop * acc).sum()
            Tn = cp[:, -1].detach().numpy()
            assert np.abs(Tn - T).max() <= 1e-12
            im[ys, xs] = acc.detach().numpy(); Tim[ys, xs] = Tn
        img.append(im); Ts.append(Tim)
    flat = [sh, alpha] + leaves["gm"] + leaves["gc"]
    g = torch.autograd.grad(loss, flat, allow_unused=True)
    g = [np.zeros(tuple(x.shape)) if y is None else y.numpy() for x, y in zip(flat, g)]
    grads = dict(gsh=g[0], ga=g[1], gm=g[2:2 + B], gc=g[2 + B:])
    return dict(img=img, T=Ts, grads=grads, take=takes, dead=deads, margins=margins, N=N, tiers=tiers, edges=edges)


def grad_ratios(got, want):
    """scenes.per_gaussian_grad_error (rtol 1e-3, atol 1e-5; <= 1 passes) per gradient tensor, the worse view"""
    N = len(want["ga"])
    out = dict(gsh=scenes.per_gaussian_grad_error(np.asarray(got["gsh"]).reshape(N, -1), want["gsh"].reshape(N, -1))[0],
               ga=scenes.per_gaussian_grad_error(got["ga"], want["ga"])[0])
    for k in ("gm", "gc"):
        out[k] = max(scenes.per_gaussian_grad_error(np.asarray(g).reshape(N, -1), w.reshape(N, -1))[0] for g, w in zip(got[k], want[k]))
    return out


def oracle_chain(case, C=4):
    """the reference's own fp32 arithmetic on the same lists (oracle.render_sh_fwd / render_sh_bwd), dropped records left out of
    the lists: its CUDA tests none of it and would hand NaN on"""
    from oracle import oracle as O
    lists = [[[i for i in lst if i not in case.bad] for lst in case.lists[v]] for v in range(B)]
    a = case.arrays(C, lists)
    N = a["N"]
    clean = lambda x: np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)  # noqa: E731
    sh, al = clean(a["sh"]), clean(a["alpha"])
    out = dict(gsh=np.zeros((N, 3, C * C)), ga=np.zeros(N), gm=[], gc=[], img=[], T=[])
    for view in a["views"]:
        m2, c2 = clean(view["m2"]), clean(view["c2"]).reshape(N, 2, 2)
        lst = (view["st"], view["en"], view["ids"])
        img, T = O.render_sh_fwd(m2, c2, sh, al, *lst, view["tlp"], view["rot"], C, view["ps"][0], view["ps"][1], H, W, THRESH, bg=view["bg"],
                                 want_T=True)
        empty = np.repeat(np.repeat((view["lens"] == 0).reshape(NTH, NTW), 16, 0), 16, 1)[:H, :W]
        img = np.where(empty[..., None], view["bg"], img)        # (the reference leaves empty tiles to the caller)
        gm, gc, gsh, ga = O.render_sh_bwd(m2, c2, sh, al, *lst, img, view["go"], view["tlp"], view["rot"], C, view["ps"][0], view["ps"][1], H, W,
                                          THRESH)
        out["gsh"] += gsh; out["ga"] += ga
        out["gm"].append(gm.astype(np.float64)); out["gc"].append(gc.reshape(N, 4).astype(np.float64))
        out["img"].append(img); out["T"].append(T.reshape(H, W))
    return out


def image_ratio(got, ref, bar):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / (bar * max(1.0, float(np.abs(ref).max()))))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

def case_len(n, tile):
    def make():
        S = Scene()
        S.front(tile, S.thin(tile, n), replace=True)      # the list IS these n entries: the staging rounds end where it does
        return S

    def check(S, ref):
        for v in range(B):
            assert len(S.lists[v][tile]) == n and ref["take"][v][tile].any(0).all() and not ref["dead"][v][tile]
    return make, check


def saturating(n_thin, n_behind, seed):
    """n_thin thin splats, nine layers of alpha 0.65 and sigma 4000 pixels (0.35^9 = 7.9e-5 < thresh <= 0.35^8; 1 / (1 - a G) < 3),
    n_behind entries of alpha 0.3 that nobody may touch -- in the middle tile, in front of its own entries: the tile's last live
    pixel dies on list entry n_thin + 9"""
    def make():
        S = Scene()
        S.rng = np.random.default_rng(seed)
        front = S.thin(MID, n_thin) + [S.add_px(24.0 + k, 23.0 - k, 4000.0, 0.65) for k in range(9)]
        behind = [S.add_px(16 + S.rng.uniform(0, 16), 16 + S.rng.uniform(0, 16), 4.0, 0.3) for _ in range(n_behind)]
        S.zero = list(behind)
        S.front(MID, front + behind)
        return S

    def check(S, ref):
        for v in range(B):
            assert last_taken(ref, v, MID) == n_thin + 9 and ref["dead"][v][MID], (v, last_taken(ref, v, MID))
            assert not ref["take"][v][MID][:, n_thin + 9:].any()
            assert len(S.lists[v][MID]) >= n_thin + 9 + n_behind
    return make, check


def case_sat_partial():
    def make():
        S = Scene()
        S.rng = np.random.default_rng(21)
        front = S.thin(MID, 20) + [S.add_px(24.0 + 0.25 * k, 24.0 - 0.125 * k, 5.0, 0.65) for k in range(14)]
        S.front(MID, front + S.thin(MID, 150 - 34), replace=True)
        return S

    def check(S, ref):
        for v in range(B):
            take = ref["take"][v][MID]
            assert take.shape[1] == 150
            lastpix = np.array([np.nonzero(r)[0][-1] if r.any() else -1 for r in take])
            assert (lastpix < 40).sum() >= 16 and (lastpix >= 140).sum() >= 16, np.bincount(lastpix + 1)
            wave = lastpix.reshape(16, 16)[0:4]          # rows 0..3: both kinds of pixel inside the one wavefront
            assert not ref["dead"][v][MID] and take[:, -1].any() and wave.max() >= 140 and lastpix.min() < 40
    return make, check


def case_unseen_round():
    """entries 32..127 of the middle tile's list have no taker: the staged rounds 1, 2 and 3 of 32 (the polynomial forward, every
    backward) and round 1 of 64 (the exact forwards), between rounds that have takers"""
    def make():
        S = Scene()
        S.rng = np.random.default_rng(5)
        seen = S.thin(MID, 32)
        # centred 6 pixels inside the tile to the LEFT (sigma 2 pixels, alpha 0.04: a G <= 4.5e-4 from 6 pixels on), listed here only
        unseen = [S.add_px(10.0, 16.0 + (k % 16) + 0.5, 2.0, 0.04) for k in range(96)]
        S.zero = list(unseen)
        S.front(MID, seen + unseen + S.thin(MID, 20))
        return S

    def check(S, ref):
        for v in range(B):
            anyone = ref["take"][v][MID].any(0)
            assert not anyone[32:128].any() and anyone[:32].all() and anyone[128:148].all() and not ref["dead"][v][MID]
    return make, check


def case_guard_trip():
    def make():
        S = Scene()
        trip = []
        for gx, gy, side in ((5, 6, +1.0), (9, 3, -1.0)):
            means = [S.pixel(v, gx + 2.25, gy - 1.5) for v in range(B)]
            covs = [iso(S.sigma(v, 2.5)) for v in range(B)]
            G, _ = gauss64(means[0], covs[0], S.pixel(0, gx, gy))
            i = S.add(means, covs, K_MIN / G * (1.0 + side * 5e-5))
            rel = float(S.alpha[i]) * gauss64(S.m2[0][i], S.c2[0][i], S.pixel(0, gx, gy))[0] / K_MIN - 1.0
            assert side * rel > 0 and abs(rel) < 0.5 * GUARD_TOL     # inside half the guard's window, one on each side
            trip.append((i, gx, gy, side))
        S.front(0, [i for i, *_ in trip])
        S.note["trip"] = trip
        return S

    def check(S, ref):
        for k, (i, gx, gy, side) in enumerate(S.note["trip"]):
            assert bool(ref["take"][0][0][gy * 16 + gx, k]) == (side > 0)
    return make, check


def case_non_psd():
    """det > 0, indefinite symmetric part: the form is negative on a wedge of pixels (G = 0 there) and the record contributes
    outside it; a faint second one whose RAW exponential of the negative form, beyond 1, would sit on the skip threshold"""
    def make():
        S = Scene()
        covs = [NON_PSD * S.sigma(v, 5.0) ** 2 for v in range(B)]
        means = [S.pixel(v, 10.0 + FRAC[0], 9.0 + FRAC[1]) for v in range(B)]
        i0 = S.add(means, covs, 0.8)
        raw = [(gauss64(means[0], covs[0], S.pixel(0, gx, gy)), (gx, gy)) for gx in range(16) for gy in range(16)]
        neg = [(g, p) for (g, q), p in raw if q < 0 and 1.5 < g < 50.0]
        assert neg
        i1 = S.add(means, covs, K_MIN / neg[0][0] * (1.0 + 1e-5))
        S.note.update(i0=i0, i1=i1, asymmetric=(i0, i1), wedge=[p for (g, q), p in raw if q < 0], out=[p for (g, q), p in raw if q > 0])
        S.front(0, [i0, i1])
        return S

    def check(S, ref):
        take = ref["take"][0][0][:, 0]
        assert S.note["wedge"] and not any(take[gy * 16 + gx] for gx, gy in S.note["wedge"])
        assert sum(take[gy * 16 + gx] for gx, gy in S.note["out"]) >= 16
        assert not any(ref["take"][0][0][gy * 16 + gx, 1] for gx, gy in S.note["wedge"])
    return make, check


def case_clamp_straddle():
    def make():
        S = Scene()
        ids = [S.add_px(18.0 + FRAC[0] + 4 * k, 19.0 + FRAC[1] + 3 * k, 3.0, al) for k, al in enumerate((0.98999, 0.99, 0.99001, 1.0))]
        S.note["ids"] = ids
        S.front(MID, S.thin(MID, 5) + ids)
        return S

    def check(S, ref):
        al = [float(S.alpha[i]) for i in S.note["ids"]]
        assert al[0] < np.float32(ALPHA_CLAMP) == al[1] < al[2] < al[3] == 1.0
        for v in range(B):
            assert all(ref["take"][v][MID][:, 5 + k].any() for k in range(4))
    return make, check


BAD_KINDS = ("det_zero", "det_negative", "nan_mean_x", "inf_mean_x", "nan_mean_y", "inf_mean_y", "nan_cov", "inf_cov", "nan_cov_row",
             "nan_alpha", "inf_alpha", "neg_inf_alpha", "zero_alpha", "neg_alpha", "nan_sh")


def case_bad_records():
    """one record of each kind of BAD_KINDS, interleaved with ordinary ones, in the first AND in the second staged round (of 32 and
    of 64: entries 0..29 and 64..93 of the middle tile's list)"""
    def make():
        S = Scene()
        S.rng = np.random.default_rng(17)
        s2 = [S.sigma(v, 5.0) ** 2 for v in range(B)]
        at = lambda gx, gy: [S.pixel(v, gx, gy) for v in range(B)]  # noqa: E731
        good = [iso(S.sigma(v, 5.0)) for v in range(B)]
        nan, inf = np.float32("nan"), np.float32("inf")

        def cov_with(val, k):
            out = []
            for c in good:
                c = c.copy().reshape(4); c[k] = val
                out.append(c.reshape(2, 2))
            return out

        def one_round(tag):
            p = lambda: (16 + float(S.rng.uniform(2, 14)), 16 + float(S.rng.uniform(2, 14)))  # noqa: E731
            sh_nan = S.rand_sh(); sh_nan[1, 5] = nan
            recs = dict(det_zero=S.add(at(*p()), [np.array([[1.0, 1.0], [1.0, 1.0]], np.float32) * s for s in s2], 0.5),
                        det_negative=S.add(at(*p()), [np.array([[1.0, 2.0], [2.0, 1.0]], np.float32) * s for s in s2], 0.5),
                        nan_mean_x=S.add([(nan, m[1]) for m in at(*p())], good, 0.5),
                        inf_mean_x=S.add([(inf, m[1]) for m in at(*p())], good, 0.5),
                        nan_mean_y=S.add([(m[0], nan) for m in at(*p())], good, 0.5),
                        inf_mean_y=S.add([(m[0], -inf) for m in at(*p())], good, 0.5),
                        nan_cov=S.add(at(*p()), cov_with(nan, 1), 0.5),
                        inf_cov=S.add(at(*p()), cov_with(inf, 3), 0.5),
                        nan_cov_row=S.add(at(22.0, 24.0), cov_with(nan, 0), 0.5),      # its centre ON a pixel row: y = 0 occurs
                        nan_alpha=S.add(at(*p()), good, nan),
                        inf_alpha=S.add(at(*p()), good, inf),
                        neg_inf_alpha=S.add(at(*p()), good, -inf),
                        zero_alpha=S.add(at(*p()), good, 0.0),
                        neg_alpha=S.add(at(*p()), good, -0.5),
                        nan_sh=S.add([(nan, m[1]) for m in at(*p())], good, 0.5, sh=sh_nan))
            assert tuple(recs) == BAD_KINDS
            S.note[tag] = recs
            order = []
            for i, thin in zip(recs.values(), S.thin(MID, len(recs))):
                order += [i, thin]
            return order
        first = one_round("first")
        between = S.thin(MID, 64 - len(first))
        second = one_round("second")
        dropped = [i for tag in ("first", "second") for k, i in S.note[tag].items() if k not in ("zero_alpha", "neg_alpha")]
        S.bad = list(dropped)
        S.zero = [i for tag in ("first", "second") for i in S.note[tag].values()]      # (alpha <= 0: a G <= 0 < 1 / 255, never taken)
        S.front(MID, first + between + second)
        return S

    def check(S, ref):
        for v in range(B):
            lst = S.lists[v][MID]
            for tag, lo in (("first", 0), ("second", 64)):
                for name, i in S.note[tag].items():
                    k = lst.index(i)
                    assert lo <= k < lo + 32 and not ref["take"][v][MID][:, k].any(), (tag, name)
            good = [k for k, i in enumerate(lst[:94]) if i not in S.zero]
            assert ref["take"][v][MID][:, good].any(0).all() and not ref["dead"][v][MID]
        for g in (ref["grads"]["gsh"], ref["grads"]["ga"], *ref["grads"]["gm"], *ref["grads"]["gc"]):
            assert not g[S.zero].any() and np.isfinite(g).all()
    return make, check


def case_empty_tiles():
    def make():
        S = Scene()
        for t in (1, 5, CORNER):
            S.front(t, [], replace=True)
        return S

    def check(S, ref):
        for v in range(B):
            for t in (1, 5, CORNER):
                ys, xs, _, _ = tile_pixels(S.arrays()["views"][v], t)
                assert (ref["img"][v][ys, xs] == S.bg.astype(np.float64)).all() and (ref["T"][v][ys, xs] == 1).all()
    return make, check


def case_big_bands():
    """coefficients of order 1 in every band, with different signs per channel: one wrong constant or sign in the basis moves
    pixels by far more than the bar"""
    def make():
        S = Scene()
        S.rng = np.random.default_rng(41)
        ids = []
        for k in range(16):
            row = S.rng.uniform(0.6, 1.4, (3, 16)) * np.where(S.rng.integers(0, 2, (3, 16)) > 0, 1.0, -1.0)
            row[:, k] = np.abs(row[:, k]) * np.array([1.0, -1.0, 1.0])     # coefficient k of splat k: signs + - + over the channels
            ids += S.thin(MID, 1, alpha=0.25, sigma_px=6.0, sh=row)
        S.note["ids"] = ids
        S.front(MID, ids)
        return S

    def check(S, ref):
        for v in range(B):
            assert ref["take"][v][MID][:, :16].any(0).all()
        sh = np.stack([S.sh[i] for i in S.note["ids"]])
        assert (np.abs(sh) >= 0.6).all() and all((np.sign(sh[k, :, k]) == (1, -1, 1)).all() for k in range(16))
    return make, check


def case_flagged(n_beyond):
    """n_beyond of the first 32 entries of the middle tile's list have row sums far beyond the polynomial form's coefficient bound
    (>= 1.25 x): more than a quarter of a staged batch of 32 (9) sends the tile to the exact fallback, fewer (7) leave those
    entries to the per-entry exact tier"""
    def make():
        S = Scene()
        S.rng = np.random.default_rng(9 + n_beyond)
        beyond = []
        for _ in range(n_beyond):
            row = S.rng.normal(0, 0.3, (3, 16)); row[:, 9:] = 0.6 * np.sign(S.rng.normal(size=(3, 7)))
            beyond += S.thin(MID, 1, alpha=0.2, sh=row)
        thin = S.thin(MID, 32 - n_beyond)
        order = []
        for k in range(32):      # spread through the round
            order.append(beyond.pop() if beyond and (k % 3 == 1) else thin.pop() if thin else beyond.pop())
        S.note.update(beyond=[i for i in order if np.abs(S.sh[i][:, 1:]).sum(1).max() > 1.0], n=n_beyond)
        S.front(MID, order)
        return S

    def check(S, ref):
        assert len(S.note["beyond"]) == n_beyond
        for i in range(len(S.alpha)):
            s = float(np.abs(S.sh[i][:, 1:]).sum(1).max())
            assert s >= 1.25 * 2.61 if i in S.note["beyond"] else s <= 0.8 * POLY_BOUND_ROW, (i, s)   # (2.61: the bound at fx = 440)
        for v in range(B):
            assert sum(i in S.note["beyond"] for i in S.lists[v][MID][:32]) == n_beyond and ref["take"][v][MID][:, :32].any(0).all()
    return make, check


def case_taylor_edge():
    """eight splats whose red row sits at <= 0.8 x the Taylor limit in both views (the colour quadratic, with its f'' L^2 terms at their
    largest) and eight at >= 1.25 x (the sigmoid of the quadratic logit), all within the coefficient bound: one coefficient, k = 15,
    whose fitted linear part is the largest of the sixteen in the middle tile (0.031 / 0.025 per unit in the two views)"""
    def make():
        S = Scene()
        S.rng = np.random.default_rng(23)
        hit, miss = [], []
        for k in range(16):
            row = S.rand_sh(high=0.0)
            row[0, 15] = (0.45 if k % 2 else 0.8) * (1.0 if k % 4 < 2 else -1.0)      # 0.62 x / 1.5 x the limit in the view nearer to it
            (hit if k % 2 else miss).extend(S.thin(MID, 1, alpha=0.2, sigma_px=6.0, sh=row))
        S.note.update(hit=hit, miss=miss)
        S.front(MID, [i for pair in zip(hit, miss) for i in pair])
        return S

    def check(S, ref):
        for v in range(B):
            assert ref["take"][v][MID][:, :16].any(0).all()
    return make, check


def check_taylor_edge_tiers(S, model):
    for v in range(B):
        kind = model["tiers"][v][MID]["kind"]
        lst = S.lists[v][MID]
        assert all(kind[lst.index(i)] == 0 for i in S.note["hit"]) and all(kind[lst.index(i)] == 1 for i in S.note["miss"]), kind[:16]


CASES = {}
for _n in (1, 31, 32, 33, 63, 64, 65, 96, 97, 257):
    CASES[f"len_{_n}"] = case_len(_n, MID)
    CASES[f"len_{_n}_corner"] = case_len(_n, CORNER)
CASES.update(sat_entry_32=saturating(23, 40, 11), sat_entry_33=saturating(24, 40, 12), sat_entry_64=saturating(55, 40, 13),
             sat_entry_65=saturating(56, 40, 14), sat_in_first_round=saturating(3, 40, 15), sat_partial=case_sat_partial(),
             unseen_round=case_unseen_round(), guard_trip=case_guard_trip(), non_psd=case_non_psd(), clamp_straddle=case_clamp_straddle(),
             bad_records=case_bad_records(), empty_tiles=case_empty_tiles(), big_bands=case_big_bands(), taylor_edge=case_taylor_edge(),
             flagged_tile_7=case_flagged(7), flagged_tile_9=case_flagged(9))
LOW_BAND_CASES = ("len_33", "len_65", "sat_entry_33", "bad_records", "big_bands")      # C = 1, 2, 3 through the exact launches
MODES = ("view", "tile", "entry", "entry no_fallback")      # `reference(basis="poly")`: which launches decide what
_BUILT = {}


def build(name, C=4):
    """the case, its reference and the oracle's ratios -- once per process; every condition the case is named for is asserted here, on
    the reference and the oracle alone, before any kernel is looked at"""
    if (name, C) not in _BUILT:
        make, check = CASES[name]
        S = make()
        ref = reference(S, C)
        if name != "guard_trip":
            assert ref["margins"]["skip"] >= MARGIN and ref["margins"]["stop"] >= MARGIN, (name, ref["margins"])
        for v in range(B):      # one tile per (view, splat)
            flat = [i for lst in S.lists[v] for i in lst]
            assert len(flat) == len(set(flat))
        check(S, ref)
        orc = oracle_chain(S, C)
        for i in S.note.get("asymmetric", ()):      # (module docstring, WHERE THE REFERENCE GIVES WAY)
            for v in range(B):
                ref["grads"]["gm"][v][i] = orc["gm"][v][i]; ref["grads"]["gc"][v][i] = orc["gc"][v][i]
        ratios = grad_ratios(orc, ref["grads"])
        ratios["img"] = max(image_ratio(orc["img"][v], ref["img"][v], EXACT_BAR) for v in range(B))
        ratios["T"] = max(image_ratio(orc["T"][v], ref["T"][v], EXACT_BAR) for v in range(B))
        print(f"[sh cases] build {name} C={C}: margins skip {ref['margins']['skip']:.2e} stop {ref['margins']['stop']:.2e}; oracle "
              + " ".join(f"{k}={x:.3f}" for k, x in ratios.items()))
        assert max(ratios.values()) <= ORACLE_SHARE, (name, ratios)      # the inputs are fair: the reference's fp32 arithmetic has room
        models = {}
        for mode in (MODES if C == 4 else ()):
            m = reference(S, C, basis="poly", mode=mode.split()[0], fallback=not mode.endswith("no_fallback"))
            for i in S.note.get("asymmetric", ()):
                for v in range(B):
                    m["grads"]["gm"][v][i] = orc["gm"][v][i]; m["grads"]["gc"][v][i] = orc["gc"][v][i]
            for k, xs in m["edges"].items():      # every tier decision clear of its edge
                assert all(x <= EDGE_LO or x >= EDGE_HI for x in xs), (name, mode, k, [x for x in xs if EDGE_LO < x < EDGE_HI])
            share = grad_ratios(m["grads"], ref["grads"])
            share["img"] = max(image_ratio(m["img"][v], ref["img"][v], EXACT_BAR) for v in range(B))      # DESIGN's promise: colours within 1e-5
            assert max(share.values()) <= 1.0 and max(share[k] for k in ("gsh", "ga", "gm", "gc")) <= ORACLE_SHARE, (name, mode, share)
            assert all(np.array_equal(m["T"][v], ref["T"][v]) for v in range(B))
            models[mode] = m
        if models:
            print(f"[sh cases] build {name}: poly model (entry, no fallback) against the exact one " + " ".join(f"{k}={x:.3f}" for k, x in share.items()))
        if name == "taylor_edge":
            for m in models.values():
                check_taylor_edge_tiers(S, m)
        if name.startswith("flagged_tile"):
            n = S.note["n"]
            assert all(models["entry"]["tiers"][v][MID]["whole"] == (n > 8) and models["tile"]["tiers"][v][MID]["whole"] for v in range(B))
            assert not any(models["entry no_fallback"]["tiers"][v][MID]["whole"] for v in range(B))
            assert all((models["entry no_fallback"]["tiers"][v][MID]["kind"][:32] == 2).sum() == n for v in range(B))
        _BUILT[(name, C)] = (S, ref, ratios, models)
    return _BUILT[(name, C)]


# ---- launches --------------------------------------------------------------------------------------------------------------------

def device_inputs(L, S, C=4):
    a = S.arrays(C)
    N = a["N"]
    d = dict(N=N, C=C, sh=L.to_dev(a["sh"]), al=L.to_dev(a["alpha"]), rows=L.to_dev(np.zeros(N, np.float32)), l1=L.to_dev(np.zeros(1, np.float32)),
             big=L.to_dev(np.full(1, 1.0e3, np.float32)), views=a["views"])
    L.lib.sh_l1_bound_rows(N, d["sh"].p, C, d["l1"].p, d["rows"].p, L.stream)
    L.sync()
    order = np.random.default_rng(2).permutation(NT).astype(np.int32)      # (uint32 on the device: the same bits)
    d["dev"] = [{k: L.to_dev(v[k]) for k in ("m2", "c2", "st", "en", "ids", "tlp", "rot", "go", "bg", "psd")} for v in a["views"]]
    d["order"] = L.to_dev(order)
    return d


def expand_moments(view, gm, gc):
    """moments -> gradients as the projection backward expands them (geometry.hip, moments_to_grads_sh), in fp64"""
    c = view["c2"]
    with np.errstate(all="ignore"):
        det = (c[:, 0] * c[:, 3] - c[:, 1] * c[:, 2]).astype(np.float64)
    det = np.where(np.isfinite(det) & (det > 0), det, 1.0)
    m = gc.astype(np.float64); h = 0.5 / det ** 2
    return gm.astype(np.float64) / det[:, None], np.stack([h * m[:, 0], h * m[:, 1], h * m[:, 1], h * m[:, 2]], 1)


def run_camera(L, d, form, nseg=0):
    """one view at a time through gsgen_vol_render_sh{,_ordered,_segmented,_bounded,_routed} and its backward.  out / T arrive
    holding SENT_IMG / SENT_T: given a background these entry points show it in an empty tile (the reference's _with_bg forms) and
    leave that tile's T to the caller (both asserted), who would have put 1 there."""
    lib, N, C = L.lib, d["N"], d["C"]
    sfx = "" if form == "plain" else "_" + form
    fwd, bwd = getattr(lib, "vol_render_sh" + sfx), getattr(lib, "vol_render_backward_sh" + sfx)
    gsh, ga = L.to_dev(np.zeros((N, 3, C * C), np.float32)), L.to_dev(np.zeros(N, np.float32))
    r = dict(img=[], T=[], gm=[], gc=[])
    for v, dv in zip(d["views"], d["dev"]):
        seg = L.to_dev(np.zeros(lib.segment_workspace_bytes(NT, nseg), np.uint8)) if nseg > 1 else None
        segp = seg.p if seg is not None else None
        extra = dict(plain=(), ordered=(d["order"].p,), segmented=(d["order"].p if nseg == 3 else None, segp, nseg),
                     bounded=(None, segp, nseg, d["l1"].p), routed=(None, segp, nseg, d["l1"].p, d["rows"].p))[form]
        head = (N, v["D"], dv["m2"].p, dv["c2"].p, d["sh"].p, d["al"].p, dv["st"].p, dv["en"].p, dv["ids"].p)
        geo = (dv["tlp"].p, dv["rot"].p, 16, NTH, NTW, v["ps"][0], v["ps"][1], H, W, C, THRESH, dv["bg"].p)
        out, T = L.to_dev(np.full((H, W, 3), SENT_IMG, np.float32)), L.to_dev(np.full((H, W), SENT_T, np.float32))
        gm, gc = L.to_dev(np.zeros((N, 2), np.float32)), L.to_dev(np.zeros((N, 4), np.float32))
        fwd(*head, out.p, *geo, T.p, *extra, L.stream)
        bwd(*head, out.p, gm.p, gc.p, gsh.p, ga.p, dv["go"].p, *geo, *extra, L.stream)
        L.sync()
        img, Tt = out.get(), T.get()
        for t in np.nonzero(v["lens"] == 0)[0]:
            ys, xs, _, _ = tile_pixels(v, t)
            assert (img[ys, xs] == v["bg"]).all() and (Tt[ys, xs] == SENT_T).all(), (form, t)
            Tt[ys, xs] = 1.0
        r["img"].append(img); r["T"].append(Tt); r["gm"].append(gm.get()); r["gc"].append(gc.get())
    r["gsh"], r["ga"] = gsh.get(), ga.get()
    return r


def run_batch(L, d, form, nseg=0, moments=False, psd=False, bound="l1", no_fallback=0):
    """gsgen_vol_render_sh_batch{,_bounded,_routed} and its backward (the routed one plain or in the moment form): out / T arrive
    holding 9, the batched forward writes every pixel"""
    from gsgen_amd._capi import ShView
    lib, N, C = L.lib, d["N"], d["C"]
    arr = (ShView * B)()
    outs = []
    for a, v, dv in zip(arr, d["views"], d["dev"]):
        o = dict(out=L.to_dev(np.full((H, W, 3), 9.0, np.float32)), T=L.to_dev(np.full((H, W), 9.0, np.float32)),
                 gm=L.to_dev(np.zeros((N, 2), np.float32)), gc=L.to_dev(np.zeros((N, 4), np.float32)),
                 seg=L.to_dev(np.zeros(lib.segment_workspace_bytes(NT, nseg), np.uint8)) if nseg > 1 else None)
        a.mean, a.cov, a.start, a.end, a.gaussian_ids = dv["m2"].p, dv["c2"].p, dv["st"].p, dv["en"].p, dv["ids"].p
        a.tile_order, a.topleft, a.c2w, a.bg_rgb = None, dv["tlp"].p, dv["rot"].p, dv["bg"].p
        a.pixel_size_x, a.pixel_size_y = (0.0, 0.0) if psd else v["ps"]      # (with pixel_size_dev the floats are ignored)
        a.pixel_size_dev = dv["psd"].p if psd else None
        a.out, a.T, a.grad_out, a.grad_mean, a.grad_cov = o["out"].p, o["T"].p, dv["go"].p, o["gm"].p, o["gc"].p
        a.segment_workspace = o["seg"].p if nseg > 1 else None
        a.route_report, a.no_fallback = None, no_fallback
        outs.append(o)
    bws = L.to_dev(np.zeros(lib.sh_batch_workspace_bytes_routed(B, NT), np.uint8))
    gsh, ga = L.to_dev(np.zeros((N, 3, C * C), np.float32)), L.to_dev(np.zeros(N, np.float32))
    geo = (16, NTH, NTW, H, W, C, THRESH, nseg)
    bnd = d[bound].p
    extra = dict(batch=(), batch_bounded=(bnd,), batch_routed=(bnd, d["rows"].p))[form]
    getattr(lib, "vol_render_sh_" + form)(B, arr, N, d["sh"].p, d["al"].p, *geo, *extra, bws.p, L.stream)
    bwd = getattr(lib, "vol_render_backward_sh_" + form + ("_moments" if moments else ""))
    bwd(B, arr, N, d["sh"].p, d["al"].p, gsh.p, ga.p, *geo, *extra, bws.p, L.stream)
    L.sync()
    r = dict(img=[o["out"].get() for o in outs], T=[o["T"].get() for o in outs], gm=[o["gm"].get() for o in outs],
             gc=[o["gc"].get() for o in outs], gsh=gsh.get(), ga=ga.get())
    if moments:
        for i, v in enumerate(d["views"]):
            r["gm"][i], r["gc"][i] = expand_moments(v, r["gm"][i], r["gc"][i])
    r["flags"] = bws.get()[lib.sh_batch_workspace_bytes(B):][:B * NT].reshape(B, NT).copy()
    return r


# (name, runner, arguments, the poly model's mode where the launch may take the polynomial basis)
FORMS_C4 = (
    ("camera", run_camera, dict(form="plain"), None),
    ("camera ordered", run_camera, dict(form="ordered"), None),
    ("camera segmented 2", run_camera, dict(form="segmented", nseg=2), None),
    ("camera segmented 3", run_camera, dict(form="segmented", nseg=3), None),
    ("camera bounded", run_camera, dict(form="bounded"), "view"),
    ("camera routed", run_camera, dict(form="routed"), "tile"),
    ("batch", run_batch, dict(form="batch"), None),
    ("batch segments 2", run_batch, dict(form="batch", nseg=2), None),
    ("batch psd", run_batch, dict(form="batch", psd=True), None),
    ("batch bounded", run_batch, dict(form="batch_bounded"), "view"),
    ("batch bounded fallback", run_batch, dict(form="batch_bounded", bound="big"), None),
    ("batch routed", run_batch, dict(form="batch_routed"), "entry"),
    ("batch routed segments 2", run_batch, dict(form="batch_routed", nseg=2), "entry"),
    ("batch routed moments", run_batch, dict(form="batch_routed", moments=True), "entry"),
    ("batch routed moments segments 2", run_batch, dict(form="batch_routed", moments=True, nseg=2), "entry"),
    ("batch routed psd", run_batch, dict(form="batch_routed", psd=True), "entry"),
)
FORMS_LOW = (("camera", run_camera, dict(form="plain"), None), ("batch", run_batch, dict(form="batch"), None))
# bit for bit, images and T (module docstring): (form, the form it must equal)
SAME_BITS = (("batch", "camera segmented 2"), ("batch segments 2", "batch"), ("batch psd", "batch"), ("batch routed", "camera routed"),
             ("batch routed segments 2", "batch routed"), ("batch routed moments", "batch routed"), ("batch routed psd", "batch routed"),
             ("batch bounded fallback", "batch"), ("camera segmented 3", "camera segmented 2"))


def check_run(L, name, what, r, ref, zero, model=None):
    bar = POLY_BAR if model is not None else EXACT_BAR
    fig = {}
    for v in range(B):
        for k in ("img", "T"):
            assert np.isfinite(r[k][v]).all(), (name, what, k, v)
            fig[k] = max(fig.get(k, 0.0), image_ratio(r[k][v], ref[k][v], bar))
    for k in ("gsh", "ga", "gm", "gc"):
        for arr in (r[k] if isinstance(r[k], list) else [r[k]]):
            assert np.isfinite(arr).all(), (name, what, k)
            if len(zero):
                assert not np.asarray(arr)[zero].any(), (name, what, k)        # exactly zero: == 0, no tolerance
    fig.update(grad_ratios(r, ref["grads"]))
    if model is not None:      # the polynomial launches against their own model too: the tighter of the two
        for k in ("img", "T"):
            fig["model " + k] = max(image_ratio(r[k][v], model[k][v], EXACT_BAR) for v in range(B))
        fig.update({"model " + k: x for k, x in grad_ratios(r, model["grads"]).items()})
    print(f"[sh cases] {L.kind} {name} {what}: " + " ".join(f"{k}={x:.3f}" for k, x in fig.items()))
    assert max(fig.values()) <= 1.0, (name, what, fig)
    return fig


def check_case(L, name, C=4):
    """one case through all its launch forms: images and T against the reference, every gradient tensor against the reference, the
    rows that must be exactly zero, the forwards bit for bit where the project documents it"""
    S, ref, _, models = build(name, C)
    d = device_inputs(L, S, C)
    zero = np.asarray(sorted(set(S.zero)), np.int64)
    runs, worst = {}, 0.0
    for what, fn, kw, mode in (FORMS_C4 if C == 4 else FORMS_LOW):
        runs[what] = fn(L, d, **kw)
        worst = max(worst, max(check_run(L, name, f"C={C} {what}", runs[what], ref, zero, models[mode] if mode else None).values()))
    if C == 4:
        with np.errstate(all="ignore"):      # every listed splat within the coefficient bound: batch and camera route alike
            rows = np.abs(np.stack(S.sh)[sorted({i for v in range(B) for lst in S.lists[v] for i in lst})][:, :, 1:]).sum(2).max(1)
        within = bool(np.isfinite(rows).all() and rows.max() <= 0.8 * POLY_BOUND_ROW)
        for a, b in SAME_BITS:
            if (a, b) == ("batch routed", "camera routed") and not within:
                continue      # (a splat beyond it: the per-camera launch renders its TILE exactly, the batch the ENTRY -- gsgen_hip.h)
            for v in range(B):
                for k in ("img", "T"):
                    assert np.array_equal(runs[a][k][v], runs[b][k][v]), (name, a, b, k, v, float(np.abs(runs[a][k][v] - runs[b][k][v]).max()))
        if name.startswith("flagged_tile"):
            n = S.note["n"]
            flags = runs["batch routed"]["flags"]
            assert (flags[:, MID] == (1 if n > 8 else 0)).all() and flags.sum() == (B if n > 8 else 0), flags
            for moments in (False, True):     # ... and kept in the polynomial kernel: the per-entry exact tier
                kept = run_batch(L, d, "batch_routed", moments=moments, no_fallback=1)
                assert not kept["flags"].any()
                worst = max(worst, max(check_run(L, name, f"C=4 batch routed no_fallback{' moments' if moments else ''}", kept, ref, zero, models["entry no_fallback"]).values()))
    print(f"[sh cases] {L.kind} {name} C={C}: worst ratio {worst:.3f}")
    return worst
