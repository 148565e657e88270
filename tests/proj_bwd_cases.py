"""Cases, fp64 references and per-entry rounding bounds for the projection backward (gsgen_amd/csrc/geometry.hip): the four batched
entry points that share k_project_bwd_views -- plain, RGB + heads, SH moments, RGB + heads moments -- and the two single-view forms
k_project_bwd<false / true>.  Shared by tests/test_proj_bwd_host.py (the CPU emulator) and tests/test_gpu_proj_bwd.py (the device);
numpy, ctypes and torch-CPU fp64 only.  The backend is step_cases' (put / ptr / get / .lib / .stream).

The reference is independent of the kernel's hand-derived chain: torch autograd in fp64 over the forward as project_one states it,
one row per (view, Gaussian) or per (view, Gaussian, pixel), so that every row's own contribution c to (d mean, d qvec, d svec) is
known.  The moment forms are fed moments of a synthetic pixel list; their reference never expands a moment, it chains every pixel's
g w and 0.5 g w w^T with w = Sigma^-1 d.

Bounds, per entry, from the reference alone; EPS = 2^-24:
  plain, heads   EPS (B + 2) mag + 2^-40 F
  moment forms   EPS (B + K + 8 kappa) mag + 2^-40 F
  colour         EPS (B + 2) sum_v |g|
  d L / d mean2d left in place of a view's first moments   EPS (K + 8 kappa) sum_k |g_k w_k|
mag = sum of |c| over the unmasked rows of the entry, F = sum of |g_cov2d|_1 |A|_1^2 |s|^2 (induced 1-norms: the stricter reading)
over them, kappa = the largest condition number of the Gaussian's symmetrised cov2d over its unmasked views.  Every check returns
the worst fraction of its bound that it saw; the tests print it."""
import ctypes

import numpy as np
import torch

import scenes
from step_cases import bits, einval, rc  # noqa: F401  (einval / rc: re-exported for the tests)

EPS = 2.0 ** -24
FLOOR = 2.0 ** -40
K = 4                 # pixels of a (view, Gaussian)'s synthetic list
SENTINEL = 5.0        # the outputs hold this before a call
FLT_MAX = 3.402823466e+38
SC = 0.84932180028801904    # sqrt(0.5 log2 e), common.hpp:chol_prep
# (B, N): lane parity, one launch of 16 views, two, three; workgroups of 64 Gaussians.  B = 0 has a test of its own
SHAPES = [(1, 63), (2, 1), (3, 65), (16, 64), (17, 130), (33, 64)]
DEGENERATE = ("nan", "det", "negdiag", "inf")
# designed rows of a scene with N >= 63 (marked rows inside the random scene)
ROW = dict(unseen=0, only0=1, only15=2, only16=3, odd=4, iso=5, iso2=6, near_iso=7, q30=8, qsmall=9, nan=10, det=11, negdiag=12,
           inf=13)
DEG_VIEW = 0   # the view in which the four degenerate rows hold their degenerate covariance


def f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------
def scene_case(B, N, seed=0, iso_third=False):
    """scene, cameras and masks.  -> dict(mean, qvec, svec, c2w [B], mask [B] of uint8 [N], depth [B] (fp32, oracle.project),
    cov2d [B] (fp32 [N,4], oracle.project))"""
    from oracle import oracle as O
    sc = scenes.random_scene(N, seed=1000 * seed + 10 * N + B, svec=0.05, spread=0.5)
    rng = np.random.default_rng(77 + 1000 * seed + 10 * N + B)
    mean, qvec, svec = sc["mean"].copy(), sc["qvec"].copy(), sc["svec"].copy()
    designed = N >= 63
    if designed:
        mean[:14] *= 0.2                         # the designed rows sit near the centre: in front of every camera
        mean[ROW["unseen"]] = (0.0, 0.0, 50.0)   # ... but this one: outside every frustum (behind the orbit cameras, z = -8.6)
        svec[ROW["iso"]] = 0.05
        svec[ROW["iso2"]] = np.float32(0.03125)
        svec[ROW["near_iso"]] = np.float32(0.05) * (1.0 + np.array([0.0, 1e-6, -1e-6]))
        assert len(set(svec[ROW["near_iso"]].tolist())) == 3   # (fp32 does hold the three apart)
        qvec[ROW["q30"]] *= np.float32(30.0)
        qvec[ROW["qsmall"]] *= np.float32(1e-3)
    if iso_third:
        svec[::3] = svec[::3, :1]
    c2w = [np.ascontiguousarray(scenes.orbit(2.5, 10, 19.0 * v), np.float32) for v in range(B)]
    mask = [(rng.random(N) < 0.7).astype(np.uint8) for _ in range(B)]
    for v in range(B):
        if not designed:
            mask[0][0] = 1   # (N = 1: the Gaussian is seen at least once)
            break
        mask[v][ROW["unseen"]] = 0
        mask[v][ROW["only0"]] = v == 0
        mask[v][ROW["only15"]] = v == 15
        mask[v][ROW["only16"]] = v == 16
        mask[v][ROW["odd"]] = v % 2
        for k in DEGENERATE:
            mask[v][ROW[k]] = 1 if v in (DEG_VIEW, B - 1) else mask[v][ROW[k]]
        for k in ("iso", "near_iso", "q30", "qsmall"):
            mask[v][ROW[k]] = 1 if v == 0 else mask[v][ROW[k]]
    depth, cov2d = [], []
    for v in range(B):
        _, c, _, d = O.project(mean, qvec, svec, c2w[v])
        depth.append(np.ascontiguousarray(d.reshape(N)))
        cov2d.append(np.ascontiguousarray(c.reshape(N, 4)))
        seen = mask[v].astype(bool)
        assert (depth[v][seen] > 0.25).all()    # every unmasked Gaussian is well in front of its camera
    return dict(B=B, N=N, mean=mean, qvec=qvec, svec=svec, c2w=c2w, mask=mask, depth=depth, cov2d=cov2d, designed=designed)


def plain_inputs(case, seed=0):
    """g_mean2d [N,2], g_cov2d [N,4] (not symmetric: the kernel symmetrises), g_depth [N] per view"""
    rng = np.random.default_rng(5 + seed + 3 * case["N"] + case["B"])
    B, N = case["B"], case["N"]
    return dict(gm=[rng.normal(size=(N, 2)).astype(np.float32) for _ in range(B)],
                gc=[rng.normal(size=(N, 4)).astype(np.float32) for _ in range(B)],
                gd=[rng.normal(size=N).astype(np.float32) for _ in range(B)])


def chan6_inputs(case, seed=0):
    rng = np.random.default_rng(11 + seed + 3 * case["N"] + case["B"])
    return [rng.normal(size=(case["N"], 6)).astype(np.float32) for _ in range(case["B"])]


def chol_prep(cov):
    """common.hpp:chol_prep restated: fp64 from the fp32 cov2d [R,4], rounded to fp32 -> float32 [R,4] = (p0, p1, p2, ok)"""
    c = np.asarray(cov, np.float32).reshape(-1, 4)
    d0, d1, d2, d3 = (c[:, i].astype(np.float64) for i in range(4))
    with np.errstate(all="ignore"):
        det = d0 * d3 - d1 * d2
        ok = (np.abs(c) <= np.float32(FLT_MAX)).all(-1) & (det > 0.0) & (d3 > 0.0)
        sdet, s3 = np.where(ok, det, 1.0), np.where(ok, d3, 1.0)
        qa, qb, qc = s3 / sdet, -0.5 * (d1 + d2) / sdet, d0 / sdet
        l11 = np.sqrt(qa)
        l21 = qb / l11
        l22s = qc - l21 * l21
        ok = ok & (l22s > 0.0)
        l22 = np.sqrt(np.where(ok, l22s, 1.0))
        out = np.zeros((c.shape[0], 4), np.float32)
        for i, l in enumerate((l11, l21, l22)):
            out[:, i] = np.where(ok, l * SC, 0.0).astype(np.float32)
    out[:, 3] = ok
    return out


def det32(cov):
    """the contraction-free fp32 determinant moments_to_grads_sh defines as the semantics, and whether it counts"""
    c = np.asarray(cov, np.float32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        det = (c[:, 0] * c[:, 3]).astype(np.float32) - (c[:, 1] * c[:, 2]).astype(np.float32)
        ok = (det > 0) & (np.abs(det) <= np.float32(FLT_MAX))
    return det.astype(np.float32), ok


def degenerate_cov(kind):
    return {"nan": (np.nan,) * 4, "det": (1e-3, 2e-3, 2e-3, 1e-3), "negdiag": (-1e-3, 0.0, 0.0, -2e-3),
            "inf": (np.inf, 0.0, 0.0, 1e-3)}[kind]


def moment_inputs(case, form, seed=0):
    """The synthetic pixel lists and their moments.  form: "heads" (Cholesky records) or "sh" (fp32 determinant).
    -> dict(cov [B] fp32 [N,4] (the views' cov2d, with the degenerate rows planted), d [B,N,K,2], g [B,N,K], w [B,N,K,2] (the
    reference's Sigma^-1 d, zero where the view's record does not count), live [B,N] (record counts), kappa [B,N],
    mom2 [B] fp32 [N,2], mom4 [B] fp32 [N,4], chol [B] fp32 [N,4])"""
    B, N = case["B"], case["N"]
    rng = np.random.default_rng(23 + seed + 3 * N + B + (100 if form == "sh" else 0))
    cov = [c.copy() for c in case["cov2d"]]
    if case["designed"] and B > 0:
        for k in DEGENERATE:
            cov[DEG_VIEW][ROW[k]] = degenerate_cov(k)
    d, g = np.zeros((B, N, K, 2)), rng.normal(size=(B, N, K))
    w, live, kappa = np.zeros((B, N, K, 2)), np.zeros((B, N), bool), np.ones((B, N))
    mom2, mom4, chol = [], [], []
    for v in range(B):
        c = cov[v].astype(np.float64)
        rec = chol_prep(cov[v])
        dt, dt_ok = det32(cov[v])
        live[v] = rec[:, 3] != 0 if form == "heads" else dt_ok
        sym = np.stack([c[:, 0], 0.5 * (c[:, 1] + c[:, 2]), 0.5 * (c[:, 1] + c[:, 2]), c[:, 3]], -1).reshape(N, 2, 2)
        fin = np.isfinite(sym).all((1, 2))
        lam, vec = np.linalg.eigh(np.where(fin[:, None, None], sym, np.eye(2)))
        with np.errstate(all="ignore"):
            kappa[v] = np.where(live[v], np.abs(lam).max(-1) / np.abs(lam).min(-1), 1.0)
        z = rng.uniform(-1.06, 1.06, size=(N, K, 2))                  # within 1.5 sigma
        d[v] = np.einsum("nij,nkj->nki", vec, np.sqrt(np.abs(lam))[:, None, :] * z)
        x, y = d[v, :, :, 0], d[v, :, :, 1]
        gk = g[v]
        with np.errstate(all="ignore"):   # (the planted NaN / Inf rows: replaced below)
            if form == "heads":
                p0, p1, p2 = (rec[:, i].astype(np.float64)[:, None] for i in range(3))
                a, b = p0 * x + p1 * y, p2 * y
                inv = np.linalg.inv(np.where(live[v][:, None, None], sym, np.eye(2)))
                w[v] = np.einsum("nij,nkj->nki", inv, d[v])
            else:
                a, b = x * c[:, 3:4] - y * c[:, 2:3], y * c[:, 0:1] - x * c[:, 1:2]   # (tx, ty) of gauss_sh_pair
                w[v] = np.stack([a, b], -1) / dt.astype(np.float64)[:, None, None]
            w[v][~live[v]] = 0.0
            m2 = np.stack([(gk * a).sum(1), (gk * b).sum(1)], -1)
            m4 = np.stack([(gk * a * a).sum(1), (gk * a * b).sum(1), (gk * b * b).sum(1), np.full(N, 77.0)], -1)
        dead = ~live[v]   # no record, no whitened offsets: finite numbers the kernel must ignore
        m2[dead], m4[dead] = rng.normal(size=(int(dead.sum()), 2)), rng.normal(size=(int(dead.sum()), 4))
        mom2.append(m2.astype(np.float32))
        mom4.append(m4.astype(np.float32))
        chol.append(rec)
    return dict(form=form, cov=cov, d=d, g=g, w=w, live=live, kappa=kappa, mom2=mom2, mom4=mom4, chol=chol)


# ------------------------------------------------------------------------------------------------------------------------------
# the fp64 reference: autograd over project_one's forward, one row at a time
# ------------------------------------------------------------------------------------------------------------------------------
def chain(mean, qvec, svec, c2w, gm, gc, gd, detach_depth):
    """Rows r = 0 .. R-1, each its own Gaussian (mean [R,3], qvec [R,4], svec [R,3]: fp32 values), camera c2w [R,3,4] and upstream
    gradients gm [R,2], gc [R,4], gd [R] (fp64).  -> (c [R,10] = the row's contribution to d mean | d qvec | d svec, f [R] =
    |gc|_1 |A|_1^2 |s|^2: the size of the terms inside the chain)"""
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))  # noqa: E731
    p, q, s = (T(f64(a)).requires_grad_(True) for a in (mean, qvec, svec))
    cam = T(f64(c2w))
    Rc, t = cam[:, :, :3], cam[:, :, 3]
    u = torch.einsum("rji,rj->ri", Rc, p - t)                      # u = Rc^T (p - t)
    qh = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)
    w, x, y, z = qh.unbind(1)
    Rq = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                      2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                      2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = Rq * s[:, None, :]
    S = M @ M.transpose(1, 2)
    ud = u.detach()
    ux, uy, uz = ud.unbind(1)
    zero = torch.zeros_like(ux)
    J = torch.stack([1 / uz, zero, -ux / uz / uz, zero, 1 / uz, -uy / uz / uz], 1).reshape(-1, 2, 3)   # (J is a constant)
    A = J @ Rc.transpose(1, 2)
    cov = A @ S @ A.transpose(1, 2)
    zz = ud[:, 2] if detach_depth else u[:, 2]
    m2 = u[:, :2] / zz[:, None]
    loss = (T(gm) * m2).sum() + (T(gc).reshape(-1, 2, 2) * cov).sum() + (T(gd) * u[:, 2]).sum()
    gp, gq, gs = torch.autograd.grad(loss, (p, q, s))
    gcn = np.abs(np.asarray(gc, np.float64)).reshape(-1, 2, 2).sum(1).max(-1)
    an = A.detach().abs().sum(1).max(-1).values.numpy()
    f = gcn * an * an * (f64(svec) ** 2).sum(-1)
    return np.concatenate([gp.numpy(), gq.numpy(), gs.numpy()], 1), f


def _rows(case, per=1):
    """the (view, Gaussian[, pixel]) rows of a case, view-major -> (mean, qvec, svec, c2w) repeated"""
    B, N = case["B"], case["N"]
    rep = lambda a: np.repeat(np.tile(a, (B,) + (1,) * (a.ndim - 1)), per, axis=0)  # noqa: E731
    cam = np.repeat(np.repeat(np.stack(case["c2w"]), N, axis=0), per, axis=0)
    return rep(case["mean"]), rep(case["qvec"]), rep(case["svec"]), cam


def heads_gdepth(case, chan6):
    """d L / d depth = g3 + 2 depth g5 of every view, fp64 from the fp32 values -> [B,N]"""
    return np.stack([f64(c[:, 3]) + 2.0 * f64(d) * f64(c[:, 5]) for c, d in zip(chan6, case["depth"])])


def reference_plain(case, inp, gdepth, detach_depth):
    """-> c [B,N,10], f [B,N]; gdepth [B,N] fp64"""
    B, N = case["B"], case["N"]
    if B == 0:
        return np.zeros((0, N, 10)), np.zeros((0, N))
    c, f = chain(*_rows(case), np.concatenate([f64(a) for a in inp["gm"]]), np.concatenate([f64(a) for a in inp["gc"]]),
                 gdepth.reshape(-1), detach_depth)
    return c.reshape(B, N, 10), f.reshape(B, N)


def reference_moments(case, mo, gdepth, detach_depth):
    """-> c [B,N,K+1,10] (the K pixels, then the depth gradient's own row), f [B,N], gm2d [B,N,2] = sum_k g_k w_k,
    gm2d_abs [B,N,2] = sum_k |g_k w_k|"""
    B, N = case["B"], case["N"]
    if B == 0:
        return np.zeros((0, N, K + 1, 10)), np.zeros((0, N)), np.zeros((0, N, 2)), np.zeros((0, N, 2))
    gw = mo["g"][..., None] * mo["w"]                                            # [B,N,K,2]
    gc = 0.5 * mo["g"][..., None, None] * mo["w"][..., :, None] * mo["w"][..., None, :]
    cp, f = chain(*_rows(case, K), gw.reshape(-1, 2), gc.reshape(-1, 4), np.zeros(B * N * K), detach_depth)
    cd, _ = chain(*_rows(case), np.zeros((B * N, 2)), np.zeros((B * N, 4)), gdepth.reshape(-1), detach_depth)
    c = np.concatenate([cp.reshape(B, N, K, 10), cd.reshape(B, N, 1, 10)], 2)
    return c, f.reshape(B, N, K).sum(-1), gw.sum(2), np.abs(gw).sum(2)


def fold(c, f, masks, factor):
    """want = sum of the unmasked rows' c, tol = EPS factor mag + 2^-40 F.  c [B,N,(P,)10], f [B,N], masks [B,N] bool,
    factor scalar or [N] -> (want [N,10], tol [N,10])"""
    m = masks.astype(np.float64)
    if c.ndim == 4:
        want, mag = (c * m[:, :, None, None]).sum((0, 2)), (np.abs(c) * m[:, :, None, None]).sum((0, 2))
    else:
        want, mag = (c * m[:, :, None]).sum(0), (np.abs(c) * m[:, :, None]).sum(0)
    F = (f * m).sum(0)
    return want, EPS * np.reshape(factor, (-1, 1)) * mag + FLOOR * F[:, None]


def fraction(got, want, tol, what):
    """worst |got - want| / tol; asserts every entry finite and within its bound (tol = 0: equal)"""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), what
    err = np.abs(got - want)
    bad = err > tol
    assert not bad.any(), (what, np.argwhere(bad)[:6].tolist(), float((err[bad] / np.maximum(tol[bad], 1e-300)).max()))
    return float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# running an entry point on a backend
# ------------------------------------------------------------------------------------------------------------------------------
def table(Bk, handles, n=None):
    """a host array of device pointers (never of length 0: the entry points test the table itself against NULL)"""
    vals = [Bk.ptr(h) for h in handles]
    return (ctypes.c_void_p * max(len(vals), 1 if n is None else n))(*vals)


class Scene:
    """a case's parameters and cameras on a backend (read only: shared by the runs of a test)"""

    def __init__(self, Bk, case):
        self.Bk, self.case = Bk, case
        self.mean, self.qvec, self.svec = (Bk.put(case[k]) for k in ("mean", "qvec", "svec"))
        self.cams = [Bk.put(c) for c in case["c2w"]]
        self.masks = [Bk.put(m) for m in case["mask"]]

    def head(self):
        Bk, c = self.Bk, self.case
        return (c["B"], c["N"], Bk.ptr(self.mean), Bk.ptr(self.qvec), Bk.ptr(self.svec))

    def outputs(self, colour=False):
        N = self.case["N"]
        return [self.Bk.put(np.full((N, k), SENTINEL, np.float32)) for k in ((3, 4, 3, 3) if colour else (3, 4, 3))]

    def read(self, outs):
        got = [self.Bk.get(h) for h in outs]
        return np.concatenate(got[:3], 1), (got[3] if len(got) > 3 else None)


def run_plain(S, inp, detach_depth, masks="table", gdepth="table"):
    """masks: "table", None (no table) or a list of handles / None per view; gdepth likewise -> [N,10]"""
    Bk = S.Bk
    hm = S.masks if masks == "table" else masks
    gdl = [Bk.put(a) for a in inp["gd"]] if gdepth == "table" else gdepth
    gm, gc = [Bk.put(a) for a in inp["gm"]], [Bk.put(a) for a in inp["gc"]]
    outs = S.outputs()
    Bk.lib.project_gaussians_backward_batch(*S.head(), table(Bk, S.cams), int(detach_depth), None if hm is None else table(Bk, hm),
                                            table(Bk, gm), table(Bk, gc), None if gdl is None else table(Bk, gdl),
                                            *[Bk.ptr(h) for h in outs], Bk.stream)
    for h, a in zip(gm + gc, inp["gm"] + inp["gc"]):   # read only
        assert np.array_equal(bits(Bk.get(h)), bits(a))
    return S.read(outs)[0]


def run_heads(S, inp, chan6, detach_depth, masks="table"):
    """-> ([N,10], colour [N,3])"""
    Bk = S.Bk
    hm = S.masks if masks == "table" else masks
    gm, gc = [Bk.put(a) for a in inp["gm"]], [Bk.put(a) for a in inp["gc"]]
    ch, dp = [Bk.put(a) for a in chan6], [Bk.put(a) for a in S.case["depth"]]
    outs = S.outputs(colour=True)
    Bk.lib.project_gaussians_backward_batch_heads(*S.head(), table(Bk, S.cams), int(detach_depth),
                                                  None if hm is None else table(Bk, hm), table(Bk, gm), table(Bk, gc),
                                                  table(Bk, ch), table(Bk, dp), *[Bk.ptr(h) for h in outs], Bk.stream)
    return S.read(outs)


def run_moments(S, mo, chan6, detach_depth, masks="table", chol=None, stats=(None, None)):
    """chol: None or a list of handles (heads form); stats: the (grad_accum, cnt) priors or None each
    -> dict(g [N,10], colour, m2 [B] (the first-moment arrays afterwards), stats (accum, cnt))"""
    Bk, form = S.Bk, mo["form"]
    hm = S.masks if masks == "table" else masks
    m2, m4 = [Bk.put(a) for a in mo["mom2"]], [Bk.put(a) for a in mo["mom4"]]
    cv = [Bk.put(a) for a in mo["cov"]]
    st = [None if a is None else Bk.put(a) for a in stats]
    mt = None if hm is None else table(Bk, hm)
    outs = S.outputs(colour=form == "heads")
    if form == "heads":
        ch, dp = [Bk.put(a) for a in chan6], [Bk.put(a) for a in S.case["depth"]]
        Bk.lib.project_gaussians_backward_batch_heads_moments(
            *S.head(), table(Bk, S.cams), int(detach_depth), mt, table(Bk, m2), table(Bk, m4), table(Bk, ch), table(Bk, dp),
            table(Bk, cv), None if chol is None else table(Bk, chol), *[Bk.ptr(h) for h in outs], Bk.ptr(st[0]), Bk.ptr(st[1]),
            Bk.stream)
    else:
        Bk.lib.project_gaussians_backward_batch_moments_sh(
            *S.head(), table(Bk, S.cams), int(detach_depth), mt, table(Bk, m2), table(Bk, m4), table(Bk, cv),
            *[Bk.ptr(h) for h in outs], Bk.ptr(st[0]), Bk.ptr(st[1]), Bk.stream)
    for h, a in zip(m4 + cv, mo["mom4"] + mo["cov"]):   # read only
        assert np.array_equal(bits(Bk.get(h)), bits(a))
    g, colour = S.read(outs)
    return dict(g=g, colour=colour, m2=[Bk.get(h) for h in m2], stats=[None if h is None else Bk.get(h) for h in st])


# ------------------------------------------------------------------------------------------------------------------------------
# checks
# ------------------------------------------------------------------------------------------------------------------------------
def mask_array(case, masks=None):
    B, N = case["B"], case["N"]
    masks = case["mask"] if masks is None else masks
    return np.stack([np.ones(N, bool) if m is None else m.astype(bool) for m in masks]) if B else np.zeros((0, N), bool)


def designed_rows_seen_as_designed(case):
    """the marked rows do what their names say in this case (so that the case cannot silently lose them)"""
    if not case["designed"]:
        return
    m, B = mask_array(case), case["B"]
    assert not m[:, ROW["unseen"]].any()
    assert m[:, ROW["only0"]].sum() == 1 and m[0, ROW["only0"]]
    assert m[:, ROW["only15"]].sum() == (B > 15) and m[:, ROW["only16"]].sum() == (B > 16)
    assert m[:, ROW["odd"]].sum() == B // 2
    s = case["svec"]
    assert s[ROW["iso"], 0] == s[ROW["iso"], 1] == s[ROW["iso"], 2]
    n30, nsm = (np.linalg.norm(case["qvec"][ROW[k]].astype(np.float64)) for k in ("q30", "qsmall"))
    assert abs(n30 - 30) < 1e-3 and abs(nsm - 1e-3) < 1e-7


def plain_check(Bk, B, N, detach_depth, iso_third=False):
    """gsgen_project_gaussians_backward_batch: the bound, two runs bit-identical, and the table shapes (no mask table, one view's
    mask NULL, no g_depth table, g_depth NULL for some views) -> worst fraction of the bound"""
    case = scene_case(B, N, iso_third=iso_third)
    designed_rows_seen_as_designed(case)
    inp, S = plain_inputs(case), Scene(Bk, case)
    gd = np.stack([f64(a) for a in inp["gd"]])
    c, f = reference_plain(case, inp, gd, detach_depth)
    c0, _ = reference_plain(case, inp, np.zeros_like(gd), detach_depth)    # without any depth gradient
    want, tol = fold(c, f, mask_array(case), B + 2)
    got = run_plain(S, inp, detach_depth)
    frac = fraction(got, want, tol, ("plain", B, N))
    assert np.array_equal(bits(run_plain(S, inp, detach_depth)), bits(got))   # no atomics: deterministic
    if case["designed"]:   # never visible: exact zeros over the sentinel
        assert not got[ROW["unseen"]].any()
    # no mask table: every view sees every Gaussian
    want, tol = fold(c, f, np.ones((B, N), bool), B + 2)
    frac = max(frac, fraction(run_plain(S, inp, detach_depth, masks=None), want, tol, ("plain, no mask table", B, N)))
    # one view's mask NULL
    v0 = min(1, B - 1)
    hm = [None if v == v0 else h for v, h in enumerate(S.masks)]
    ma = mask_array(case, [None if v == v0 else m for v, m in enumerate(case["mask"])])
    want, tol = fold(c, f, ma, B + 2)
    frac = max(frac, fraction(run_plain(S, inp, detach_depth, masks=hm), want, tol, ("plain, one mask NULL", B, N)))
    # no g_depth table; g_depth NULL in the odd views
    want, tol = fold(c0, f, mask_array(case), B + 2)
    frac = max(frac, fraction(run_plain(S, inp, detach_depth, gdepth=None), want, tol, ("plain, no g_depth", B, N)))
    odd = (np.arange(B) % 2 == 1)[:, None, None]
    want, tol = fold(np.where(odd, c0, c), f, mask_array(case), B + 2)
    gdl = [None if v % 2 else Bk.put(a) for v, a in enumerate(inp["gd"])]
    frac = max(frac, fraction(run_plain(S, inp, detach_depth, gdepth=gdl), want, tol, ("plain, some g_depth NULL", B, N)))
    return frac


def colour_reference(case, chan6):
    m = mask_array(case)[:, :, None]
    g = np.stack([f64(a[:, :3]) for a in chan6]) if case["B"] else np.zeros((0, case["N"], 3))
    return (g * m).sum(0), EPS * (case["B"] + 2) * (np.abs(g) * m).sum(0)


def heads_check(Bk, B, N, detach_depth):
    """gsgen_project_gaussians_backward_batch_heads -> worst fractions (gradients, colour)"""
    case = scene_case(B, N, seed=1)
    designed_rows_seen_as_designed(case)
    inp, chan6, S = plain_inputs(case, 1), chan6_inputs(case), Scene(Bk, case)
    c, f = reference_plain(case, inp, heads_gdepth(case, chan6), detach_depth)
    want, tol = fold(c, f, mask_array(case), B + 2)
    got, colour = run_heads(S, inp, chan6, detach_depth)
    frac = fraction(got, want, tol, ("heads", B, N))
    fc = fraction(colour, *colour_reference(case, chan6), ("heads colour", B, N))
    again, colour2 = run_heads(S, inp, chan6, detach_depth)
    assert np.array_equal(bits(again), bits(got)) and np.array_equal(bits(colour2), bits(colour))
    # the depth^2 head alone moves d mean: the reference without it differs by more than the bound somewhere
    no5 = [a.copy() for a in chan6]
    for a in no5:
        a[:, 5] = 0.0
    c5, _ = reference_plain(case, inp, heads_gdepth(case, no5), detach_depth)
    assert (np.abs(fold(c5, f, mask_array(case), B + 2)[0] - want) > tol).any()
    # no mask table
    want, tol = fold(c, f, np.ones((B, N), bool), B + 2)
    got, colour = run_heads(S, inp, chan6, detach_depth, masks=None)
    frac = max(frac, fraction(got, want, tol, ("heads, no mask table", B, N)))
    g = np.stack([f64(a[:, :3]) for a in chan6])
    fc = max(fc, fraction(colour, g.sum(0), EPS * (B + 2) * np.abs(g).sum(0), ("heads colour, no mask table", B, N)))
    return frac, fc


def moments_check(Bk, B, N, form, detach_depth, device_chol=None):
    """One moment form on one shape.  device_chol (heads): callable(case) -> (handles of the records the projection launch left,
    their frustum masks [B] uint8) on this backend; None: the restated records.
    -> dict of worst fractions: g, m2d (the view's d L / d mean2d left in place), stat, colour; and median of EPS (B + K + 8 kappa)"""
    case = scene_case(B, N, seed=2 if form == "heads" else 3)
    designed_rows_seen_as_designed(case)
    mo, S = moment_inputs(case, form), Scene(Bk, case)
    chan6 = chan6_inputs(case, 2) if form == "heads" else None
    ma = mask_array(case)
    gd = heads_gdepth(case, chan6) if form == "heads" else np.zeros((B, N))
    c, f, gm2d, gm2d_abs = reference_moments(case, mo, gd, detach_depth)
    kap = np.where(ma & mo["live"], mo["kappa"], 1.0).max(0)
    assert (kap <= 100).sum() * 2 >= N, "the kappa term would make the bound vacuous on most of this case"
    factor = B + K + 8 * kap
    want, tol = fold(c, f, ma, factor)
    rng = np.random.default_rng(B + N)
    prior = ((rng.random(N) * 1e-2 + 1e-3).astype(np.float32), rng.integers(1, 6, N).astype(np.float32))
    out = run_moments(S, mo, chan6, detach_depth, stats=prior)
    fr = dict(g=fraction(out["g"], want, tol, (form, B, N)), median_factor=float(np.median(EPS * factor)))
    if form == "heads":
        fr["colour"] = fraction(out["colour"], *colour_reference(case, chan6), (form, "colour", B, N))
    # the views' first-moment arrays afterwards: d L / d mean2d on the unmasked rows, the moments' own bits on the masked ones
    fr["m2d"], norms = 0.0, np.zeros((B, N))
    for v in range(B):
        seen = ma[v]
        assert np.array_equal(bits(out["m2"][v][~seen]), bits(mo["mom2"][v][~seen])), (form, "masked rows touched", v)
        t2 = EPS * (K + 8 * np.where(mo["live"][v], mo["kappa"][v], 1.0))[:, None] * gm2d_abs[v]
        fr["m2d"] = max(fr["m2d"], fraction(out["m2"][v][seen], gm2d[v][seen], t2[seen], (form, "mean2d in place", v)))
        dead = seen & ~mo["live"][v]
        assert not out["m2"][v][dead].any(), (form, "a degenerate record left a gradient", v)
        norms[v] = np.where(seen, np.sqrt((out["m2"][v].astype(np.float64) ** 2).sum(-1)), 0.0)
    # statistics: prior + sum of the norms of what was left in place (those values are bounded above), prior + visits
    visits = ma.sum(0)
    acc, cnt = out["stats"]
    want_acc = prior[0].astype(np.float64) + norms.sum(0)
    fr["stat"] = fraction(acc[visits > 0], want_acc[visits > 0], (EPS * (B + 2) * want_acc)[visits > 0], (form, "stat_grad_accum"))
    assert np.array_equal(cnt, prior[1] + visits.astype(np.float32)), (form, "stat_cnt")
    for got_, pr in zip((acc, cnt), prior):
        assert np.array_equal(bits(got_[visits == 0]), bits(pr[visits == 0])), (form, "statistics touched without a visit")
    # either statistics pointer NULL: the gradients keep their bits, the other half is as before (or untouched)
    o2 = run_moments(S, mo, chan6, detach_depth, stats=(prior[0], None))
    assert np.array_equal(bits(o2["g"]), bits(out["g"])) and np.array_equal(bits(o2["stats"][0]), bits(acc))
    o3 = run_moments(S, mo, chan6, detach_depth, stats=(None, prior[1]))
    assert np.array_equal(bits(o3["g"]), bits(out["g"])) and np.array_equal(bits(o3["stats"][1]), bits(prior[1]))
    for v in range(B):
        assert np.array_equal(bits(o3["m2"][v]), bits(out["m2"][v]))
    # the degenerate rows: nothing through mean2d / cov2d from that view, depth and colour still, a visit, finite
    if case["designed"] and B > 0:
        for k in DEGENERATE:
            r = ROW[k]
            assert ma[DEG_VIEW, r] and np.isfinite(out["g"][r]).all()
            # (a negative definite covariance has a positive determinant: the SH form's semantics evaluate it)
            assert mo["live"][DEG_VIEW, r] == (form == "sh" and k == "negdiag"), (form, k)
            if not mo["live"][DEG_VIEW, r]:
                assert not np.abs(c[DEG_VIEW, r, :K]).any() and not out["m2"][DEG_VIEW][r].any()
            assert cnt[r] == prior[1][r] + visits[r]
        if form == "heads":
            assert np.abs(c[DEG_VIEW, ROW["nan"], K]).max() > 0   # its depth gradient does arrive
    # the records as a table (heads): bit-equal gradients
    if form == "heads" and B > 0:
        # a row whose ok word is 0 may hold any factor (a culled row of the projection launch holds the unit covariance's): the
        # degenerate rows of the table carry that, so that only the ok word keeps them out
        unit = chol_prep(np.array([[1.0, 0.0, 0.0, 1.0]], np.float32))[0]
        unit[3] = 0.0
        if device_chol is None:
            recs = [a.copy() for a in mo["chol"]]
            recs[DEG_VIEW][~mo["live"][DEG_VIEW]] = unit
            hch, hmasks = [Bk.put(a) for a in recs], "table"
        else:
            hch, fmask = device_chol(case)
            for v in range(B):
                rec, fm = Bk.get(hch[v]), fmask[v].astype(bool)
                assert fm.sum() * 2 > N and (not case["designed"] or not fm[ROW["unseen"]])
                clean = chol_prep(case["cov2d"][v])
                assert np.array_equal(bits(rec[fm]), bits(clean[fm])), ("device records differ from chol_prep restated", v)
                assert not rec[~fm, 3].any(), ("ok word set on a culled row", v)
            # (the planted degenerate covariances are not the projection launch's)
            rec = Bk.get(hch[DEG_VIEW])
            rec[~mo["live"][DEG_VIEW]] = unit
            hch = list(hch)
            hch[DEG_VIEW] = Bk.put(rec)
            hmasks = [Bk.put(m & f_) for m, f_ in zip(case["mask"], fmask)]
        a = run_moments(S, mo, chan6, detach_depth, masks=hmasks, chol=hch, stats=prior)
        b = run_moments(S, mo, chan6, detach_depth, masks=hmasks, stats=prior)
        for x, y in [(a["g"], b["g"]), (a["colour"], b["colour"])] + list(zip(a["stats"], b["stats"])):
            assert np.array_equal(bits(x), bits(y)), "records from the table and records formed in the kernel disagree"
        for x, y in zip(a["m2"], b["m2"]):   # (equal values: the zeros a record without its ok word leaves take the sign of its factor)
            assert np.array_equal(x, y), "d L / d mean2d from the table's records and from the kernel's disagree"
        if device_chol is None:
            assert np.array_equal(bits(a["g"]), bits(out["g"]))
    else:   # determinism of the SH form
        b = run_moments(S, mo, chan6, detach_depth, stats=prior)
        assert np.array_equal(bits(b["g"]), bits(out["g"]))
    return fr


def empty_batch_check(Bk, N=65):
    """n_views = 0 zero-fills the sentinel-filled outputs, in every form"""
    case = scene_case(0, N)
    S = Scene(Bk, case)
    inp = plain_inputs(case)
    assert not run_plain(S, inp, 1).any() and not run_plain(S, inp, 0, masks=None, gdepth=None).any()
    g, col = run_heads(S, inp, [], 1)
    assert not g.any() and not col.any()
    for form in ("heads", "sh"):
        prior = (np.full(N, 0.5, np.float32), np.full(N, 2.0, np.float32))
        out = run_moments(S, moment_inputs(case, form), [], 1, stats=prior)
        assert not out["g"].any() and (out["colour"] is None or not out["colour"].any())
        assert np.array_equal(out["stats"][0], prior[0]) and np.array_equal(out["stats"][1], prior[1])


def single_view_check(Bk, N, detach_depth):
    """k_project_bwd<false> (overwrite: zeros on masked rows) and <true> (accumulate: masked rows untouched, two cameras into shared
    arrays), same reference, the plain bound with B = 1 per launch -> worst fraction"""
    case = scene_case(2, N, seed=4)
    inp, S = plain_inputs(case, 4), Scene(Bk, case)
    gd = np.stack([f64(a) for a in inp["gd"]])
    c, f = reference_plain(case, inp, gd, detach_depth)
    ma = mask_array(case)
    lib, p = Bk.lib, Bk.ptr
    hg = [[Bk.put(inp[k][v]) for k in ("gm", "gc", "gd")] for v in range(2)]
    frac = 0.0
    for v in range(2):
        outs = S.outputs()
        lib.project_gaussians_backward_masked(N, p(S.mean), p(S.qvec), p(S.svec), p(S.cams[v]), int(detach_depth), p(S.masks[v]),
                                              p(hg[v][0]), p(hg[v][1]), p(hg[v][2]), *[p(h) for h in outs], Bk.stream)
        got = S.read(outs)[0]
        want, tol = fold(c[v:v + 1], f[v:v + 1], ma[v:v + 1], 3)
        frac = max(frac, fraction(got, want, tol, ("masked", v, N)))
        assert not got[~ma[v]].any()
    # the unmasked entry point, no g_depth
    c0, _ = reference_plain(case, inp, np.zeros_like(gd), detach_depth)
    outs = S.outputs()
    lib.project_gaussians_backward(N, p(S.mean), p(S.qvec), p(S.svec), p(S.cams[0]), int(detach_depth), p(hg[0][0]), p(hg[0][1]), None,
                                   *[p(h) for h in outs], Bk.stream)
    want, tol = fold(c0[:1], f[:1], np.ones((1, N), bool), 3)
    frac = max(frac, fraction(S.read(outs)[0], want, tol, ("unmasked", N)))
    # accumulate: two cameras into shared arrays that hold a prior (one more rounding per camera: the additions)
    prior = np.random.default_rng(N).normal(size=(N, 10)).astype(np.float32)
    outs = [Bk.put(np.ascontiguousarray(prior[:, a:b])) for a, b in ((0, 3), (3, 7), (7, 10))]
    for v in range(2):
        lib.project_gaussians_backward_accum(N, p(S.mean), p(S.qvec), p(S.svec), p(S.cams[v]), int(detach_depth), p(S.masks[v]),
                                             p(hg[v][0]), p(hg[v][1]), p(hg[v][2]), *[p(h) for h in outs], Bk.stream)
    got = S.read(outs)[0]
    want, tol = fold(c, f, ma, 3)
    pr = prior.astype(np.float64)
    frac = max(frac, fraction(got, want + pr, tol + EPS * 2 * (np.abs(pr) + np.abs(c * ma[:, :, None]).sum(0)), ("accum", N)))
    none = ~ma.any(0)
    assert np.array_equal(bits(got[none]), bits(prior[none]))
    return frac


def bad_arguments_check(Bk, N=65, B=3):
    """GSGEN_EINVAL before any launch: the outputs keep the sentinel.  Every pointer handed over is valid and large enough."""
    case = scene_case(B, N, seed=5)
    S, inp, chan6 = Scene(Bk, case), plain_inputs(case, 5), chan6_inputs(case, 5)
    mo = moment_inputs(case, "heads")
    lib, p, EI = Bk.lib, Bk.ptr, einval()
    T = lambda hs: table(Bk, hs)  # noqa: E731
    gm, gc = [Bk.put(a) for a in inp["gm"]], [Bk.put(a) for a in inp["gc"]]
    ch, dp = [Bk.put(a) for a in chan6], [Bk.put(a) for a in case["depth"]]
    m2, m4, cv = ([Bk.put(a) for a in mo[k]] for k in ("mom2", "mom4", "cov"))
    outs = S.outputs(colour=True)
    o = [p(h) for h in outs]
    hole = lambda hs: T([None if v == 1 else h for v, h in enumerate(hs)])  # noqa: E731
    head, cams, masks, s = S.head(), T(S.cams), T(S.masks), Bk.stream
    calls = [
        # heads without g_color / depth / g_chan6
        (lib.project_gaussians_backward_batch_heads, (*head, cams, 1, masks, T(gm), T(gc), T(ch), T(dp), *o[:3], None, s)),
        (lib.project_gaussians_backward_batch_heads, (*head, cams, 1, masks, T(gm), T(gc), T(ch), None, *o, s)),
        (lib.project_gaussians_backward_batch_heads, (*head, cams, 1, masks, T(gm), T(gc), None, T(dp), *o, s)),
        # moment forms without cov2d
        (lib.project_gaussians_backward_batch_moments_sh, (*head, cams, 1, masks, T(m2), T(m4), None, *o[:3], None, None, s)),
        (lib.project_gaussians_backward_batch_heads_moments,
         (*head, cams, 1, masks, T(m2), T(m4), T(ch), T(dp), None, None, *o, None, None, s)),
        # a NULL entry inside a required table
        (lib.project_gaussians_backward_batch, (*head, hole(S.cams), 1, masks, T(gm), T(gc), None, *o[:3], s)),
        (lib.project_gaussians_backward_batch, (*head, cams, 1, masks, hole(gm), T(gc), None, *o[:3], s)),
        (lib.project_gaussians_backward_batch, (*head, cams, 1, masks, T(gm), hole(gc), None, *o[:3], s)),
        (lib.project_gaussians_backward_batch_heads, (*head, cams, 1, masks, T(gm), T(gc), hole(ch), T(dp), *o, s)),
        (lib.project_gaussians_backward_batch_heads, (*head, cams, 1, masks, T(gm), T(gc), T(ch), hole(dp), *o, s)),
        (lib.project_gaussians_backward_batch_moments_sh, (*head, cams, 1, masks, T(m2), T(m4), hole(cv), *o[:3], None, None, s)),
        (lib.project_gaussians_backward_batch_heads_moments,
         (*head, cams, 1, masks, T(m2), T(m4), T(ch), T(dp), hole(cv), None, *o, None, None, s)),
        # n_views > 0 with no camera table; no output array
        (lib.project_gaussians_backward_batch, (*head, None, 1, masks, T(gm), T(gc), None, *o[:3], s)),
        (lib.project_gaussians_backward_batch, (*head, cams, 1, masks, T(gm), T(gc), None, o[0], None, o[2], s)),
    ]
    for i, (fn, args) in enumerate(calls):
        assert rc(fn, *args) == EI, (i, fn.__name__)
    for h in outs:
        assert (Bk.get(h) == np.float32(SENTINEL)).all()
    for h, a in zip(m2, mo["mom2"]):
        assert np.array_equal(bits(Bk.get(h)), bits(a))
    return len(calls)
