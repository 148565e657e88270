"""Cases, fp64 references and rounding bounds for the kernels of a training step that are not the render: the fused Adam step, the SH
coefficient bounds that decide the polynomial routing, and the densify / prune statistics.  Shared by tests/test_step_kernels_host.py
(the CPU emulator) and tests/test_gpu_step_kernels.py (the device); numpy and ctypes only.

A backend hides where the arrays live:  put(array, skew=0) -> handle whose address is 16-byte aligned plus 4 * skew bytes,
ptr(handle) -> address (None for None), get(handle) -> numpy copy, .lib -> gsgen_amd._capi.Lib, .stream.

The bounds are derived from the roundings of the kernels' expressions (DESIGN.md "The step's small kernels at their edges"), never
from what a kernel returned; every check returns the worst fraction of its bound that it saw, and the tests print it."""
import ctypes
import re
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = 2.0 ** -23       # one fp32 ulp of 1
TINY = 2.0 ** -149   # the smallest fp32 sub-normal


class HostBackend:
    """arrays in host memory, for the emulator build of the library"""
    stream = None

    def __init__(self, lib):
        self.lib = lib

    def put(self, a, skew=0):
        a = np.ascontiguousarray(a)
        raw = np.empty(a.nbytes + 32, np.uint8)
        off = (-raw.ctypes.data) % 16 + 4 * skew
        h = raw[off:off + a.nbytes].view(a.dtype).reshape(a.shape)
        h[...] = a
        return h

    def ptr(self, h):
        return None if h is None else h.ctypes.data

    def get(self, h):
        return h.copy()


def einval():
    """the value of GSGEN_EINVAL as the header states it"""
    txt = open(os.path.join(ROOT, "include", "gsgen_hip.h")).read()
    return int(re.search(r"#define\s+GSGEN_EINVAL\s+\(?(-?\d+)\)?", txt).group(1))


def rc(fn, *args):
    """the C function's return code (the ctypes wrappers raise on a non-zero one and name it)"""
    from gsgen_amd._capi import GsgenError
    try:
        fn(*args)
    except GsgenError as e:
        return int(re.search(r"\(code (-?\d+)\)", str(e)).group(1))
    return 0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. Adam
# ------------------------------------------------------------------------------------------------------------------------------
ADAM_CASES = [(1, [1]), (2, [1, 2]), (3, [3]), (5, [1, 2, 3, 5, 5]), (1021, [1, 2, 3, 5, 5, 9, 1020, 1021]), (1024, [1024]),
              (1025, [511, 1025]), (3074, [7, 7, 7, 1030, 3073, 3074])]
ADAM_STEPS = (1, 2, 1000, 100000)
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-15


def _wide(rng, n, lo=-24, hi=2):
    """normal x 10^U{lo..hi}: from gradients whose square vanishes in fp32, through squares that are sub-normal, to large ones"""
    return (rng.normal(size=n) * 10.0 ** rng.integers(lo, hi + 1, n)).astype(np.float32)


def group_of(n, ends):
    """element -> group, by the kernel's rule: the last group k with i >= ends[k - 1]"""
    return np.minimum(np.searchsorted(np.asarray(ends, np.int64), np.arange(n), side="right"), len(ends) - 1)


def adam_inputs(n, ends, step, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * n + step % 97)
    g = _wide(rng, n)
    g[rng.random(n) < 0.1] = 0.0
    edge = sorted({i for e in ends for i in (e - 1, e) if 0 <= i < n})   # both sides of every group boundary
    for i in edge:   # ... non-zero, and with a square that fp32 holds to a few digits at least: the self-check's factor stays large
        while abs(g[i]) < 1e-19:
            g[i] = _wide(rng, 1, lo=-17)[0]
    p = (rng.normal(size=n) * 10.0 ** rng.integers(-12, 1, n)).astype(np.float32)
    p[edge] = 0.0   # (there an element given its neighbour's learning rate is visible however small that rate is: see adam_moved_boundaries)
    if step == 1:
        m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    else:
        m = _wide(rng, n)
        v = (_wide(rng, n).astype(np.float64) ** 2).astype(np.float32)
        m[rng.random(n) < 1 / 3] = 0.0
        v[rng.random(n) < 1 / 3] = 0.0
    lrs = np.array([10.0 ** -(k + 1) for k in range(len(ends))], np.float32)
    return dict(n=n, ends=np.array(ends, np.uint64), step=step, p=p, g=g, m=m, v=v, lrs=lrs)


def adam_scalars(lib, case):
    """the nine fp32 scalars of the step, from gsgen_adam_step_scalars -- asserted to be the documented double-precision expressions"""
    ng = len(case["ends"])
    s9 = np.full(9, 7.0, np.float32)
    lib.adam_step_scalars(ng, case["lrs"].ctypes.data, BETA1, BETA2, case["step"], s9.ctypes.data)
    b1, b2, t = np.float64(np.float32(BETA1)), np.float64(np.float32(BETA2)), case["step"]
    for k in range(8):
        want = np.float32(np.float64(case["lrs"][k]) / (1.0 - b1 ** t)) if k < ng else np.float32(0)
        assert s9[k] == want, (k, s9[k], want)
    assert s9[8] == np.float32(np.sqrt(1.0 - b2 ** t)), s9[8]
    return s9


def adam_reference(case, s9, ends=None):
    """fp64 from the fp32 inputs -> dict of p, m, v and the per-entry bounds tol_p, tol_m, tol_v"""
    n = case["n"]
    ends = case["ends"] if ends is None else ends
    p, g, m, v = (case[k].astype(np.float64) for k in "pgmv")
    w1 = np.float64(np.float32(1.0) - np.float32(BETA1))
    w2 = np.float64(np.float32(1.0) - np.float32(BETA2))
    b2, eps = np.float64(np.float32(BETA2)), np.float64(np.float32(ADAM_EPS))
    ss = s9[:8].astype(np.float64)[group_of(n, ends)]
    bc2 = np.float64(s9[8])
    m1 = m + (g - m) * w1
    v1 = v * b2 + (w2 * g) * g
    den = np.sqrt(v1) / bc2 + eps
    u = ss * m1 / den
    p1 = p - u
    tol_m = 4 * E * (np.abs(m) + np.abs(g)) + TINY
    tol_v = 4 * E * v1 + TINY
    tol_p = (E * (np.abs(p1) + np.abs(u)) + ss * tol_m / den
             + np.abs(u) * (0.5 * (4 * E + TINY / np.maximum(v1, TINY)) + 6 * E) + TINY)
    return dict(p=p1, m=m1, v=v1, tol_p=tol_p, tol_m=tol_m, tol_v=tol_v)


def adam_fractions(got, ref):
    """(p, m, v) fp32 results -> the worst |got - ref| / tol of each"""
    out = []
    for k, a in zip("pmv", got):
        assert np.isfinite(a).all(), k
        out.append(float((np.abs(a.astype(np.float64) - ref[k]) / ref["tol_" + k]).max()))
    return tuple(out)


def adam_moved_boundaries(case, s9):
    """The self-check of the bound: the reference evaluated with ONE group end moved by one element leaves tol_p at every element
    whose group that changes.  -> the smallest factor by which it does (inf where a case has no boundary to move)."""
    ref = adam_reference(case, s9)
    ends, n = [int(e) for e in case["ends"]], case["n"]
    worst = np.inf
    for k in range(len(ends) - 1):   # (the last end is n by contract)
        for d in (-1, 1):
            moved = list(ends)
            moved[k] += d
            if moved[k] < 0 or moved[k] > n or sorted(moved) != moved:
                continue
            changed = np.nonzero(group_of(n, moved) != group_of(n, ends))[0]
            assert len(changed) == 1 and case["g"][changed[0]] != 0.0
            wrong = adam_reference(case, s9, np.array(moved, np.uint64))
            worst = min(worst, float((np.abs(wrong["p"] - ref["p"]) / ref["tol_p"])[changed[0]]))
    return worst


def adam_run(B, case, s9=None):
    """one step on the backend -> (p, m, v).  s9 given: gsgen_adam_step_device_scalars reading them from the backend's memory"""
    h = [B.put(case[k]) for k in "pgmv"]
    args = (case["n"], B.ptr(h[0]), B.ptr(h[1]), B.ptr(h[2]), B.ptr(h[3]), len(case["ends"]), case["ends"].ctypes.data)
    if s9 is None:
        B.lib.adam_step(*args, case["lrs"].ctypes.data, BETA1, BETA2, ADAM_EPS, case["step"], B.stream)
    else:
        hs = B.put(s9)
        B.lib.adam_step_device_scalars(*args, BETA1, BETA2, ADAM_EPS, B.ptr(hs), B.stream)
    out = (B.get(h[0]), B.get(h[2]), B.get(h[3]))
    assert np.array_equal(B.get(h[1]), case["g"])   # the gradient is read only
    return out


def adam_check(B, n, ends, step):
    """-> (worst fractions of tol_p, tol_m, tol_v; smallest moved-boundary factor)"""
    case = adam_inputs(n, ends, step)
    s9 = adam_scalars(B.lib, case)
    ref = adam_reference(case, s9)
    got = adam_run(B, case)
    fr = adam_fractions(got, ref)
    assert max(fr) <= 1.0, (n, ends, step, fr)
    dev = adam_run(B, case, s9)
    for a, b, k in zip(got, dev, "pmv"):   # the two entry points: identical bits
        assert np.array_equal(bits(a), bits(b)), k
    moved = adam_moved_boundaries(case, s9)
    assert moved > 1.0, (n, ends, step, moved)
    return fr, moved


# ------------------------------------------------------------------------------------------------------------------------------
# 2. SH coefficient bounds
# ------------------------------------------------------------------------------------------------------------------------------
SH_NS = (1, 15, 16, 17, 10923, 16 * 1024 + 17)
SH_CASES = [(N, C, skew) for C in (1, 2, 3, 4) for skew in (0, 1) for N in SH_NS] + [(131072 + 5, 2, 0), (131072 + 5, 2, 1)]
F3E38 = np.float32(3.0e38)


def sh_planted(N):
    return [0, min(N - 1, 15), (N - 1) // 16 * 16, N - 1]


def sh_coeffs(N, C, seed=0):
    CC = C * C
    rng = np.random.default_rng(seed + 31 * C + N)
    sh = (0.05 * rng.normal(size=(N, 3, CC))).astype(np.float32)
    sh[:, :, 0] = 1e6   # the constant term must never count
    if CC > 1:
        for j, i in enumerate(sh_planted(N)):
            sh[i, j % 3, 1 + (5 * j) % (CC - 1)] += np.float32(3.0)
    return sh


def sh_reference(sh):
    """-> (rows64 [N], per-(splat, channel) sums [N, 3]) in fp64"""
    per_row = np.abs(sh[:, :, 1:].astype(np.float64)).sum(-1)
    return per_row.max(-1), per_row


def _sh_launch(B, N, C, hsh):
    """rows + maximum and the plain bound, both over a stale 9e9 -> (rows, out_max, bound, handle of the bound)"""
    hrows, hmax, hb = B.put(np.full(N, 9e9, np.float32)), B.put(np.full(1, 9e9, np.float32)), B.put(np.full(1, 9e9, np.float32))
    B.lib.sh_l1_bound_rows(N, B.ptr(hsh), C, B.ptr(hmax), B.ptr(hrows), B.stream)
    B.lib.sh_l1_bound(N, B.ptr(hsh), C, B.ptr(hb), B.stream)
    return B.get(hrows), B.get(hmax)[0], B.get(hb)[0], hb


def sh_check(B, N, C, skew, variants=True):
    """every assertion of the bound passes on one shape -> worst fraction of the tolerance C^2 E rows64"""
    CC = C * C
    sh = sh_coeffs(N, C)
    rows64, per_row = sh_reference(sh)
    tol = CC * E * rows64
    hsh = B.put(sh, skew)
    assert B.ptr(hsh) % 16 == 4 * skew
    rows, omax, bound, hb = _sh_launch(B, N, C, hsh)
    frac = 0.0
    err = np.abs(rows.astype(np.float64) - rows64)
    assert (err <= tol).all(), (N, C, skew, float((err / np.maximum(tol, 1e-300)).max()))
    if CC > 1:
        frac = float((err / tol).max())
        assert rows64.max() > 3.0 and rows64[N - 1] > 3.0   # (the planted coefficients: the maximum sits where the case put it)
    assert bits(omax) == bits(rows.max())
    assert abs(float(bound) - rows64.max()) <= CC * E * rows64.max()
    if CC > 1:
        frac = max(frac, abs(float(bound) - rows64.max()) / (CC * E * rows64.max()))
    # the running form: a larger value stays, a zeroed one rises to exactly out_max; out_max = NULL
    hbig, hzero = B.put(np.full(1, 1e30, np.float32)), B.put(np.zeros(1, np.float32))
    hr2, hr3, hr4 = (B.put(np.full(N, 9e9, np.float32)) for _ in range(3))
    B.lib.sh_l1_bound_rows_running(N, B.ptr(hsh), C, B.ptr(hbig), B.ptr(hr2), B.stream)
    B.lib.sh_l1_bound_rows_running(N, B.ptr(hsh), C, B.ptr(hzero), B.ptr(hr3), B.stream)
    B.lib.sh_l1_bound_rows(N, B.ptr(hsh), C, None, B.ptr(hr4), B.stream)
    assert B.get(hbig)[0] == np.float32(1e30) and bits(B.get(hzero)[0]) == bits(omax)
    for h in (hr2, hr3, hr4):
        assert np.array_equal(bits(B.get(h)), bits(rows))
    # the check: strict > against the bound itself, and the number of ROWS (splat, channel) above 2.0
    assert not (np.abs(per_row - 2.0) <= CC * E * 2.0 * 4).any()   # (no row of the case is near the threshold)
    hbad, h2 = B.put(np.full(1, 77, np.uint32)), B.put(np.full(1, 2.0, np.float32))
    B.lib.sh_l1_bound_check(N, B.ptr(hsh), C, B.ptr(hb), B.ptr(hbad), B.stream)
    assert B.get(hbad)[0] == 0
    B.lib.sh_l1_bound_check(N, B.ptr(hsh), C, B.ptr(h2), B.ptr(hbad), B.stream)
    assert B.get(hbad)[0] == int((per_row > 2.0).sum())
    assert CC == 1 or int((per_row > 2.0).sum()) >= 1
    if not variants:
        return frac
    # all higher bands zero: 0 everywhere (at C == 1 there are none: the case above already is this one)
    z = sh.copy()
    z[:, :, 1:] = 0.0
    rz, mz, bz, _ = _sh_launch(B, N, C, B.put(z, skew))
    assert not rz.any() and bits(mz) == 0 and bits(bz) == 0
    if CC == 1:
        assert not rows.any() and bits(omax) == 0 and bits(bound) == 0
        return frac
    # NaN: that splat's row and both maxima read 3e38 ("no bound"); +Inf: inf.  In the last, partial group of 16.
    for bad, want in ((np.float32(np.nan), F3E38), (np.float32(np.inf), np.float32(np.inf))):
        x = sh.copy()
        i = N - 1 if N < 3 else N - 2
        x[i, 1, CC - 1] = bad
        rx, mx, bx, _ = _sh_launch(B, N, C, B.put(x, skew))
        assert rx[i] == want and mx == want and bx == want, (N, C, skew, bad, rx[i], mx, bx)
        keep = np.arange(N) != i
        assert np.array_equal(bits(rx[keep]), bits(rows[keep]))
    return frac


# ------------------------------------------------------------------------------------------------------------------------------
# 3. densify / prune statistics
# ------------------------------------------------------------------------------------------------------------------------------
DENSIFY_NS = (1, 255, 256, 257)
DENSIFY_VIEWS = (1, 16, 17, 33)
LATE_VIEW = 20   # a view of the second launch's chunk (16 views per launch)


def densify_case(N, n_views, null_view, seed=0):
    """null_view: the mask of view min(2, n_views - 1) is NULL (every Gaussian visible there); otherwise every view has a mask, one
    Gaussian is visible in none and one only in view LATE_VIEW.  Both: a NaN covariance in one view, a negative-trace Gaussian."""
    rng = np.random.default_rng(seed + 100 * N + n_views + (5000 if null_view else 0))
    A = rng.normal(size=(n_views, N, 2, 2)) * 0.02
    covs = [np.ascontiguousarray((A[v] @ A[v].transpose(0, 2, 1)).reshape(N, 4) * (0.5 + 0.1 * v), np.float32) for v in range(n_views)]
    gms = [(rng.normal(size=(N, 2)) * 1e-3 * (1 + v)).astype(np.float32) for v in range(n_views)]
    masks = [(rng.random(N) < 0.6).astype(np.uint8) for _ in range(n_views)]
    prior = [(rng.random(N) * 1e-3).astype(np.float32), rng.random(N).astype(np.float32), rng.integers(0, 5, N).astype(np.float32)]
    sp = {}
    if N >= 8:
        sp = dict(unseen=N - 1, late=N - 2, nan=N - 3, neg=0)
        nan_view = min(1, n_views - 1)
        covs[nan_view][sp["nan"]] = np.nan
        masks[nan_view][sp["nan"]] = 1
        masks[n_views - 1][sp["nan"]] = 1   # (seen again with a finite radius: in the second launch where there is one)
        for v in range(n_views):
            a, b = rng.random(2) * 1e-3 + 1e-4
            covs[v][sp["neg"]] = (-a, 0.0, 0.0, -b)
            masks[v][sp["neg"]] = 1
            if not null_view:
                masks[v][sp["unseen"]] = 0
                masks[v][sp["late"]] = 1 if v == LATE_VIEW else 0
        prior[1][sp["unseen"]], prior[2][sp["unseen"]] = 0.375, 3.0
        prior[0][sp["unseen"]] = 2.5e-4
        prior[0][sp["neg"]] = 0.0
    if null_view:
        masks[min(2, n_views - 1)] = None
    return dict(N=N, n_views=n_views, covs=covs, gms=gms, masks=masks, prior=prior, special=sp, null_view=null_view)


def densify_reference(case):
    """oracle.densify_update view by view -> (max_radii2d, grad_accum, cnt, bound on grad_accum)"""
    from oracle import oracle as O
    ref = [a.copy() for a in case["prior"]]
    total = case["prior"][1].astype(np.float64)
    for cov, gm, mask in zip(case["covs"], case["gms"], case["masks"]):
        O.densify_update(cov, gm, mask, *ref)
        seen = np.ones(case["N"], bool) if mask is None else mask.astype(bool)
        total = total + np.where(seen, np.sqrt((gm.astype(np.float64) ** 2).sum(-1)), 0.0)
    return ref[0], ref[1], ref[2], (case["n_views"] + 1) * E * total


def densify_check(B, N, n_views, null_view):
    """-> worst fraction of the grad_accum bound"""
    case = densify_case(N, n_views, null_view)
    want_r, want_a, want_c, tol = densify_reference(case)
    nv, lib, sp = n_views, B.lib, case["special"]
    hc, hg = [B.put(a) for a in case["covs"]], [B.put(a) for a in case["gms"]]
    hm = [None if a is None else B.put(a) for a in case["masks"]]
    tab = lambda hs: (ctypes.c_void_p * nv)(*[B.ptr(h) for h in hs])  # noqa: E731
    fresh = lambda: [B.put(a) for a in case["prior"]]  # noqa: E731
    st = fresh()
    lib.densify_update_batch(nv, N, tab(hc), tab(hg), tab(hm), B.ptr(st[0]), B.ptr(st[1]), B.ptr(st[2]), B.stream)
    r, a, c = (B.get(h) for h in st)
    assert np.array_equal(bits(r), bits(want_r)), np.nonzero(bits(r) != bits(want_r))[0][:8]
    assert np.array_equal(bits(c), bits(want_c))
    err = np.abs(a.astype(np.float64) - want_a.astype(np.float64))
    assert (err <= tol).all()
    frac = float((err / tol).max())
    if sp:
        assert np.isnan(r[sp["nan"]]) and r[sp["neg"]] == case["prior"][0][sp["neg"]]
        if not null_view:
            for h, k in zip((r, a, c), range(3)):   # visible in no view: untouched
                assert bits(h[sp["unseen"]]) == bits(case["prior"][k][sp["unseen"]])
            assert c[sp["late"]] == case["prior"][2][sp["late"]] + (1.0 if nv > LATE_VIEW else 0.0)
        # NaN still sticks after a later launch with finite radii (the single-view form, every Gaussian visible)
        fin = np.tile(np.array([4e-4, 0, 0, 4e-4], np.float32), (N, 1))
        later, hfin = B.put(r), B.put(fin)
        lib.densify_update(N, B.ptr(hfin), None, None, B.ptr(later), None, None, B.stream)
        later = B.get(later)
        assert np.isnan(later[sp["nan"]]) and later[sp["neg"]] == np.float32(4e-4) and (later[:-3] >= r[:-3]).all()
    # the halves on their own: radii only; the gradient sum without the count
    st2 = fresh()
    lib.densify_update_batch(nv, N, tab(hc), None, tab(hm), B.ptr(st2[0]), None, None, B.stream)
    lib.densify_update_batch(nv, N, None, tab(hg), tab(hm), None, B.ptr(st2[1]), None, B.stream)
    assert np.array_equal(bits(B.get(st2[0])), bits(want_r)) and np.array_equal(B.get(st2[2]), case["prior"][2])
    assert (np.abs(B.get(st2[1]).astype(np.float64) - want_a) <= tol).all()
    # the single-view form on view 0 == the oracle's statement
    from oracle import oracle as O
    one, st3 = [x.copy() for x in case["prior"]], fresh()
    O.densify_update(case["covs"][0], case["gms"][0], case["masks"][0], *one)
    lib.densify_update(N, B.ptr(hc[0]), B.ptr(hg[0]), B.ptr(hm[0]), B.ptr(st3[0]), B.ptr(st3[1]), B.ptr(st3[2]), B.stream)
    for h, w in zip(st3, one):
        assert np.array_equal(bits(B.get(h)), bits(w))
    st4 = fresh()
    lib.densify_update(N, B.ptr(hc[0]), None, B.ptr(hm[0]), B.ptr(st4[0]), None, None, B.stream)
    lib.densify_update(N, None, B.ptr(hg[0]), B.ptr(hm[0]), None, B.ptr(st4[1]), None, B.stream)
    assert np.array_equal(bits(B.get(st4[0])), bits(one[0])) and np.array_equal(bits(B.get(st4[1])), bits(one[1]))
    assert np.array_equal(B.get(st4[2]), case["prior"][2])
    # the pairs that must come together
    EI, p = einval(), B.ptr
    before = [B.get(h) for h in st]
    for args in ((tab(hc), None, None, None, None, None), (None, tab(hg), None, None, None, None),
                 (tab(hc), None, None, p(st[0]), None, p(st[2])), (None, None, None, p(st[0]), None, None),
                 (None, None, None, None, p(st[1]), None)):
        assert rc(lib.densify_update_batch, nv, N, *args, B.stream) == EI
    for args in ((p(hc[0]), None, None, None, None, None), (None, p(hg[0]), None, None, None, None),
                 (p(hc[0]), None, None, p(st[0]), None, p(st[2])), (None, None, None, p(st[0]), None, None),
                 (None, None, None, None, p(st[1]), None)):
        assert rc(lib.densify_update, N, *args, B.stream) == EI
    for h, b in zip(st, before):   # nothing was launched
        assert np.array_equal(bits(B.get(h)), bits(b))
    return frac
