"""The kernels of a training step that are not the render, on the device at their edges: the cases of tests/step_cases.py (fused Adam
step, SH coefficient bounds, densify / prune statistics -- the same ones tests/test_step_kernels_host.py runs on the emulator) through
the C ABI on device tensors, the two Adam entry points and the two FusedAdam forms bit against bit, and renders whose parameters are
FusedAdam's views of one flat buffer at sizes where those views are only 4-byte aligned."""
import numpy as np
import pytest
import torch

import scenes
import step_cases as S

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


class GpuBackend:
    """step_cases' backend on device tensors: a handle is a typed view into a byte tensor, 16-byte aligned plus 4 * skew bytes"""

    def __init__(self):
        from gsgen_amd import _capi
        self.lib = _capi.load()
        self.stream = torch.cuda.current_stream(dev()).cuda_stream

    def put(self, a, skew=0):
        a = np.ascontiguousarray(a)
        raw = torch.empty(a.nbytes + 32, dtype=torch.uint8, device=dev())
        assert raw.data_ptr() % 16 == 0
        h = raw[4 * skew:4 * skew + a.nbytes]
        h.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))
        h._np = (a.dtype, a.shape)
        return h

    def ptr(self, h):
        return None if h is None else h.data_ptr()

    def get(self, h):
        dtype, shape = h._np
        return h.cpu().numpy().view(dtype).reshape(shape).copy()


@pytest.fixture(scope="module")
def gpu():
    return GpuBackend()


@pytest.mark.parametrize("n,ends", S.ADAM_CASES, ids=[f"n{n}" for n, _ in S.ADAM_CASES])
def test_adam_step_within_rounding_bounds(gpu, n, ends):
    """gsgen_adam_step against the fp64 reference at the per-entry rounding bounds, every step count; inside adam_check also:
    gsgen_adam_step_device_scalars on the same inputs gives identical bits in p, m and v"""
    worst = [0.0, 0.0, 0.0]
    for step in S.ADAM_STEPS:
        fr, _ = S.adam_check(gpu, n, ends, step)
        worst = [max(a, b) for a, b in zip(worst, fr)]
    print(f"[adam gpu] n={n}: worst fraction of tol_p / tol_m / tol_v = {worst[0]:.3f} / {worst[1]:.3f} / {worst[2]:.3f}")


@pytest.mark.parametrize("N,C,skew", S.SH_CASES, ids=[f"N{N}-C{C}-{'skew4' if k else 'aligned'}" for N, C, k in S.SH_CASES])
def test_sh_bounds_against_fp64(gpu, N, C, skew):
    frac = S.sh_check(gpu, N, C, skew)
    print(f"[sh bound gpu] N={N} C={C} base%16={4 * skew}: worst fraction of C^2 E rows64 = {frac:.3f}")


@pytest.mark.parametrize("null_view", [True, False])
@pytest.mark.parametrize("n_views", S.DENSIFY_VIEWS)
@pytest.mark.parametrize("N", S.DENSIFY_NS)
def test_densify_statistics_against_the_oracle(gpu, N, n_views, null_view):
    frac = S.densify_check(gpu, N, n_views, null_view)
    print(f"[densify gpu] N={N} views={n_views} null_view={null_view}: worst fraction of the grad_accum bound = {frac:.3f}")


def test_fused_adam_forms_agree_bit_for_bit():
    """FusedAdam(...) and FusedAdam(..., capturable=True): five fields of 37 rows, three steps, the same gradients, learning rates
    that change every step -- parameters and both moments identical bits"""
    from gsgen_amd.optim import FusedAdam
    gen = torch.Generator().manual_seed(0)
    shapes = {"mean": (37, 3), "qvec": (37, 4), "svec": (37, 3), "color": (37, 3), "alpha": (37,)}
    init = {k: torch.randn(*sh, generator=gen).to(dev()) for k, sh in shapes.items()}
    lr0 = {"mean": 5e-3, "qvec": 1e-3, "svec": 5e-3, "color": 1e-2, "alpha": 3e-2}
    a, b = FusedAdam(init, lr0), FusedAdam(init, lr0, capturable=True)
    assert a.n == 37 * 14 and a.n % 4 != 0
    for step in range(1, 4):
        g = (torch.randn(a.n, generator=gen) * 10.0 ** (step - 3)).to(dev())
        lrs = {k: v * (1.0 + 0.5 * step) / step ** 2 for k, v in lr0.items()}
        for o in (a, b):
            o.grad.copy_(g)
            o.step(lrs)
        torch.cuda.synchronize()
        assert a.step_count == b.step_count == step
        for x, y, what in ((a.flat, b.flat, "p"), (a.exp_avg, b.exp_avg, "m"), (a.exp_avg_sq, b.exp_avg_sq, "v")):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (step, what)
    assert not torch.equal(a.flat, torch.cat([init[k].reshape(-1) for k in shapes]))
    for k in shapes:   # the parameters handed out are still the views
        assert torch.equal(a.params[k].detach(), b.params[k].detach())


@pytest.mark.parametrize("N", [1001, 1002, 1003])
def test_renders_from_the_flat_buffer_views_at_4_byte_alignment(N):
    """BatchRenderer on FusedAdam's parameter views where N % 4 != 0 puts qvec (3 N floats in), svec (7 N), sh (11 N) and colour off
    16-byte alignment, against the same renders on freshly allocated copies of the same values: C = 4 routed ("auto": the polynomial
    kernel, whose transform reads sh as float4 from global memory) and exact, C = 0, and render_heads on raw fields with activations.
    Forward images and T: identical bits (the same kernels on the same values; the forward is deterministic).  Gradients: within
    per_gaussian_grad_error(rtol=1e-4, atol=1e-6), the allowance for two orders of the backward's atomics."""
    from gsgen_amd import _capi
    from gsgen_amd import batch as Bm
    from gsgen_amd import renderer as R
    from gsgen_amd.optim import FusedAdam
    T_ = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev())  # noqa: E731
    sc = scenes.random_scene(N, seed=N, svec=0.04, spread=0.25, C=4)
    sc["sh"][:, :, 1:] *= 0.02
    W, H = 64, 48
    cams = [scenes.Camera(W, H, fx=fx, c2w=scenes.orbit(2.5, 10 + 20 * i, 40.0 + 100 * i)) for i, fx in enumerate((260.0, 300.0))]
    cis, c2ws = [R.CameraInfo(*c.intr) for c in cams], [c.c2w for c in cams]
    S_ = R.sh_l1_bound(T_(sc["sh"]))
    assert all(_capi.load().sh_poly_applies(S_, 1.0 / c.fx, 4) for c in cams)   # "auto" runs the polynomial kernel in both views
    logit = lambda x: np.log(np.clip(x, 1e-3, 1 - 1e-3) / (1 - np.clip(x, 1e-3, 1 - 1e-3)))  # noqa: E731
    keys = ("mean", "qvec", "svec", "alpha", "sh", "color")
    fa = FusedAdam({k: T_(sc[k]) for k in keys}, {k: 1e-3 for k in keys})
    rkeys = ("mean", "qvec", "svec", "alpha", "color")
    raw = FusedAdam({"mean": T_(sc["mean"]), "qvec": T_(sc["qvec"]), "svec": T_(np.log(sc["svec"])), "alpha": T_(logit(sc["alpha"])),
                     "color": T_(logit(sc["color"]))}, {k: 1e-3 for k in rkeys})
    for o, ks in ((fa, ("qvec", "svec", "sh", "color")), (raw, ("qvec", "svec", "color"))):
        assert o.flat.data_ptr() % 16 == 0
        for k in ks:
            off = {"qvec": 3 * N, "svec": 7 * N, "alpha": 10 * N, "sh": 11 * N, "color": (59 if o is fa else 11) * N}[k]
            assert o.params[k].data_ptr() == o.flat.data_ptr() + 4 * off
            assert o.params[k].data_ptr() % 16 == (4 * off) % 16 != 0, k
            assert o.params[k].grad.data_ptr() % 16 != 0
    gen = torch.Generator(device=dev()).manual_seed(3)
    go3 = torch.randn(2, H, W, 3, device=dev(), generator=gen)
    go1 = [torch.randn(2, H, W, 1, device=dev(), generator=gen) for _ in range(3)]

    def run(views):
        if views:
            P, Q = fa.params, raw.params
            fa.zero_grad(); raw.zero_grad()
        else:   # freshly allocated tensors of the same values
            P = {k: fa.params[k].detach().clone().requires_grad_(True) for k in keys}
            Q = {k: raw.params[k].detach().clone().requires_grad_(True) for k in rkeys}
            assert all(t.data_ptr() % 16 == 0 for t in list(P.values()) + list(Q.values()))
        br = Bm.BatchRenderer(N, W, H, dev(), max_batch=2)
        out, grads = {}, {}

        def take(name, P_, ks, outs, gos):
            sum((o * g).sum() for o, g in zip(outs, gos)).backward()
            torch.cuda.synchronize()
            out[name] = [o.detach().cpu().numpy() for o in outs]
            grads[name] = {k: P_[k].grad.detach().cpu().numpy().copy() for k in ks}
            for k in ks:
                P_[k].grad.zero_()

        geo = ("mean", "qvec", "svec", "alpha")
        for basis in ("auto", "exact"):
            rgb, T = br.render(P["mean"], P["qvec"], P["svec"], P["alpha"], P["sh"], cis, c2ws, C=4, sh_basis=basis)
            take("sh-" + basis, P, geo + ("sh",), (rgb, T.detach()), (go3, go1[0]))
        rgb, T = br.render(P["mean"], P["qvec"], P["svec"], P["alpha"], P["color"], cis, c2ws, C=0)
        take("rgb", P, geo + ("color",), (rgb, T.detach()), (go3, go1[0]))
        rgb, dep, opa, d2, T = br.render_heads(Q["mean"], Q["qvec"], Q["svec"], Q["alpha"], Q["color"], cis, c2ws,
                                               activations=("exp", "sigmoid", "sigmoid"))
        take("heads", Q, rkeys, (rgb, dep, opa, d2, T.detach()), (go3, go1[0], go1[1], go1[2], go1[0]))
        if views:   # autograd accumulated straight into the flat gradient
            assert fa.params["sh"].grad.data_ptr() == fa.grad.data_ptr() + 4 * 11 * N
        return out, grads

    o_v, g_v = run(True)
    o_c, g_c = run(False)
    worst = 0.0
    for name in o_c:
        for a, b in zip(o_v[name], o_c[name]):
            assert np.isfinite(b).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
        assert np.abs(o_c[name][0]).max() > 0.05   # (the cameras do see the scene)
        for k, want in g_c[name].items():
            assert np.abs(want).max() > 0, (name, k)
            ratio, row = scenes.per_gaussian_grad_error(g_v[name][k], want, rtol=1e-4, atol=1e-6)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, k, ratio, row)
    assert np.abs(o_c["sh-auto"][0] - o_c["sh-exact"][0]).max() > 0   # the routed render did take another kernel
    print(f"[flat views] N={N}: worst per-Gaussian gradient error = {worst:.3f} of its allowance")
