"""gsgen_amd.guidance on the MI355X against the torch restatements of tests/guidance_cases.py, to the bound those restatements' own fp32
error sets (no fixed tolerance), and the properties a trainer relies on: the exact identity, adjointness, agreement with torch's own
F.interpolate on the device, bit equality from run to run, the table cache, a captured forward + backward whose replay sees new values,
and the seam behind a BatchRenderer render against the reference's torch sequences."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guidance_cases as GC
import scenes
from refpy_cases import rel_rows

pytestmark = pytest.mark.gpu

from gsgen_amd import _capi  # noqa: E402
from gsgen_amd import guidance as GG  # noqa: E402

DEV = "cuda"


def dev(a):
    return torch.as_tensor(np.array(a)).to(DEV)  # (a copy: the cases' arrays are read-only)


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def as_bhwc(t, layout):
    """a kernel's output as a float32 [B,OH,OW,C] array"""
    t = t.detach().float()
    return (t.permute(0, 2, 3, 1) if layout == "BCHW" else t).cpu().numpy()


def in_layout(g, layout, half):
    """an upstream gradient [B,OH,OW,C] array as the tensor autograd hands the kernel"""
    t = dev(g)
    t = t.permute(0, 3, 1, 2).contiguous() if layout == "BCHW" else t
    return t.half() if half else t


def raw_backward(g, shape, scale, planar):
    """gsgen_guidance_input_backward itself (autograd only ever delivers the output's dtype: this reaches the other pairings), through
    the tables a forward with these sizes built"""
    B, H, W, Cc = shape
    OH, OW = (g.shape[2], g.shape[3]) if planar else (g.shape[1], g.shape[2])
    lib = _capi.load()
    ws, nbytes, build = GG._tables(lib, g.device, H, W, OH, OW)
    assert build == 0  # (the forward before this call made them)
    gx = torch.full(shape, 7.0, device=DEV)
    lib.guidance_input_backward(g.data_ptr(), int(g.dtype == torch.float16), int(planar), B, H, W, Cc, OH, OW, scale, gx.data_ptr(), ws.data_ptr(),
                                nbytes, torch.cuda.current_stream().cuda_stream)
    return gx


@pytest.mark.parametrize("case", GC.RESIZE_CASES, ids=GC.resize_id)
def test_resize_meets_the_restatements_own_error(case):
    H, W, OH, OW, Cc, B = case
    d = GC.resize_case(case)
    name = GC.resize_id(case)
    dead_y, dead_x = GC.untouched(H, OH), GC.untouched(W, OW)
    for layout in GG.LAYOUTS:
        for half in (False, True):
            x = dev(d["x"]).requires_grad_(True)
            out = GG.to_guidance(x, (OH, OW), GC.SCALE, GC.SHIFT, torch.float16 if half else torch.float32, layout)
            assert out.shape == ((B, Cc, OH, OW) if layout == "BCHW" else (B, OH, OW, Cc)) and out.is_contiguous()
            assert out.dtype == (torch.float16 if half else torch.float32) and out.requires_grad
            GC.check(f"{name} out {layout} half={half}", as_bhwc(out, layout), d["out64"], d["out32"], half)
            which = "16" if half else "32"
            out.backward(in_layout(d["g" + which], layout, half))
            gx = x.grad.cpu().numpy()
            GC.check(f"{name} grad {layout} g_half={half}", gx, d[f"gx{which}64"], d[f"gx{which}32"])
            assert not gx[:, dead_y].any() and not gx[:, :, dead_x].any()  # an input no output reads: exact zeros
            # the other pairing of output and upstream types, through the C entry point
            other = "32" if half else "16"
            gx2 = raw_backward(in_layout(d["g" + other], layout, not half), tuple(x.shape), GC.SCALE, layout == "BCHW").cpu().numpy()
            GC.check(f"{name} grad {layout} g_half={not half} (raw)", gx2, d[f"gx{other}64"], d[f"gx{other}32"])
            assert not gx2[:, dead_y].any() and not gx2[:, :, dead_x].any()


def test_identity_is_bit_exact():
    """16 x 16 -> 16 x 16: every l1 is 0, so the fp32 forward is x * 2 - 1 in fp32 and the backward 2 * g, bit for bit"""
    for case in ((16, 16, 16, 16, 3, 3), (16, 16, 16, 16, 1, 3)):
        d = GC.resize_case(case)
        for layout in GG.LAYOUTS:
            x = dev(d["x"]).requires_grad_(True)
            out = GG.to_guidance(x, 16, 2.0, -1.0, torch.float32, layout)
            want = x.detach() * 2.0 - 1.0
            assert torch.equal(bits(out), bits(want.permute(0, 3, 1, 2) if layout == "BCHW" else want))
            g = in_layout(d["g32"], layout, False)
            out.backward(g)
            want_g = 2.0 * dev(d["g32"])
            assert torch.equal(bits(x.grad), bits(want_g))
            plain = GG.to_guidance(x.detach(), 16, 1.0, 0.0, torch.float32, "BHWC")
            assert torch.equal(bits(plain), bits(x))


@pytest.mark.parametrize("case", [c for c in GC.RESIZE_CASES if c[5] == 3 and c[4] == 3], ids=GC.resize_id)
def test_adjoint_and_agreement_with_torchs_interpolate_on_the_device(case):
    """<forward(x), g> = <x, backward(g)> for the fp32, no-affine form, to the bound tests/test_guidance_host.py derives for the two
    sums; and output and gradient against F.interpolate's on the device, within the restatement's bound"""
    H, W, OH, OW, Cc, B = case
    d = GC.resize_case(case)
    name = GC.resize_id(case)
    x = dev(d["x"]).requires_grad_(True)
    out = GG.to_guidance(x, (OH, OW), 1.0, 0.0, torch.float32, "BCHW")
    gt = in_layout(d["g32"], "BCHW", False)
    out.backward(gt)
    g, x64 = d["g32"].astype(np.float64), d["x"].astype(np.float64)
    lhs, rhs = (as_bhwc(out, "BCHW").astype(np.float64) * g).sum(), (x64 * x.grad.cpu().numpy().astype(np.float64)).sum()
    e32 = abs((d["out_plain32"] * g).sum() - (x64 * d["gx32_plain32"]).sum())
    bound = 4 * max(e32, GC.FLOOR * np.abs(d["out_plain64"] * g).sum())
    print(f"{name}: <f(x), g> {lhs:.9e} <x, b(g)> {rhs:.9e} differ by {abs(lhs - rhs):.3e} bound {bound:.3e} (fp32 torch {e32:.3e})")
    assert abs(lhs - rhs) <= bound
    xt = dev(d["x"]).requires_grad_(True)
    ref = F.interpolate(xt.permute(0, 3, 1, 2), (OH, OW), mode="bilinear", align_corners=False)
    ref.backward(gt)
    for what, a, b, y64, y32 in (("out", out, ref, d["out_plain64"], d["out_plain32"]),
                                 ("grad", x.grad, xt.grad, d["gx32_plain64"], d["gx32_plain32"])):
        a = as_bhwc(a, "BCHW") if what == "out" else a.cpu().numpy()
        b = as_bhwc(b, "BCHW") if what == "out" else b.cpu().numpy()
        tol = 4 * max(np.abs(y32 - y64).max(), GC.FLOOR * np.abs(y64).max())
        diff = np.abs(a.astype(np.float64) - b).max()
        print(f"{name}: {what} against F.interpolate on the device: {diff:.3e} bound {tol:.3e}")
        assert diff <= tol
        GC.check(f"{name} plain {what}", a, y64, y32)


def test_run_to_run_bit_equality_the_table_cache_and_a_side_stream():
    case = (130, 70, 32, 48, 3, 3)
    d = GC.resize_case(case)

    def once(layout, half):
        x = dev(d["x"]).requires_grad_(True)
        out = GG.to_guidance(x, (32, 48), 2.0, -1.0, torch.float16 if half else torch.float32, layout)
        out.backward(in_layout(d["g16"], layout, half))
        return out, x.grad
    for layout in GG.LAYOUTS:
        for half in (False, True):
            a, b = once(layout, half), once(layout, half)  # (the second reads the cached tables)
            assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
            assert a[1].abs().max() > 0
    key = [k for k in GG._TABLES if k[2:] == (130, 70, 32, 48)]
    assert len(key) == 1
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    a = once("BCHW", True)
    with torch.cuda.stream(s):
        b = once("BCHW", True)  # (another stream: tables of its own)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))
    assert len([k for k in GG._TABLES if k[2:] == (130, 70, 32, 48)]) == 2


def test_the_call_shapes_of_the_reference():
    import gsgen_amd
    gen = torch.Generator(DEV).manual_seed(3)
    rgb = torch.rand(2, 24, 20, 3, device=DEV, generator=gen)
    v = GG.vae_input(rgb, 40)
    assert v.shape == (2, 3, 40, 40) and v.dtype == torch.float16
    assert torch.equal(bits(v), bits(GG.to_guidance(rgb, (40, 40), 2.0, -1.0, torch.float16, "BCHW")))
    assert torch.equal(bits(gsgen_amd.vae_input(rgb, 40)), bits(v))
    assert GG.vae_input(rgb[:, :6, :5]).shape == (2, 3, 512, 512)
    f = GG.if_input(rgb)
    assert f.shape == (2, 3, 64, 64) and f.dtype == torch.float32
    lat = GG.rgb_as_latents(rgb)
    assert lat.shape == (2, 3, 64, 64) and lat.dtype == torch.float32
    assert torch.equal(bits(f), bits(lat * 2.0 - 1.0))  # (the affine is one multiply and one add after the interpolation)
    r = GG.resize(rgb, (12, 30))
    assert r.shape == (2, 12, 30, 3) and r.dtype == torch.float32
    one = GG.resize(rgb[1], (12, 30))
    assert one.shape == (12, 30, 3) and torch.equal(bits(one), bits(r[1]))
    depth = torch.rand(2, 24, 20, 1, device=DEV, generator=gen)
    assert GG.resize(depth, 9).shape == (2, 9, 9, 1)
    assert GG.vae_input(rgb[0], 40).shape == (1, 3, 40, 40)
    # a strided view takes its gradient in the caller's layout
    full = torch.rand(2, 30, 26, 3, device=DEV, generator=gen).requires_grad_(True)
    crop = (slice(None), slice(3, 27), slice(2, 22))
    a = GG.vae_input(full[crop], 40)
    a.float().sum().backward()
    ref = full.detach()[crop].contiguous().requires_grad_(True)
    b = GG.vae_input(ref, 40)
    b.float().sum().backward()
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(full.grad[crop]), bits(ref.grad)) and ref.grad.abs().max() > 0
    # no gradient asked: none made
    assert not GG.vae_input(rgb, 40).requires_grad


def test_forward_and_backward_replay_in_a_captured_graph_on_new_images():
    case = (23, 7, 7, 13, 3, 3)
    d = GC.resize_case(case)
    x = dev(d["x"]).requires_grad_(True)
    g = in_layout(d["g16"], "BCHW", True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        GG.vae_input(x, (7, 13)).backward(g)  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = GG.vae_input(x, (7, 13))
        out.backward(g)
    gen = torch.Generator().manual_seed(77)
    for k in range(3):
        x_new, g_new = torch.rand(x.shape, generator=gen), torch.randn(g.shape, generator=gen).half()
        with torch.no_grad():
            x.copy_(x_new.to(DEV))
            g.copy_(g_new.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone(), x.grad.clone()
        e = x_new.to(DEV).requires_grad_(True)
        eo = GG.vae_input(e, (7, 13))
        eo.backward(g_new.to(DEV))
        assert torch.equal(bits(got[0]), bits(eo)) and torch.equal(bits(got[1]), bits(e.grad)), k
        assert got[1].abs().max() > 0


# ---- the SDS loss --------------------------------------------------------------------------------------------------------------
def run_sds(latents, grad, clip, scale=None, need_grad=True):
    lt = dev(latents).requires_grad_(need_grad)
    loss, each, norm = GG.sds_loss(lt, dev(grad), clip)
    assert loss.shape == () and norm.shape == () and each.shape == (lt.shape[0],)
    assert loss.dtype == each.dtype == norm.dtype == torch.float32
    assert loss.requires_grad == need_grad and not each.requires_grad and not norm.requires_grad
    if need_grad:
        (loss if scale is None else scale * loss).backward()
        assert lt.grad.shape == lt.shape
    return loss.detach().cpu().numpy(), each.cpu().numpy(), norm.cpu().numpy(), lt.grad.cpu().numpy() if need_grad else None


@pytest.mark.parametrize("case", GC.SDS_CASES, ids=GC.sds_id)
def test_sds_loss_meets_the_restatements_own_error(case):
    d = GC.sds_case(case)
    loss, each, norm, g = run_sds(d["latents"], d["grad"], case[1])
    GC.check_sds(case, loss, each, norm, g)
    assert np.isfinite(loss) and np.isfinite(each).all() and np.isfinite(norm) and np.isfinite(g).all()
    if case[2] == "zeros":
        assert loss == 0.0 and norm == 0.0 and not each.any() and not g.any()
    if case[2] == "nonfinite":
        assert (np.abs(g[np.isinf(d["grad"])]) == np.float32(case[1]) / np.float32(case[0][0])).all()  # +-inf: clipped
    again = run_sds(d["latents"], d["grad"], case[1])
    assert all(a.tobytes() == b.tobytes() for a, b in zip((loss, each, norm, g), again))  # bit-identical from run to run
    only = run_sds(d["latents"], d["grad"], case[1], need_grad=False)
    assert only[0].tobytes() == loss.tobytes() and only[1].tobytes() == each.tobytes() and only[2].tobytes() == norm.tobytes()
    _, _, _, g3 = run_sds(d["latents"], d["grad"], case[1], scale=3.0)
    GC.check_sds(case, loss, each, norm, g3, scale=3.0)
    _, _, _, g2 = run_sds(d["latents"], d["grad"], case[1], scale=2.0)
    assert g2.tobytes() == (2.0 * g).astype(np.float32).tobytes()


def test_sds_grad_is_detached_and_the_package_name():
    import gsgen_amd
    case = GC.SDS_CASES[3]
    d = GC.sds_case(case)
    lt, gr = dev(d["latents"]).requires_grad_(True), dev(d["grad"]).requires_grad_(True)
    loss, each, norm = gsgen_amd.sds_loss(lt, gr, grad_clip_val=case[1])
    loss.backward()
    assert gr.grad is None and lt.grad is not None
    GC.check_sds(case, loss.item(), each.cpu().numpy(), norm.item(), lt.grad.cpu().numpy())


def test_sds_replays_in_a_captured_graph_on_new_values():
    case = ((2, 4, 5, 7), 1.0, "nonfinite")
    lat0, grad0 = GC.sds_inputs(case)
    lt, gr = dev(lat0).requires_grad_(True), dev(grad0)
    scale = torch.tensor(1.0, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        (GG.sds_loss(lt, gr, 1.0)[0] * scale).backward()  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    lt.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, each, norm = GG.sds_loss(lt, gr, 1.0)
        (loss * scale).backward()
    for k in range(1, 4):
        lat_new, grad_new = GC.sds_inputs(case, seed_offset=k)
        with torch.no_grad():
            lt.copy_(dev(lat_new))
            gr.copy_(dev(grad_new))
            scale.fill_(1.0 + k)  # (the upstream scalar is read on the device: a replay sees the new one)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in (loss, each, norm, lt.grad)]
        e = dev(lat_new).requires_grad_(True)
        el, ee, en = GG.sds_loss(e, dev(grad_new), 1.0)
        (el * (1.0 + k)).backward()
        for a, b in zip(got, (el, ee, en, e.grad)):
            assert torch.equal(bits(a), bits(b)), k
        assert got[3].abs().max() > 0 and np.isfinite(got[0].item())


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_the_seam_behind_a_batch_heads_render():
    """BatchRenderer heads render of two 64 x 64 views -> vae_input at 32 x 32 -> a fixed random linear stand-in for the encoder ->
    sds_loss -> backward, against the same step with the reference's torch sequences (stable_diffusion.py:274-312): the parameter
    gradients per Gaussian at the suite's rtol"""
    from gsgen_amd import renderer as R
    from gsgen_amd.batch import BatchRenderer
    sc = scenes.random_scene(3000, seed=7, svec=0.05)
    N, W, H, S = sc["mean"].shape[0], 64, 64, 32
    cams = [scenes.Camera(W, H, fx=70.0, c2w=scenes.orbit(2.4, 10 + 5 * i, 70.0 * i)) for i in range(2)]
    cis = [R.CameraInfo(*cam.intr) for cam in cams]
    names = ("mean", "qvec", "svec", "alpha", "color")
    P = {k: dev(sc[k]).requires_grad_(True) for k in names}
    gen = torch.Generator(DEV).manual_seed(1)
    enc = torch.randn(3 * S * S, 4 * 8 * 8, device=DEV, generator=gen) / (3 * S * S) ** 0.5
    noise = torch.randn(2, 4, 8, 8, device=DEV, generator=gen)
    br = BatchRenderer(N, W, H, torch.device(DEV), max_batch=2)
    grads, losses = {}, {}
    for which in ("fused", "torch"):
        out = br.render_heads(P["mean"], P["qvec"], P["svec"], P["alpha"], P["color"], cis, [cam.c2w for cam in cams], detach_depth=False)
        rgb = out[0]
        assert rgb.shape == (2, H, W, 3)
        if which == "fused":
            img = GG.vae_input(rgb, S)
        else:
            img = (F.interpolate(rgb.permute(0, 3, 1, 2), (S, S), mode="bilinear", align_corners=False) * 2.0 - 1.0).to(torch.float16)
        latents = (img.float().flatten(1) @ enc).view(2, 4, 8, 8)
        grad = 0.5 * latents.detach() + noise  # (the UNet's stand-in: a fixed function of the latents)
        if which == "fused":
            loss = GG.sds_loss(latents, grad, 1.0)[0]
        else:
            loss = GC.sds_torch(latents, torch.nan_to_num(grad), 1.0)[0]
        loss.backward()
        losses[which] = loss.item()
        grads[which] = {k: P[k].grad.cpu().numpy().copy() for k in P if P[k].grad is not None}
        for k in P:
            P[k].grad = None
    print(f"loss fused {losses['fused']:.9e} torch {losses['torch']:.9e}")
    assert abs(losses["fused"] - losses["torch"]) <= 1e-3 * abs(losses["torch"])
    assert np.isfinite(grads["fused"]["mean"]).all() and np.abs(grads["fused"]["mean"]).max() > 0
    for k in grads["torch"]:
        assert np.isfinite(grads["fused"][k]).all(), k
        if np.abs(grads["torch"][k]).max() > 0:
            worst = rel_rows(grads["fused"][k], grads["torch"][k])
            print(f"{k}: worst row {worst:.3f} of its tolerance")
            assert worst <= 1.0, k
