"""gsgen_amd.loss on the MI355X against the torch restatement of tests/loss_cases.py, to the bound that restatement's own fp32
error sets (no fixed tolerance), and the properties a trainer relies on: the reference's call forms, the upstream scale, bit
equality from run to run, a captured forward + backward, and the loss behind a BatchRenderer render."""
import types

import numpy as np
import pytest
import torch

import loss_cases as LC
import scenes
from refpy_cases import rel_rows

pytestmark = pytest.mark.gpu

from gsgen_amd import loss as GL  # noqa: E402

DEV = "cuda"


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def run(out, gt, w, base, ws, scale=None):
    """-> (loss as a Python float, d loss / d out as a float32 array)"""
    o = dev(out).requires_grad_(True)
    L = GL.image_loss(o, dev(gt), w, base, ws)
    assert L.shape == () and L.dtype == torch.float32 and L.requires_grad
    (L if scale is None else scale * L).backward()
    return float(L.item()), o.grad.cpu().numpy()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize("name", LC.NAMES)
def test_image_loss_meets_the_restatements_own_error(name):
    c = LC.case(name)
    L, g = run(c["out"], c["gt"], c["w"], c["base"], c["ws"])
    if c["kind"] == "same":
        LC.check_same(name, L, g)
    else:
        LC.check_bound(name, L, g)


def test_ssim_loss_terms_three_dimensional_and_non_contiguous_inputs():
    c = LC.case("smooth-2x37x53x3-ws11-l1")
    out, gt = dev(c["out"]), dev(c["gt"])
    total, ssim, base = GL.image_loss_terms(out, gt, 0.2, "l1", 11)
    assert not ssim.requires_grad and not base.requires_grad and not total.requires_grad  # (out does not ask for a gradient)
    o64, g64 = torch.as_tensor(c["out"]).double(), torch.as_tensor(c["gt"]).double()
    want_ssim, want_base = float(LC.image_loss_torch(o64, g64, 1.0, "l1", 11)), float((o64 - g64).abs().mean())
    ssim32 = float(LC.image_loss_torch(torch.as_tensor(c["out"]), torch.as_tensor(c["gt"]), 1.0, "l1", 11))
    tol = 4 * max(abs(ssim32 - want_ssim), 2.0 ** -22 * want_ssim)  # (the bound of loss_cases.check_bound, for the term alone)
    assert abs(float(ssim) - want_ssim) <= tol and abs(float(base) - want_base) <= 2.0 ** -22 * want_base
    assert abs(float(GL.ssim_loss(out, gt, 11)) - want_ssim) <= tol
    assert float(total) == float(GL.image_loss(out, gt, 0.2, "l1", 11))
    # [H, W, C] is a batch of one
    assert bits(GL.image_loss(out[0], gt[0], 0.2, "l1", 11)).item() == bits(GL.image_loss(out[:1], gt[:1], 0.2, "l1", 11)).item()
    # a channels-first tensor viewed channels last, and a strided crop: made contiguous, the gradient arrives in the caller's layout
    chw = out.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    La = GL.image_loss(chw.permute(0, 2, 3, 1)[:, 3:30, 5:45], gt[:, 3:30, 5:45], 0.2, "l2", 7)
    La.backward()
    ref = out[:, 3:30, 5:45].contiguous().requires_grad_(True)
    Lb = GL.image_loss(ref, gt[:, 3:30, 5:45].contiguous(), 0.2, "l2", 7)
    Lb.backward()
    assert bits(La).item() == bits(Lb).item()
    assert torch.equal(bits(chw.grad.permute(0, 2, 3, 1)[:, 3:30, 5:45]), bits(ref.grad))
    outside = chw.grad.permute(0, 2, 3, 1).clone()
    outside[:, 3:30, 5:45] = 0
    assert not outside.any()  # (zero outside the crop)


def test_the_references_call_forms():
    """get_image_loss on [B,H,W,3] and get_loss_fn on [H,W,3] against the restatement called the way utils/loss.py calls kornia"""
    c = LC.case("noise-2x37x53x3-ws11-l2")
    for kind in ("l1", "l2"):
        o = dev(c["out"]).requires_grad_(True)
        GL.get_image_loss(0.3, kind)(o, dev(c["gt"])).backward()
        o64 = torch.as_tensor(c["out"]).double().requires_grad_(True)
        L64 = LC.image_loss_torch(o64, torch.as_tensor(c["gt"]).double(), 0.3, kind, 11)
        L64.backward()
        o32 = torch.as_tensor(c["out"]).requires_grad_(True)
        LC.image_loss_torch(o32, torch.as_tensor(c["gt"]), 0.3, kind, 11).backward()
        e32 = (o32.grad.double() - o64.grad).abs().max().item()
        err = (o.grad.cpu().double() - o64.grad).abs().max().item()
        assert err <= 4 * max(e32, 2.0 ** -22 * o64.grad.abs().max().item()), (kind, err, e32)
    cfg = types.SimpleNamespace(loss_fn="l1", ssim_loss_mult=0.25, ssim_loss_win_size=7)
    o = dev(c["out"][1]).requires_grad_(True)
    L = GL.get_loss_fn(cfg)(o, dev(c["gt"][1]))
    L.backward()
    o64 = torch.as_tensor(c["out"][1]).double().requires_grad_(True)
    L64 = LC.image_loss_torch(o64[None], torch.as_tensor(c["gt"][1]).double()[None], 0.25, "l1", 7)
    L64.backward()
    o32 = torch.as_tensor(c["out"][1]).requires_grad_(True)
    L32 = LC.image_loss_torch(o32[None], torch.as_tensor(c["gt"][1])[None], 0.25, "l1", 7)
    L32.backward()
    e32 = (o32.grad.double() - o64.grad).abs().max().item()
    assert (o.grad.cpu().double() - o64.grad).abs().max().item() <= 4 * max(e32, 2.0 ** -22 * o64.grad.abs().max().item())
    assert abs(float(L) - float(L64)) <= 4 * max(abs(float(L32) - float(L64)), 2.0 ** -22 * float(L64))


def test_upstream_scale_and_run_to_run_bit_equality():
    c = LC.case("noise-2x37x53x3-ws11-l2")
    L0, g0 = run(c["out"], c["gt"], 0.2, "l2", 11)
    L1, g1 = run(c["out"], c["gt"], 0.2, "l2", 11)
    assert L0 == L1 and g0.tobytes() == g1.tobytes()
    _, g3 = run(c["out"], c["gt"], 0.2, "l2", 11, scale=3.0)
    assert (np.abs(g3 - 3.0 * g0) <= np.spacing(np.abs(3.0 * g0))).all()  # one ulp, entry by entry
    assert np.abs(g0).max() > 0
    # no gradient wanted: the forward alone gives the same loss bit for bit
    with torch.no_grad():
        Ln = GL.image_loss(dev(c["out"]), dev(c["gt"]), 0.2, "l2", 11)
    assert float(Ln) == L0 and not Ln.requires_grad


def test_forward_and_backward_replay_in_a_captured_graph():
    c = LC.case("noise-2x37x53x3-ws11-l2")
    other = [LC.make_images("smooth", 2, 37, 53, 3, seed) for seed in (11, 12)]
    out, gt = dev(c["out"]).requires_grad_(True), dev(c["gt"])
    scale = torch.tensor(1.0, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        (GL.image_loss(out, gt, 0.2, "l1", 11) * scale).backward()  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    out.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L = GL.image_loss(out, gt, 0.2, "l1", 11)
        (L * scale).backward()
    for k, (o_new, g_new) in enumerate(other):
        with torch.no_grad():
            out.copy_(dev(o_new))
            gt.copy_(dev(g_new))
            scale.fill_(1.0 + k)  # (the upstream scalar is read on the device: a replay sees the new one)
        graph.replay()
        torch.cuda.synchronize()
        got_L, got_g = L.clone(), out.grad.clone()
        eager = dev(o_new).requires_grad_(True)
        Le = GL.image_loss(eager, dev(g_new), 0.2, "l1", 11)
        (Le * (1.0 + k)).backward()
        assert bits(got_L).item() == bits(Le).item(), k
        assert torch.equal(bits(got_g), bits(eager.grad)), k


def test_image_loss_behind_a_batch_render():
    """BatchRenderer RGB render at 64 x 48 -> image_loss -> backward: the parameter gradients against the same render followed by
    the fp32 torch restatement on the device"""
    from gsgen_amd import renderer as R
    from gsgen_amd.batch import BatchRenderer
    sc = scenes.random_scene(1500, seed=5, svec=0.05, C=2)
    N, W, H = sc["mean"].shape[0], 64, 48
    cams = [scenes.Camera(W, H, fx=60.0, c2w=scenes.orbit(2.4, 10 + 5 * i, 70.0 * i)) for i in range(2)]
    cis = [R.CameraInfo(*cam.intr) for cam in cams]
    names = ("mean", "qvec", "svec", "alpha")
    P = {k: dev(sc[k]).requires_grad_(True) for k in names}
    P["col"] = torch.sigmoid(dev(sc["sh"][:, :, 0])).requires_grad_(True)
    gt = torch.rand(2, H, W, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    br = BatchRenderer(N, W, H, torch.device(DEV), max_batch=2)
    grads = {}
    for which, fn in (("fused", lambda o: GL.image_loss(o, gt, 0.2, "l2", 11)), ("torch", lambda o: LC.image_loss_torch(o, gt, 0.2, "l2", 11))):
        rgb, _ = br.render(P["mean"], P["qvec"], P["svec"], P["alpha"], P["col"], cis, [cam.c2w for cam in cams], C=0)
        assert rgb.shape == (2, H, W, 3)
        fn(rgb).backward()
        grads[which] = {k: P[k].grad.cpu().numpy().copy() for k in P}
        for k in P:
            P[k].grad = None
    for k in P:
        assert np.abs(grads["torch"][k]).max() > 0, k
        assert rel_rows(grads["fused"][k], grads["torch"][k]) <= 1.0, k
