"""gsgen_amd.loss's Pearson depth loss on the MI355X against the torch restatement of tests/depth_loss_cases.py, to the bound that
restatement's own fp32 error sets (no fixed tolerance), and the properties a trainer relies on: gradients to either depth map, the
reference's call form, broadcast gt and mask, the upstream scale, bit equality from run to run, a captured forward + backward whose
replay sees new depths AND a new mask, and the loss behind a BatchRenderer heads render."""
import numpy as np
import pytest
import torch

import depth_loss_cases as DC
import scenes
from refpy_cases import rel_rows

pytestmark = pytest.mark.gpu

from gsgen_amd import loss as GL  # noqa: E402

DEV = "cuda"


def dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def run(name, grads=("pred", "gt"), scale=None, fn=None):
    """-> (loss as a Python float, corr [B] array, d loss / d pred or None, d loss / d gt or None): the case's arrays as [B,H,W,1]
    depth maps (gt [1,H,W,1] when shared) and a [B,H,W] / [1,H,W] bool mask, as the trainer holds them"""
    c = DC.case(name)
    pred, gt, mask = dev(c["pred"])[..., None], dev(c["gt"])[..., None], dev(c["mask"])
    pred.requires_grad_("pred" in grads)
    gt.requires_grad_("gt" in grads)
    if fn is None:
        L, corr = GL.pearson_depth_loss_terms(pred, gt, mask)
        assert corr.shape == (pred.shape[0],) and not corr.requires_grad and corr.dtype == torch.float32
    else:
        L, corr = fn(pred, gt, mask), None
    assert L.shape == () and L.dtype == torch.float32 and L.requires_grad == bool(grads)
    if grads:
        (L if scale is None else scale * L).backward()
    g = [None if t.grad is None else t.grad[..., 0].cpu().numpy() for t in (pred, gt)]
    return float(L.item()), None if corr is None else corr.cpu().numpy(), g[0], g[1]


@pytest.mark.parametrize("name", DC.NAMES)
def test_depth_loss_meets_the_restatements_own_error(name):
    L, corr, gp, gg = run(name)
    DC.check_bound(name, L, gp, gg)
    DC.check_corr(name, corr)
    c = DC.case(name)
    dead = np.isnan(c["c64"])
    assert not gp[dead].any()  # a degenerate image: exact zeros
    if c["mask"] is not None:
        assert not gp[~np.broadcast_to(c["mask"], gp.shape)].any()


def test_gradients_to_pred_only_to_gt_only_and_to_both():
    """trainer.py:432 calls depth_loss(pearson, estimated, rendered): the rendered depth is the SECOND argument there"""
    for name in ("offset100-3x64x64-rand70", "affine-1x160x200-two", "nans-3x64x64-none-sharedgt"):
        L, _, gp, gg = run(name)
        Lp, _, gp1, none = run(name, grads=("pred",))
        assert none is None and Lp == L and gp1.tobytes() == gp.tobytes()
        Lg, _, none, gg1 = run(name, grads=("gt",))
        assert none is None and Lg == L and gg1.tobytes() == gg.tobytes()
        DC.check_bound(name, Lg, None, gg1)
        Ln, _, a, b = run(name, grads=())
        assert Ln == L and a is None and b is None


def test_upstream_scale_and_run_to_run_bit_equality():
    name = "offset100-3x64x64-rand70"
    L0, c0, p0, g0 = run(name)
    L1, c1, p1, g1 = run(name)
    assert L0 == L1 and c0.tobytes() == c1.tobytes() and p0.tobytes() == p1.tobytes() and g0.tobytes() == g1.tobytes()
    assert np.abs(p0).max() > 0 and np.abs(g0).max() > 0
    L3, _, p3, g3 = run(name, scale=3.0)
    assert L3 == L0
    DC.check_bound(name, L3, p3, g3, scale=3.0)
    _, _, p2, g2 = run(name, scale=2.0)
    assert p2.tobytes() == (2.0 * p0).astype(np.float32).tobytes() and g2.tobytes() == (2.0 * g0).astype(np.float32).tobytes()


def test_the_references_call_form_and_the_package_names():
    import gsgen_amd
    name = "affine-2x37x53-rand70"
    L, _, gp, gg = run(name)
    for fn in (lambda p, g, m: GL.depth_loss(None, p, g, m), lambda p, g, m: gsgen_amd.depth_loss(object(), p, g, m),
               lambda p, g, m: GL.pearson_depth_loss(p, g, m)):
        L1, _, gp1, gg1 = run(name, fn=fn)
        assert L1 == L and gp1.tobytes() == gp.tobytes() and gg1.tobytes() == gg.tobytes()
    # without a mask: the reference's ones_like(depth_gt[..., 0])
    c = DC.case(name)
    pred, gt = dev(c["pred"])[..., None], dev(c["gt"])[..., None]
    ones = torch.ones_like(gt[..., 0], dtype=torch.bool)
    assert bits(GL.depth_loss(None, pred, gt)).item() == bits(GL.depth_loss(None, pred, gt, ones)).item()
    assert bits(GL.depth_loss(None, pred, gt, ones.to(torch.uint8))).item() == bits(GL.depth_loss(None, pred, gt)).item()


def test_shapes_a_batch_of_one_and_broadcast_by_stride():
    c = DC.case("affine-3x64x64-rand70")
    pred, gt, mask = dev(c["pred"]), dev(c["gt"]), dev(c["mask"])
    want = GL.pearson_depth_loss(pred[..., None], gt[..., None], mask)
    assert bits(GL.pearson_depth_loss(pred, gt, mask)).item() == bits(want).item()              # [B,H,W]
    one = GL.pearson_depth_loss(pred[:1], gt[:1], mask[:1])
    assert bits(GL.pearson_depth_loss(pred[0, ..., None], gt[0, ..., None], mask[0])).item() == bits(one).item()   # [H,W,1]
    assert bits(GL.pearson_depth_loss(pred[0], gt[0], mask[0])).item() == bits(one).item()      # [H,W]
    assert bits(GL.pearson_depth_loss(pred[0], gt[:1, ..., None], mask[:1])).item() == bits(one).item()
    # one gt and one mask for the batch ([1,H,W,1], [H,W,1], [H,W] / [1,H,W], [H,W]) = their materialised repeats, bit for bit
    rep_gt, rep_m = gt[1:2].expand(3, -1, -1).contiguous(), mask[2:3].expand(3, -1, -1).contiguous()
    p_rep = pred.clone().requires_grad_(True)
    L_rep, corr_rep = GL.pearson_depth_loss_terms(p_rep, rep_gt, rep_m)
    L_rep.backward()
    for g_in, m_in in ((gt[1:2, ..., None], mask[2:3]), (gt[1, ..., None], mask[2]), (gt[1], mask[2:3])):
        p = pred.clone().requires_grad_(True)
        L, corr = GL.pearson_depth_loss_terms(p, g_in, m_in)
        L.backward()
        assert bits(L).item() == bits(L_rep).item() and torch.equal(bits(corr), bits(corr_rep)) and torch.equal(bits(p.grad), bits(p_rep.grad))
    # a broadcast gt that requires a gradient: expanded, and autograd sums the batch's gradients onto the one image
    g_rep = rep_gt.clone().requires_grad_(True)
    GL.pearson_depth_loss(pred, g_rep, rep_m).backward()
    g_one = gt[1:2].clone().requires_grad_(True)
    L = GL.pearson_depth_loss(pred, g_one, mask[2])
    L.backward()
    assert bits(L).item() == bits(L_rep).item() and g_one.grad.shape == g_one.shape
    assert torch.equal(bits(g_one.grad), bits(g_rep.grad.sum(0, keepdim=True)))


def test_a_strided_crop_takes_its_gradient_in_the_callers_layout():
    c = DC.case("offset100-3x64x64-rand70")
    full_p, full_g, mask = dev(c["pred"]).requires_grad_(True), dev(c["gt"]).requires_grad_(True), dev(c["mask"])
    crop = (slice(None), slice(3, 40), slice(5, 58))
    La = GL.pearson_depth_loss(full_p[crop][..., None], full_g[crop][..., None], mask[crop])
    La.backward()
    ref_p, ref_g = full_p.detach()[crop].contiguous().requires_grad_(True), full_g.detach()[crop].contiguous().requires_grad_(True)
    Lb = GL.pearson_depth_loss(ref_p, ref_g, mask[crop].contiguous())
    Lb.backward()
    assert bits(La).item() == bits(Lb).item()
    for full, ref in ((full_p, ref_p), (full_g, ref_g)):
        assert torch.equal(bits(full.grad[crop]), bits(ref.grad)) and ref.grad.abs().max() > 0
        outside = full.grad.clone()
        outside[crop] = 0
        assert not outside.any()  # (zero outside the crop)
    # a transposed view and a transposed mask
    pt = dev(c["pred"]).transpose(1, 2).contiguous().requires_grad_(True)
    Lt = GL.pearson_depth_loss(pt.transpose(1, 2), dev(c["gt"]), mask.transpose(1, 2).contiguous().transpose(1, 2))
    Lt.backward()
    Lf = GL.pearson_depth_loss(full_p.detach().requires_grad_(False), dev(c["gt"]), mask)
    assert bits(Lt).item() == bits(Lf).item() and pt.grad.shape == pt.shape


def test_forward_and_backward_replay_in_a_captured_graph_on_new_depths_and_a_new_mask():
    B, H, W = 2, 37, 53
    c = DC.case("affine-2x37x53-rand70")
    others = []
    for k, (values, mkind) in enumerate((("offset100", "rand70"), ("nans", "onefalse"), ("anti", "two"))):
        p, g = DC.make_depths(values, B, H, W, 900 + k)
        others.append((p, g, DC.make_mask(mkind, B, H, W, 900 + k)))
    pred, gt, mask = dev(c["pred"]).requires_grad_(True), dev(c["gt"]).requires_grad_(True), dev(c["mask"])
    scale = torch.tensor(1.0, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        (GL.pearson_depth_loss(pred, gt, mask) * scale).backward()  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    pred.grad = gt.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L, corr = GL.pearson_depth_loss_terms(pred, gt, mask)
        (L * scale).backward()
    for k, (p_new, g_new, m_new) in enumerate(others):
        with torch.no_grad():
            pred.copy_(dev(p_new))
            gt.copy_(dev(g_new))
            mask.copy_(dev(m_new))
            scale.fill_(1.0 + k)  # (the upstream scalar is read on the device: a replay sees the new one)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in (L, corr, pred.grad, gt.grad)]
        ep, eg = dev(p_new).requires_grad_(True), dev(g_new).requires_grad_(True)
        Le, ce = GL.pearson_depth_loss_terms(ep, eg, dev(m_new))
        (Le * (1.0 + k)).backward()
        for a, b in zip(got, (Le, ce, ep.grad, eg.grad)):
            assert torch.equal(bits(a), bits(b)), k
        assert got[2].abs().max() > 0, k


def test_depth_loss_behind_a_batch_heads_render():
    """BatchRenderer heads render at 64 x 48 -> depth_loss on out["depth"] under the opacity mask -> backward: the parameter gradients
    against the same render followed by the fp32 torch restatement on the device; they reach the means and are finite"""
    from gsgen_amd import renderer as R
    from gsgen_amd.batch import BatchRenderer
    sc = scenes.random_scene(1500, seed=5, svec=0.05)
    N, W, H = sc["mean"].shape[0], 64, 48
    cams = [scenes.Camera(W, H, fx=60.0, c2w=scenes.orbit(2.4, 10 + 5 * i, 70.0 * i)) for i in range(2)]
    cis = [R.CameraInfo(*cam.intr) for cam in cams]
    names = ("mean", "qvec", "svec", "alpha", "color")
    P = {k: dev(sc[k]).requires_grad_(True) for k in names}
    gen = torch.Generator(DEV).manual_seed(1)
    yy, xx = torch.meshgrid(torch.linspace(0, 3, H, device=DEV), torch.linspace(0, 3, W, device=DEV), indexing="ij")
    gt = (2.0 + torch.sin(2 * xx + yy)[None] + 0.3 * torch.rand(1, H, W, device=DEV, generator=gen))[..., None]  # one map for both views
    br = BatchRenderer(N, W, H, torch.device(DEV), max_batch=2)
    grads = {}
    for which in ("fused", "torch"):
        out = br.render_heads(P["mean"], P["qvec"], P["svec"], P["alpha"], P["color"], cis, [cam.c2w for cam in cams], detach_depth=False)
        depth, opacity = out[1], out[2]
        assert depth.shape == (2, H, W, 1)
        mask = opacity.detach()[..., 0] > opacity.detach().median()  # (about the better-covered half of the pixels)
        assert int(mask[0].sum()) > 50 and int(mask[1].sum()) > 50
        if which == "fused":
            L = GL.depth_loss(None, depth, gt, mask)
        else:
            L = DC.depth_loss_torch(torch.nan_to_num(depth[..., 0]), gt[..., 0], mask)[0]
        L.backward()
        grads[which] = {k: P[k].grad.cpu().numpy().copy() for k in P if P[k].grad is not None}
        for k in P:
            P[k].grad = None
    assert np.isfinite(grads["fused"]["mean"]).all() and np.abs(grads["fused"]["mean"]).max() > 0
    for k in grads["torch"]:
        assert np.isfinite(grads["fused"][k]).all(), k
        if np.abs(grads["torch"][k]).max() > 0:
            assert rel_rows(grads["fused"][k], grads["torch"][k]) <= 1.0, k
