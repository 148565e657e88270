"""gsgen_amd.loss's map regularisers on the MI355X against the torch restatement of tests/map_loss_cases.py, to the bound that
restatement's own fp32 error sets (no fixed tolerance), and the properties a trainer relies on: each term alone, a missing z_var,
views and offset bases, the scheduled closure on the model's dict, the loss behind the model's forward, and a captured forward +
backward whose replay sees new maps AND new weights."""
import numpy as np
import pytest
import torch

import map_loss_cases as MC
import scenes as S
from refpy_cases import rel_rows

pytestmark = pytest.mark.gpu

from gsgen_amd import loss as GL  # noqa: E402

DEV = "cuda"


def dev(a):
    return None if a is None else torch.tensor(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def run(name, weights=MC.W, scale=None, grads=("o", "v"), device_weights=False, maps=None):
    """-> (out4 [total, T_s, T_o, T_z] array, d total / d opacity or None, d total / d z_var or None): the case's arrays as [B,H,W,1]
    maps, as the model hands them over"""
    o, v = MC.inputs(name) if maps is None else maps
    o, v = dev(o)[..., None], dev(v)[..., None]
    o.requires_grad_("o" in grads)
    v.requires_grad_("v" in grads)
    if device_weights:
        total, terms = GL.map_loss_terms(o, v, weights=torch.tensor(weights, device=DEV))
    else:
        total, terms = GL.map_loss_terms(o, v if weights[2] != 0 else None, *weights)
    assert total.shape == () and total.dtype == torch.float32 and terms.shape == (3,) and not terms.requires_grad
    if grads:
        (total if scale is None else scale * total).backward()
    g = [None if t.grad is None else t.grad[..., 0].cpu().numpy() for t in (o, v)]
    return np.concatenate([total.detach().cpu().numpy()[None], terms.cpu().numpy()]), g[0], g[1]


@pytest.mark.parametrize("name", MC.NAMES)
def test_map_loss_meets_the_restatements_own_error(name):
    out, go, gv = run(name)
    MC.check_bound(name, out, go, gv)
    again = run(name)
    assert out.tobytes() == again[0].tobytes() and go.tobytes() == again[1].tobytes() and gv.tobytes() == again[2].tobytes()
    out_d, go_d, gv_d = run(name, device_weights=True)
    assert out_d.tobytes() == out.tobytes() and go_d.tobytes() == go.tobytes() and gv_d.tobytes() == gv.tobytes()


@pytest.mark.parametrize("name", ["disc-1x160x200", "half-1x160x200", "boundary-1x1x2049", "zoffset-2x5x7"])
def test_each_term_alone_and_the_unweighted_functions(name):
    out, _, _ = run(name)
    o, v = (dev(a)[..., None] for a in MC.inputs(name))
    for k, fn in enumerate((GL.sparsity_loss, GL.opague_loss, lambda a: GL.z_var_loss(v, a))):
        w1 = tuple(1.0 if j == k else 0.0 for j in range(3))
        out1, go1, gv1 = run(name, weights=w1)
        assert out1[1 + k].tobytes() == out[1 + k].tobytes() and out1[0].tobytes() == out[1 + k].tobytes()
        assert not out1[[1 + j for j in range(3) if j != k]].any()  # a masked-off term reports 0
        assert gv1 is None or k == 2
        MC.check_bound(name, out1, go1, gv1, weights=w1)
        assert bits(fn(o)).item() == bits(torch.tensor(out[1 + k])).item()
    assert bits(GL.map_loss(o, v, *MC.W)).item() == bits(torch.tensor(out[0])).item()


def test_upstream_scale():
    name = "disc-1x160x200"
    out0, go0, gv0 = run(name)
    out2, go2, gv2 = run(name, scale=2.0)
    assert out2.tobytes() == out0.tobytes()
    assert go2.tobytes() == (2.0 * go0).astype(np.float32).tobytes() and gv2.tobytes() == (2.0 * gv0).astype(np.float32).tobytes()
    out3, go3, gv3 = run(name, scale=3.0)
    MC.check_bound(name, out3, go3, gv3, scale=3.0)


@pytest.mark.parametrize("name", [n for n in MC.NAMES if n.startswith("nan_")])
def test_a_nan_pixel_reaches_its_terms_and_no_other_pixels_gradient(name):
    out, go, gv = run(name)
    if name.startswith("nan_o"):
        assert np.isnan(out).all()
    else:
        assert np.isnan(out[0]) and np.isnan(out[3]) and np.isfinite(out[1]) and np.isfinite(out[2])
    _, cgo, cgv = run(name, maps=MC.clean_of(name))
    others = np.ones(go.size, bool)
    others[MC.NAN_AT] = False
    for a, b in ((go, cgo), (gv, cgv)):
        assert a.reshape(-1)[others].tobytes() == b.reshape(-1)[others].tobytes() and np.isfinite(a.reshape(-1)[others]).all()


@pytest.mark.parametrize("name", ["boundary-2x5x7", "boundary-1x1x2049", "zeros-2x5x7", "ones-2x5x7"])
def test_the_clamp_and_the_threshold_are_decided_as_the_restatement_decides_them(name):
    o, _ = MC.inputs(name)
    inside, m = MC.masks(o)
    n = MC.BOUNDARY.size if name.startswith("boundary") else o.size
    head = lambda a: np.asarray(a).reshape(-1)[:n]  # noqa: E731
    _, go_e, _ = run(name, weights=(0.0, 1.0, 0.0), grads=("o",))
    _, go_z, gv_z = run(name, weights=(0.0, 0.0, 1.0))
    r_e, r_z = MC.reference(name, torch.float32, (0.0, 1.0, 0.0)), MC.reference(name, torch.float32, (0.0, 0.0, 1.0))
    edge = np.abs(head(o) - np.float32(0.5)) > 0.25  # (within an ulp of 0.5 the difference of the two logs may itself round to 0)
    assert ((head(go_e) != 0) == (head(r_e["go"]) != 0))[edge].all()
    assert ((head(go_z) != 0) == (head(r_z["go"]) != 0)).all() and ((head(gv_z) != 0) == (head(r_z["gv"]) != 0)).all()
    assert not head(go_e)[~head(inside)].any() and (head(go_e)[head(inside) & edge] != 0).all()
    assert ((head(gv_z) != 0) == head(m)).all() and ((head(go_z) != 0) == head(inside & m)).all()
    if name.startswith(("zeros", "ones")):
        assert not go_e.any() and not go_z.any() and (gv_z != 0).all() == name.startswith("ones")


def test_views_offset_bases_and_the_shapes():
    name = "disc-1x160x200"
    o, v = (dev(a) for a in MC.inputs(name))
    want, want_terms = GL.map_loss_terms(o[..., None], v[..., None], *MC.W)
    ro, rv = o.clone().requires_grad_(True), v.clone().requires_grad_(True)
    GL.map_loss(ro, rv, *MC.W).backward()
    assert bits(GL.map_loss(o, v, *MC.W)).item() == bits(want).item()                           # [B,H,W]
    assert bits(GL.map_loss(o[0], v[0], *MC.W)).item() == bits(want).item()                     # [H,W]
    assert bits(GL.map_loss(o[0, ..., None], v[0, ..., None], *MC.W)).item() == bits(want).item()  # [H,W,1]
    # a base 4, 8 and 12 bytes past a 16-byte boundary: no copy (the views are contiguous), the same bits
    P = o.numel()
    for k in (1, 2, 3):
        bo, bv = torch.empty(P + 4, device=DEV), torch.empty(P + 4, device=DEV)
        vo, vv = bo[k:k + P].view(o.shape), bv[k:k + P].view(v.shape)
        vo.copy_(o)
        vv.copy_(v)
        assert vo.data_ptr() % 16 == 4 * k and vo.is_contiguous()
        vo.requires_grad_(True)
        vv.requires_grad_(True)
        total, terms = GL.map_loss_terms(vo, vv, *MC.W)
        total.backward()
        assert bits(total).item() == bits(want).item() and torch.equal(bits(terms), bits(want_terms)), k
        assert torch.equal(bits(vo.grad), bits(ro.grad)) and torch.equal(bits(vv.grad), bits(rv.grad)), k
    # a transposed (non-contiguous) pair: the same pixels in another order -> the caller's layout for the gradients
    to, tv = o.transpose(1, 2).contiguous().requires_grad_(True), v.transpose(1, 2).contiguous().requires_grad_(True)
    GL.map_loss(to.transpose(1, 2), tv.transpose(1, 2), *MC.W).backward()
    assert to.grad.shape == to.shape and torch.equal(bits(to.grad.transpose(1, 2)), bits(ro.grad))
    assert torch.equal(bits(tv.grad.transpose(1, 2)), bits(rv.grad))
    # a strided crop
    crop = (slice(None), slice(3, 140), slice(5, 158))
    fo, fv = o.clone().requires_grad_(True), v.clone().requires_grad_(True)
    La = GL.map_loss(fo[crop][..., None], fv[crop][..., None], *MC.W)
    La.backward()
    co, cv = o[crop].contiguous().requires_grad_(True), v[crop].contiguous().requires_grad_(True)
    Lb = GL.map_loss(co, cv, *MC.W)
    Lb.backward()
    assert bits(La).item() == bits(Lb).item() and torch.equal(bits(fo.grad[crop]), bits(co.grad)) and torch.equal(bits(fv.grad[crop]), bits(cv.grad))
    outside = fo.grad.clone()
    outside[crop] = 0
    assert not outside.any()


def test_without_z_var():
    name = "disc-1x160x200"
    out, go, _ = run(name, weights=(0.5, 0.25, 0.0))
    o = dev(MC.inputs(name)[0])[..., None].requires_grad_(True)
    total, terms = GL.map_loss_terms(o, None, 0.5, 0.25)
    total.backward()
    assert bits(total).item() == bits(torch.tensor(out[0])).item() and float(terms[2]) == 0.0
    assert o.grad[..., 0].cpu().numpy().tobytes() == go.tobytes()
    # device weights without z_var: the two opacity terms, whatever the third weight holds
    total_d, terms_d = GL.map_loss_terms(o.detach(), None, weights=torch.tensor([0.5, 0.25, 9.0], device=DEV))
    assert bits(total_d).item() == bits(total).item() and torch.equal(bits(terms_d), bits(terms))
    with pytest.raises(ValueError, match="should turn off the `rgb_only` flag"):
        GL.map_loss(o, None, 0.5, 0.25, 1.0)
    # only z_var requires a gradient
    v = dev(MC.inputs(name)[1])[..., None].requires_grad_(True)
    GL.map_loss(o.detach(), v, *MC.W).backward()
    assert v.grad is not None and float(v.grad.abs().max()) > 0


def test_get_map_loss_on_the_models_dict_at_two_steps_of_a_schedule():
    name = "disc-1x160x200"
    o, v = (dev(a)[..., None] for a in MC.inputs(name))
    cfg = {"sparsity": [100, 1.0, 0.1, 200], "opague": 0.25, "z_var": [0, 0.0, 4.0, 1000]}  # piecewise: (s0, v0, v1, s1)
    fn = GL.get_map_loss(cfg, max_steps=1000)
    for step, w in ((50, (1.0, 0.25, 0.2)), (150, (0.55, 0.25, 0.6))):
        out = {"rgb": torch.zeros(1, 160, 200, 3, device=DEV), "depth": torch.zeros_like(o), "opacity": o.clone().requires_grad_(True),
               "z_var": v.clone().requires_grad_(True)}
        loss, logs = fn(out, step)
        assert loss.shape == () and loss.is_cuda and set(logs) == {"sparsity", "opague", "z_var"}
        assert all(t.shape == () and t.is_cuda and not t.requires_grad for t in logs.values())
        loss.backward()
        want, wo, wv = run(name, weights=w)
        got = np.array([float(loss.detach()), float(logs["sparsity"]), float(logs["opague"]), float(logs["z_var"])], np.float32)
        MC.check_bound(name, got, out["opacity"].grad[..., 0].cpu().numpy(), out["z_var"].grad[..., 0].cpu().numpy(), weights=w)
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()  # (the schedule's value is a double: not the same bits as w)
    # z_var switched off at step 0 (weight 0): the term is not evaluated and reports 0
    loss, logs = fn({"opacity": o, "z_var": v}, 0)
    assert float(logs["z_var"]) == 0.0 and float(logs["sparsity"]) > 0


def small_model():
    from gsgen_amd.model import GaussianSplattingRenderer
    from gsgen_amd.renderer import CameraInfo
    cfg = dict(device=DEV, svec_act="exp", alpha_act="sigmoid", color_act="sigmoid", tile_size=16, T_thresh=1e-4, depth_detach=True,
               background=dict(type="fixed", color=[0.1, 0.2, 0.3]), densify=dict(enabled=False), prune=dict(enabled=False))
    sc = S.pointe_scene(2000, seed=3, svec=0.03, C=1)
    init = {k: torch.tensor(sc[k], device=DEV) for k in ("mean", "qvec", "svec", "color", "alpha")}
    cams = [S.Camera(64, 64, fx=70.0, c2w=S.orbit(3.0, 20.0, 30.0 + 90.0 * i)) for i in range(2)]
    m = GaussianSplattingRenderer(cfg, init)
    return m, {"c2w": torch.stack([torch.tensor(c.c2w) for c in cams]), "camera_info": [CameraInfo(*c.intr) for c in cams]}


def test_map_loss_behind_the_models_forward():
    """model forward at 64 x 64, B = 2 -> get_map_loss -> backward: the parameter gradients against the fp32 torch composition on the
    same `out`, at the suite's per-Gaussian rtol"""
    m, batch = small_model()
    out = m(batch)
    assert out["opacity"].shape == (2, 64, 64, 1) and out["z_var"].shape == (2, 64, 64, 1)
    assert int((out["opacity"] > 0.5).sum()) > 20  # (the z_var term sees pixels)
    w = (1.0, 0.5, 3.0)
    params = [p for p in m.parameters() if p.requires_grad]
    loss, logs = GL.get_map_loss({"sparsity": w[0], "opague": w[1], "z_var": w[2]})(out, 10)
    g_fused = torch.autograd.grad(loss, params, retain_graph=True, allow_unused=True)
    s, e, z = MC.map_loss_torch(out["opacity"], out["z_var"])
    g_torch = torch.autograd.grad(w[0] * s.mean() + w[1] * e.mean() + w[2] * z.mean(), params, retain_graph=True, allow_unused=True)
    seen, largest = 0, max(float(b.abs().max()) for b in g_torch if b is not None)
    for p, a, b in zip(params, g_fused, g_torch):
        assert (a is None) == (b is None)
        if b is None or float(b.abs().max()) <= 1e-9 * largest:
            continue  # (the scene's Gaussians are isotropic: the gradient to their rotations is 0, and what arrives is rounding noise)
        assert torch.isfinite(a).all()
        assert rel_rows(a.cpu().numpy(), b.cpu().numpy()) <= 1.0, tuple(p.shape)
        seen += 1
    assert seen >= 3 and any(p is m.mean and b is not None for p, b in zip(params, g_torch))
    loss.backward()  # the closure's own call form
    assert m.mean.grad is not None and float(m.mean.grad.abs().max()) > 0


def test_forward_and_backward_replay_in_a_captured_graph_on_new_maps_and_new_weights():
    name = "disc-1x32x64"
    o0, v0 = MC.inputs(name)
    others = [MC.make_maps(values, 1, 32, 64, 900 + k) + (w,) for k, (values, w) in
              enumerate((("uniform", (0.1, 0.2, 0.3)), ("half", (1.0, 0.0, 2.0)), ("boundary", (0.25, 3.0, 0.5))))]
    o, v = dev(o0).requires_grad_(True), dev(v0).requires_grad_(True)
    weights = torch.tensor(MC.W, device=DEV)
    scale = torch.tensor(1.0, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        (GL.map_loss(o, v, weights=weights) * scale).backward()  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    o.grad = v.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # (one stream: nothing in the capture forks)
        total, terms = GL.map_loss_terms(o, v, weights=weights)
        (total * scale).backward()
    for k, (o_new, v_new, w_new) in enumerate(others):
        with torch.no_grad():
            o.copy_(dev(o_new))
            v.copy_(dev(v_new))
            weights.copy_(torch.tensor(w_new))
            scale.fill_(1.0 + k)  # (the upstream scalar is read on the device: a replay sees the new one)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in (total, terms, o.grad, v.grad)]
        eo, ev = dev(o_new).requires_grad_(True), dev(v_new).requires_grad_(True)
        te, pe = GL.map_loss_terms(eo, ev, weights=torch.tensor(w_new, device=DEV))
        (te * (1.0 + k)).backward()
        for a, b in zip(got, (te, pe, eo.grad, ev.grad)):
            assert torch.equal(bits(a), bits(b)), k
        assert got[2].abs().max() > 0, k
