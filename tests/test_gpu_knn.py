"""The kNN kernel (gsgen_amd/csrc/knn.hip) on the MI355X: exact against a torch brute force on bench's cfg2 cloud and a 1 %-outlier
variant, deterministic, capturable; the model features built on it against the reference's own results (tests/golden/knn)."""
import numpy as np
import pytest
import torch

import knn_cases as KC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def brute(pts, K, chunk=2048):
    """the kernel's formula and tie rule in torch: dx*dx + dy*dy + dz*dz (d = p_j - p_i), then topk on (float bits << 32 | j)"""
    N = pts.shape[0]
    out_d, out_i = [], []
    j = torch.arange(N, device=pts.device, dtype=torch.int64)
    for a in range(0, N, chunk):
        q = pts[a:a + chunk]
        dx = pts[None, :, 0] - q[:, None, 0]
        dy = pts[None, :, 1] - q[:, None, 1]
        dz = pts[None, :, 2] - q[:, None, 2]
        d2 = dx * dx
        d2 = d2 + dy * dy
        d2 = d2 + dz * dz
        key = (d2.view(torch.int32).to(torch.int64) << 32) | j[None, :]
        k = torch.topk(key, K, dim=1, largest=False, sorted=True).values
        out_d.append((k >> 32).to(torch.int32).view(torch.float32))
        out_i.append(k & 0xFFFFFFFF)
    return torch.cat(out_d), torch.cat(out_i)


def cfg2_cloud(outliers=False):
    import bench
    sc, _, _ = bench.make_workload("cfg2")
    p = torch.tensor(sc["mean"], device=DEV, dtype=torch.float32)
    if outliers:
        p = with_outliers(p)
    return p


def with_outliers(p, frac=0.01, seed=0):
    """frac of the points moved to 100x the cloud's radius (random directions)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    c = p.mean(0)
    r = float((p - c).norm(dim=1).max())
    n = int(p.shape[0] * frac)
    sel = torch.randperm(p.shape[0], generator=g)[:n].to(p.device)
    d = torch.randn(n, 3, generator=g).to(p.device)
    q = p.clone()
    q[sel] = c + 100.0 * r * d / d.norm(dim=1, keepdim=True)
    return q


@pytest.mark.parametrize("outliers", [False, True])
def test_knn_is_the_brute_force_on_cfg2(outliers):
    from gsgen_amd.knn import knn_raw
    p = cfg2_cloud(outliers)
    bd, bi = brute(p, 32)
    for K in (1, 2, 4, 8, 32):
        d, i = knn_raw(p, K)
        torch.cuda.synchronize()
        assert torch.equal(i.long(), bi[:, :K]), (K, int((i.long() != bi[:, :K]).sum()))
        assert torch.equal(d.view(torch.int32), bd[:, :K].contiguous().view(torch.int32)), K


def test_knn_nan_rows_and_duplicates():
    from gsgen_amd.knn import knn_points
    g = torch.Generator(device="cpu").manual_seed(1)
    p = torch.rand(5000, 3, generator=g)
    p[1000:1100] = p[:100]
    p[7, 1] = float("nan")
    p[9] = float("inf")
    p = p.to(DEV)
    d, i = knn_points(p, 4)
    fin = torch.isfinite(p).all(1)
    q = p.clone()
    q[~fin] = 1e30  # (the brute force: far away instead of non-finite)
    bd, bi = brute(q, 4)
    assert torch.equal(i[fin], bi[fin]) and torch.equal(d[fin], bd[fin])
    assert (i[~fin] == -1).all() and torch.isinf(d[~fin]).all()
    first = torch.arange(100, device=DEV)
    ok = fin[:100] & fin[1000:1100]  # (rows 7 and 9 were made non-finite after the copy)
    assert (i[1000:1100, 0] == first)[ok].all()  # a lower-index duplicate comes before self


def test_knn_is_deterministic():
    from gsgen_amd.knn import knn_raw
    p = cfg2_cloud(True)
    a = knn_raw(p, 8)
    b = knn_raw(p, 8)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_knn_points_replays_in_a_captured_graph():
    from gsgen_amd.knn import knn_points
    p = cfg2_cloud()
    static = p.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        knn_points(static, 4)  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gd, gi = knn_points(static, 4)
    static.copy_(with_outliers(p, 0.05, seed=3) * 0.5)
    graph.replay()
    ed, ei = knn_points(static, 4)
    torch.cuda.synchronize()
    assert torch.equal(gi, ei) and torch.equal(gd.view(torch.int32), ed.view(torch.int32))


def test_nearest_neighbor_initialize_and_K_nearest_neighbors():
    from gsgen_amd import knn as KNN
    p = cfg2_cloud()[:20000]
    bd, bi = brute(p, 4)
    init = KNN.nearest_neighbor_initialize(p, k=3)
    assert init.device.type == "cpu"  # (as the reference returns it)
    torch.testing.assert_close(init, bd[:, 1:].mean(1).cpu())
    nn, idx, dist = KNN.K_nearest_neighbors(p, 4, return_dist=True)
    assert torch.equal(idx, bi[:, 1:]) and torch.equal(nn, p[bi[:, 1:]])
    pos, i1 = KNN.nearest_neighbor(p)
    assert torch.equal(i1, bi[:, 1]) and torch.equal(pos, p[bi[:, 1]])
    assert torch.equal(KNN.nearest_neighbor_initialize(p.cpu().numpy(), k=3), init)


def test_model_densify_by_compatness_matches_the_reference_golden():
    z = KC.load("densify_compat")
    m = KC.model_with_adam(z, DEV)
    assert m.densify_by_compatness(3) == int(z["n_new"])
    KC.check_after(m, z, bitwise=False)


def test_model_densify_shrink_then_densify_config_matches_the_reference_golden():
    """densify(step) with a conf/shrink_then_densify.yaml-shaped node (use_legacy, type shrink_then_compatness), the legacy step
    selecting nothing: the shrink-then-compatness rows of the reference, statistics reset"""
    z0, z = KC.load("densify_compat"), KC.load("densify_shrink")
    dcfg = dict(enabled=True, type="shrink_then_compatness", use_legacy=True, warm_up=0, end=100, period=10, mean2d_thresh=1e9,
                split_thresh=0.02, surface_shrink=1.5, K=3)
    m = KC.model_with_adam(z0, DEV, densify=dcfg)
    m.train()
    m.reset_densify_info()
    m.densify(10, verbose=False)
    # (the legacy step restarts the optimiser, as the reference's densify_legacy does: compare the fields, then the state the new
    # optimiser holds is empty)
    for k in KC.FIELDS:
        np.testing.assert_allclose(getattr(m, KC.ATTR[k]).detach().cpu().numpy(), z["after_" + k], rtol=2e-5, atol=2e-6, err_msg=k)
    assert m.mean_2d_grad_accum.shape[0] == m.N and float(m.mean_2d_grad_accum.abs().sum()) == 0.0


@pytest.mark.parametrize("name", list(KC.PENALTIES))
def test_model_penalties_match_the_reference_golden(name):
    z = KC.load("penalties")
    m = KC.model_from_raw({k: z["raw_" + k] for k in KC.FIELDS}, DEV, penalty=KC.PENALTIES[name])
    loss = m.auxiliary_loss(int(z["step"]))
    loss.backward()
    np.testing.assert_allclose(loss.detach().cpu().numpy(), z[name + "_value"], rtol=1e-5)
    for k in KC.FIELDS:
        g = getattr(m, KC.ATTR[k]).grad
        g = np.zeros_like(z[f"{name}_grad_{k}"]) if g is None else g.cpu().numpy()
        np.testing.assert_allclose(g, z[f"{name}_grad_{k}"], rtol=1e-4, atol=1e-7, err_msg=k)


def test_reference_config_training_step_runs():
    """regular.yaml-shaped penalty (alpha center_weighted at 100) plus NN and compat: forward -> loss -> backward ->
    auxiliary_loss -> optimizer.step()"""
    import scenes
    from gsgen_amd.renderer import CameraInfo
    z = KC.load("penalties")
    pen = {"alpha": {"type": "center_weighted", "value": 100.0}, "NN": {"value": 1.0}, "compat": {"type": "l1", "value": 1.0}}
    m = KC.model_from_raw({k: z["raw_" + k] for k in KC.FIELDS}, DEV, penalty=pen)
    m.setup_lr(KC.LR)
    m.set_optimizer(dict(type="Adam", opt_args=dict(eps=1e-15)))
    m.train()
    cams = [scenes.Camera(64, 48, fx=60.0, c2w=scenes.orbit(3.0, 20, 40 + 90 * i)) for i in range(2)]
    batch = {"c2w": np.stack([c.c2w for c in cams]), "camera_info": [CameraInfo(*c.intr) for c in cams]}
    mean0 = m.mean.detach().clone()
    out = m(batch)
    loss = out["rgb"].mean() + out["opacity"].mean()
    loss = loss + m.auxiliary_loss(1)
    loss.backward()
    m.post_backward()
    m.optimizer.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item() and not torch.equal(mean0, m.mean.detach())
