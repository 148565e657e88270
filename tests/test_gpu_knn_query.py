"""gsgen_knn_query and gsgen_density_grid (gsgen_amd/csrc/knn.hip) on the MI355X through gsgen_amd.knn / gsgen_amd.density: exact
against a torch brute force for queries that are not points of the cloud, deterministic, capturable; the density lattice against
the reference's own grid (tests/golden/density) and through every Python entry point."""
import numpy as np
import pytest
import torch

import density_cases as DC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def brute(pts, qs, K, chunk=2048):
    """the kernel's formula and tie rule in torch: dx*dx + dy*dy + dz*dz (d = p_j - q), then topk on (float bits << 32 | j)"""
    N = pts.shape[0]
    out_d, out_i = [], []
    j = torch.arange(N, device=pts.device, dtype=torch.int64)
    for a in range(0, qs.shape[0], chunk):
        q = qs[a:a + chunk]
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


_CLOUD = {}


def cloud(outliers=False):
    """20 000 points of bench's cfg2 cloud (a fixed random subset), plain or with 1 % far outliers"""
    if not _CLOUD:
        import bench
        sc, _, _ = bench.make_workload("cfg2")
        p = torch.tensor(sc["mean"], dtype=torch.float32)
        p = p[torch.randperm(p.shape[0], generator=torch.Generator().manual_seed(4))[:20000]].to(DEV)
        _CLOUD[False], _CLOUD[True] = p, with_outliers(p)
    return _CLOUD[outliers]


def make_queries(p, n=8192, seed=9):
    """half jittered points, a quarter uniform in 1.1 x the bounding box, a quarter at 3 .. 100 x the radius"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    pc = p.cpu()
    med = pc.median(0).values
    r = float((pc - med).norm(dim=1).quantile(0.98))  # (the core's radius: far outliers do not set it)
    jit = pc[torch.randint(0, pc.shape[0], (n // 2,), generator=g)] + 1e-3 * r * torch.randn(n // 2, 3, generator=g)
    lo, hi = pc.min(0).values, pc.max(0).values
    ctr, half = (lo + hi) / 2, (hi - lo) / 2 * 1.1
    uni = ctr + (torch.rand(n // 4, 3, generator=g) * 2 - 1) * half
    d = torch.randn(n // 4, 3, generator=g)
    far = med + d / d.norm(dim=1, keepdim=True) * r * torch.exp(torch.empty(n // 4, 1).uniform_(np.log(3.0), np.log(100.0), generator=g))
    q = torch.cat([jit, uni, far])
    return q[torch.randperm(q.shape[0], generator=g)].to(p.device)


_REF = {}


def reference(outliers):
    if outliers not in _REF:
        p = cloud(outliers)
        q = make_queries(p)
        _REF[outliers] = (p, q) + brute(p, q, 32)
    return _REF[outliers]


@pytest.mark.parametrize("outliers", [False, True])
def test_knn_query_is_the_brute_force(outliers):
    from gsgen_amd.knn import knn_raw
    p, q, bd, bi = reference(outliers)
    for K in (1, 4, 8, 32):
        d, i = knn_raw(p, K, query=q)
        torch.cuda.synchronize()
        assert d.shape == (q.shape[0], K) and i.dtype == torch.int32
        assert torch.equal(i.long(), bi[:, :K]), (K, int((i.long() != bi[:, :K]).sum()))
        assert torch.equal(d.view(torch.int32), bd[:, :K].contiguous().view(torch.int32)), K


def test_knn_query_nan_queries_nan_points_and_determinism():
    from gsgen_amd.knn import knn_points, knn_raw
    p, q, _, _ = reference(True)
    p, q = p.clone(), q[:3000].clone()
    p[7, 1] = float("nan")
    p[9] = float("inf")
    p[100:120, 2] = float("nan")
    q[5, 0] = float("nan")
    q[11] = float("-inf")
    d, i = knn_points(p, 4, query=q)
    finp, finq = torch.isfinite(p).all(1), torch.isfinite(q).all(1)
    pp = p.clone()
    pp[~finp] = 1e30  # (the brute force: far away instead of non-finite)
    bd, bi = brute(pp, q[finq], 4)
    assert torch.equal(i[finq], bi) and torch.equal(d[finq].view(torch.int32), bd.view(torch.int32))
    assert (i[~finq] == -1).all() and torch.isinf(d[~finq]).all() and int((~finq).sum()) == 2
    assert not torch.isin(i, torch.nonzero(~finp).reshape(-1)).any()
    a, b = knn_raw(p, 8, query=q), knn_raw(p, 8, query=q)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_K_nearest_neighbors_with_and_without_a_query():
    from gsgen_amd import knn as KNN
    p, q, bd, bi = reference(False)
    nn, idx, dist = KNN.K_nearest_neighbors(p, 4, query=q, return_dist=True)
    assert idx.shape == (q.shape[0], 3) and idx.dtype == torch.int64
    assert torch.equal(idx, bi[:, 1:4]) and torch.equal(nn, p[bi[:, 1:4]])
    assert torch.equal(dist.view(torch.int32), bd[:, 1:4].contiguous().view(torch.int32))
    nn2, idx2 = KNN.K_nearest_neighbors(p, 4, query=q)
    assert torch.equal(idx2, idx) and torch.equal(nn2, nn)
    sd, si = brute(p, p, 4)  # query=None: the self search, as before
    nn, idx, dist = KNN.K_nearest_neighbors(p, 4, return_dist=True)
    assert torch.equal(idx, si[:, 1:]) and torch.equal(nn, p[si[:, 1:]]) and torch.equal(dist.view(torch.int32), sd[:, 1:].contiguous().view(torch.int32))
    d0, i0 = KNN.knn_raw(p, 4)
    d1, i1 = KNN.knn_raw(p, 4, query=None)
    assert torch.equal(i0, i1) and torch.equal(d0.view(torch.int32), d1.view(torch.int32)) and torch.equal(i0.long(), si)
    with pytest.raises(NotImplementedError):  # (no CPU implementation)
        KNN.knn_raw(p, 4, query=q.cpu())


def golden_fields():
    z = DC.load_golden()
    t = {k: torch.tensor(z[k], device=DEV) for k in ("mean", "qvec", "svec", "alpha", "scale", "opacity", "axis")}
    return z, t


def test_knn_query_and_density_grid_replay_in_a_captured_graph():
    from gsgen_amd.density import density_grid
    from gsgen_amd.knn import knn_points
    p, q, _, _ = reference(False)
    z, t = golden_fields()
    sp, sq = p.clone(), q.clone()
    sm, sqv, ss, so = (t[k].clone() for k in ("mean", "qvec", "scale", "opacity"))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        knn_points(sp, 4, query=sq)  # (warm-up outside the capture)
        density_grid(sm, sqv, ss, so, 1.5, 20)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gd, gi = knn_points(sp, 4, query=sq)
        gg = density_grid(sm, sqv, ss, so, 1.5, 20)
    sp.copy_(with_outliers(p, 0.05, seed=3) * 0.5)
    sq.copy_(q.flip(0) * 0.7 + 0.01)
    sm.copy_(t["mean"].flip(0) * 0.8)
    ss.copy_(t["scale"] * 1.5)
    so.copy_(t["opacity"].flip(0))
    graph.replay()
    ed, ei = knn_points(sp, 4, query=sq)
    eg = density_grid(sm, sqv, ss, so, 1.5, 20)
    torch.cuda.synchronize()
    assert torch.equal(gi, ei) and torch.equal(gd.view(torch.int32), ed.view(torch.int32))
    assert torch.equal(gg.view(torch.int32), eg.view(torch.int32)) and float(eg.max()) > 0


def test_density_grid_matches_the_reference_golden():
    """tests/golden/density: on the fixture's lattice (the reference's CPU linspace: a device linspace need not give the same bits, so
    the coordinates go in as arrays) the kernel's grid lies within the per-point bound of the fp64 grid, its max-abs and RMS error
    at most twice the reference's own; L as get_density_val_grid_from_ckpt derives it equals the reference's"""
    from gsgen_amd.density import density_grid_axes, get_density_val_grid_from_ckpt
    z, t = golden_fields()
    out = density_grid_axes(t["mean"], t["qvec"], t["scale"], t["opacity"], t["axis"], t["axis"], t["axis"], int(z["K"]), True)
    assert out.shape == (24, 24, 24) and out.dtype == torch.float32
    DC.check_golden_grid(out.cpu().numpy(), z)
    _, L = get_density_val_grid_from_ckpt({k: t[k] for k in ("mean", "qvec", "svec", "alpha")}, reso=4, K=int(z["K"]))
    assert L == float(z["L"])
    # the kernel's neighbour set on the device = the fixture's (K + 1 nearest, nearest dropped): the other choice is far off
    other = density_grid_axes(t["mean"], t["qvec"], t["scale"], t["opacity"], t["axis"], t["axis"], t["axis"], int(z["K"]), False)
    assert int(((other.cpu().numpy() - z["grid64"]) > z["bound"]).sum()) > 1000


def test_density_entry_points_agree_at_reso_32():
    from gsgen_amd.density import density_grid, get_density_val_grid_from_ckpt
    import knn_cases as KC
    z, t = golden_fields()
    ckpt = {k: t[k] for k in ("mean", "qvec", "svec", "alpha")}
    grid, L = get_density_val_grid_from_ckpt(ckpt, batch_size=7, reso=32, K=3)
    assert L == float(z["L"]) and grid.shape == (32, 32, 32)
    direct = density_grid(t["mean"], t["qvec"], torch.exp(t["svec"]), torch.sigmoid(t["alpha"]), L, 32, K=3, skip_nearest=True)
    assert torch.equal(grid.view(torch.int32), direct.view(torch.int32)) and float(grid.max()) > 0.1
    grid2, L2 = get_density_val_grid_from_ckpt(ckpt, L=1.0, reso=32, K=3)
    assert L2 == 1.0 and not torch.equal(grid2, grid)
    raw = {"mean": z["mean"], "qvec": z["qvec"], "svec": z["svec"], "alpha": z["alpha"], "color": np.zeros((z["mean"].shape[0], 3), np.float32)}
    m = KC.model_from_raw(raw, DEV)
    mg = m.get_density_val_grid(L, 32, K=3)
    assert torch.equal(mg.view(torch.int32), grid.view(torch.int32))
    assert torch.equal(m.get_density_val_grid(-1.0, 32).view(torch.int32), grid.view(torch.int32))
