"""gsgen_density_points (gsgen_amd/csrc/knn.hip) on the MI355X through gsgen_amd.density.field_at: the value bit-equal to the
lattice kernel's, value / gradient / colour against the fp64 restatement of tests/density_points_cases.py on a 20 000-point cloud
with far outliers, bit equality from run to run, a captured call, and the Python entry point's forms."""
import numpy as np
import pytest
import torch

import density_cases as DC
import density_points_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = [(1, 0), (3, 1), (8, 1), (31, 1)]  # Ks = 1, 4, 9, 32
KS_LIST = tuple(K + s for K, s in CASES)


def bits(t):
    return t.contiguous().view(torch.int32)


def golden_fields():
    z = DC.load_golden()
    return z, {k: torch.tensor(z[k], device=DEV) for k in ("mean", "qvec", "scale", "opacity", "axis")}


@pytest.mark.parametrize("K,skip", [(1, 0), (2, 0), (2, 1), (4, 1), (8, 1), (16, 1), (31, 1)])
def test_field_at_equals_the_lattice_bit_for_bit(K, skip):
    """the golden fields on their own 24^3 lattice, at every list width: field_at(...).density at the lattice's points is
    density_grid_axes', bit for bit; gradient and colour do not change it"""
    from gsgen_amd.density import density_grid_axes, field_at
    z, t = golden_fields()
    ax = t["axis"]
    grid = density_grid_axes(t["mean"], t["qvec"], t["scale"], t["opacity"], ax, ax, ax, K, bool(skip))
    pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1)  # [24, 24, 24, 3]
    color = torch.rand(t["mean"].shape[0], 3, device=DEV)
    f = field_at(t["mean"], t["qvec"], t["scale"], t["opacity"], pts, K, bool(skip), color=color)
    assert f.density.shape == (24, 24, 24) and f.grad.shape == (24, 24, 24, 3) and f.rgb.shape == (24, 24, 24, 3)
    assert torch.equal(bits(f.density), bits(grid)) and int((grid > 1e-6).sum()) > 500
    only = field_at(t["mean"], t["qvec"], t["scale"], t["opacity"], pts, K, bool(skip), grad=False)
    assert only.grad is None and only.rgb is None and torch.equal(bits(only.density), bits(grid))


def brute_idx(pts, qs, K, chunk=2048):
    """the kernel's formula and tie rule in torch: dx*dx + dy*dy + dz*dz (d = p_j - q), then topk on (float bits << 32 | j);
    a non-finite query's row is -1"""
    N = pts.shape[0]
    out = []
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
        out.append(torch.where(torch.isfinite(q).all(1, keepdim=True), k & 0xFFFFFFFF, torch.full_like(k, -1)))
    return torch.cat(out)


def with_outliers(p, frac=0.01, seed=0):
    """frac of the points moved to 100x the cloud's radius (random directions): test_gpu_knn_query.with_outliers, rebuilt"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    c = p.mean(0)
    r = float((p - c).norm(dim=1).max())
    n = int(p.shape[0] * frac)
    sel = torch.randperm(p.shape[0], generator=g)[:n]
    d = torch.randn(n, 3, generator=g)
    q = p.clone()
    q[sel] = c + 100.0 * r * d / d.norm(dim=1, keepdim=True)
    return q


_CASE = {}


def case():
    """20 000 points of bench's cfg2 cloud (the fixed random subset of test_gpu_knn_query.cloud) with 1 % far outliers, fields from
    density_points_cases.fields_for, and 4 096 queries: jittered centres, exact copies, uniform in 1.1 x the bounding box, 3 .. 100 x
    the core's radius away, two non-finite rows; drawn with a surplus and filtered by density_points_cases.gap_free.  -> (g as
    NumPy, g as tensors, queries, the brute-force list of 32)"""
    if not _CASE:
        import bench
        sc, _, _ = bench.make_workload("cfg2")
        p = torch.tensor(sc["mean"], dtype=torch.float32)
        p = with_outliers(p[torch.randperm(p.shape[0], generator=torch.Generator().manual_seed(4))[:20000]]).numpy()
        g = PC.fields_for(p, 77)
        rng = np.random.default_rng(78)
        med = np.median(p, axis=0).astype(np.float64)
        r = float(np.quantile(np.linalg.norm(p - med, axis=1), 0.98))
        s = float(np.median(g["scale"]))
        jit = p[rng.integers(0, p.shape[0], 2200)] + s * rng.normal(size=(2200, 3)) * rng.uniform(0.1, 3.0, (2200, 1))
        copies = p[rng.integers(0, p.shape[0], 300)]
        lo, hi = p.min(0).astype(np.float64), p.max(0).astype(np.float64)
        uni = (lo + hi) / 2 + (rng.uniform(size=(900, 3)) * 2 - 1) * (hi - lo) / 2 * 1.1
        d = rng.normal(size=(1200, 3))
        far = med + d / np.linalg.norm(d, axis=1, keepdims=True) * r * np.exp(rng.uniform(np.log(3.0), np.log(100.0), (1200, 1)))
        q = np.concatenate([jit, copies, uni, far]).astype(np.float32)
        q = q[rng.permutation(q.shape[0])]
        tg = {k: torch.tensor(v, device=DEV) for k, v in g.items()}
        idx = brute_idx(tg["mean"], torch.tensor(q, device=DEV), 32).cpu().numpy().astype(np.int32)
        keep = PC.gap_free(g, q, KS_LIST, idx=idx)
        q, idx = q[keep][:4096].copy(), idx[keep][:4096].copy()
        assert q.shape[0] == 4096
        q[1], q[300] = (np.nan, 0.0, 0.0), (0.0, -np.inf, 1.0)
        idx[[1, 300]] = -1
        _CASE["c"] = (g, tg, q, idx)
    return _CASE["c"]


_RUNS = {}


def run(K, skip):
    from gsgen_amd.density import field_at
    if (K, skip) not in _RUNS:
        g, tg, q, _ = case()
        f = field_at(tg["mean"], tg["qvec"], tg["scale"], tg["opacity"], torch.tensor(q, device=DEV), K, bool(skip), color=tg["color"])
        again = field_at(tg["mean"], tg["qvec"], tg["scale"], tg["opacity"], torch.tensor(q, device=DEV), K, bool(skip), color=tg["color"])
        torch.cuda.synchronize()
        for a, b in zip(f, again):  # two runs: the same bits
            assert torch.equal(bits(a), bits(b))
        _RUNS[K, skip] = tuple(x.cpu().numpy() for x in f)
    return _RUNS[K, skip]


@pytest.mark.parametrize("K,skip", CASES)
def test_field_at_against_fp64(K, skip):
    """value, gradient and colour within the counted bounds, the colour's fallback rows bit-equal to the nearest centre's colour,
    non-finite queries zero; two runs bit-identical"""
    g, _, q, idx = case()
    density, grad, rgb = run(K, skip)
    low = PC.check_against_fp64("cfg2+outliers", g, q, np.ascontiguousarray(idx[:, :K + skip]), K, skip, density, grad, rgb)
    assert 100 <= low <= 3000, low  # (both branches of the colour are taken)
    assert (np.abs(grad).max(1) > 1e-3).sum() >= 1000


def test_field_at_replays_in_a_captured_graph():
    from gsgen_amd.density import field_at
    g, tg, q, _ = case()
    s = {k: v.clone() for k, v in tg.items()}
    sq = torch.tensor(q[:3000], device=DEV)
    call = lambda: field_at(s["mean"], s["qvec"], s["scale"], s["opacity"], sq, 3, True, color=s["color"])  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = call()
    before = [x.clone() for x in got]
    s["mean"].copy_(tg["mean"].flip(0) * 0.8)
    s["scale"].copy_(tg["scale"] * 1.5)
    s["opacity"].copy_(tg["opacity"].flip(0))
    s["color"].copy_(tg["color"].flip(0))
    sq.copy_(torch.nan_to_num(sq.flip(0), nan=0.0, posinf=1.0, neginf=-1.0) * 0.7 + 0.01)
    graph.replay()
    eager = call()
    torch.cuda.synchronize()
    for a, b, c in zip(got, eager, before):
        assert torch.equal(bits(a), bits(b)) and not torch.equal(bits(a), bits(c))
    assert float(eager.density.max()) > 0.1


def test_field_at_forms_and_checks():
    from gsgen_amd.density import field_at
    z, t = golden_fields()
    args = (t["mean"], t["qvec"], t["scale"], t["opacity"])
    pts = t["mean"][:50] + 0.01
    color = torch.rand(t["mean"].shape[0], 3, device=DEV)
    full = field_at(*args, pts, color=color)
    assert full._fields == ("density", "grad", "rgb") and full.density.shape == (50,) and full.grad.shape == (50, 3)
    assert full.rgb.dtype == torch.float32 and full.rgb.is_cuda
    lo, hi = color.min(0).values, color.max(0).values
    assert bool((full.rgb >= lo).all()) and bool((full.rgb <= hi).all())
    none = field_at(*args, pts, density=False, grad=False)
    assert none == (None, None, None)
    g_only = field_at(*args, pts.double().reshape(5, 10, 3), density=False)  # (made float32; leading dimensions kept)
    assert g_only.density is None and g_only.grad.shape == (5, 10, 3) and torch.equal(bits(g_only.grad.reshape(50, 3)), bits(full.grad))
    empty = field_at(*args, pts[:0], color=color)
    assert empty.density.shape == (0,) and empty.grad.shape == (0, 3) and empty.rgb.shape == (0, 3)
    with pytest.raises(ValueError, match="points"):
        field_at(*args, pts[:, :2])
    with pytest.raises(ValueError, match="color"):
        field_at(*args, pts, color=color[:5])
    with pytest.raises(ValueError, match="skip_nearest"):
        field_at(*args, pts, K=32, skip_nearest=True)
    with pytest.raises(ValueError, match="CUDA"):
        field_at(t["mean"].cpu(), *args[1:], pts)
