"""gsgen_point_normals on the MI355X through gsgen_amd.normals: normals, curvatures and frames against the fp64 restatement of
tests/normals_cases.py on 20 000-point clouds (bench's cfg2 cloud with 1 % far outliers, a noisy shell) at every list width, the
tie to gsgen_amd.knn's own lists, bit equality from run to run, the pytorch3d-shaped entry points, and a captured call."""
import numpy as np
import pytest
import torch

import normals_cases as NC

pytestmark = pytest.mark.gpu
DEV = "cuda"
KS = (3, 8, 30, 32, 33, 50, 64)


def bits(t):
    return t.contiguous().view(torch.int32)


def brute_idx(pts, K, chunk=2048):
    """the kernel's formula and tie rule in torch (test_gpu_density_points.brute_idx for the self search): dx*dx + dy*dy + dz*dz,
    d = p_j - p_i, then topk on (float bits << 32 | j); every point of these clouds is finite"""
    j = torch.arange(pts.shape[0], device=pts.device, dtype=torch.int64)
    out = []
    for a in range(0, pts.shape[0], chunk):
        q = pts[a:a + chunk]
        dx = pts[None, :, 0] - q[:, None, 0]
        dy = pts[None, :, 1] - q[:, None, 1]
        dz = pts[None, :, 2] - q[:, None, 2]
        d2 = dx * dx
        d2 = d2 + dy * dy
        d2 = d2 + dz * dz
        key = (d2.view(torch.int32).to(torch.int64) << 32) | j[None, :]
        out.append(torch.topk(key, K, dim=1, largest=False, sorted=True).values & 0xFFFFFFFF)
    return torch.cat(out)


_CASES = {}


def case(name):
    """-> (points as NumPy, points on the device, the brute-force list of 64 as NumPy), built once"""
    if name not in _CASES:
        if name == "cfg2+outliers":  # the cloud of test_gpu_density_points.case(): 20 000 points of bench's cfg2, 1 % at 100 x the radius
            import bench
            from test_gpu_density_points import with_outliers
            sc, _, _ = bench.make_workload("cfg2")
            p = torch.tensor(sc["mean"], dtype=torch.float32)
            p = with_outliers(p[torch.randperm(p.shape[0], generator=torch.Generator().manual_seed(4))[:20000]]).numpy()
        else:
            p = NC.shell(20000, 21)
        t = torch.tensor(p, device=DEV)
        _CASES[name] = (p, t, brute_idx(t, 64).cpu().numpy().astype(np.int32))
    return _CASES[name]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", ("cfg2+outliers", "shell"))
def test_normals_against_fp64(name, K):
    """bounds and caps of normals_cases on the brute-force list; for K <= 32 that list is knn_raw's, row for row; two runs
    bit-identical; disambiguation off gives the same directions up to sign"""
    from gsgen_amd.knn import knn_raw
    from gsgen_amd.normals import normals_raw
    p, t, idx64 = case(name)
    idx = np.ascontiguousarray(idx64[:, :K])
    out = normals_raw(t, K, True)
    again = normals_raw(t, K, True)
    off = normals_raw(t, K, False)
    if K <= 32:
        own = knn_raw(t, K)[1].cpu().numpy()
        np.testing.assert_array_equal(own, idx)
        idx = own  # (the verdict below is on the existing search's own list)
    for k in out:
        assert torch.equal(bits(out[k]), bits(again[k])), k
    out, off = ({k: v.cpu().numpy() for k, v in o.items()} for o in (out, off))
    NC.check_against_fp64(name, p, idx, K, True, out, is_designated=True)
    NC.check_against_fp64(name, p, idx, K, False, off, is_designated=True)
    assert out["curvature"].tobytes() == off["curvature"].tobytes()
    assert np.array_equal(np.abs(out["normals"]), np.abs(off["normals"]))


def test_entry_points_agree_with_normals_raw():
    from gsgen_amd import normals as GN
    _, t, _ = case("shell")
    a, b = t[:5000].contiguous(), (t[5000:10000] * 1.5 + 0.25).contiguous()
    for K, dis in ((30, True), (50, False)):
        ra, rb = GN.normals_raw(a, K, dis), GN.normals_raw(b, K, dis)
        n = GN.estimate_normal(a, K, dis)
        assert n.shape == (5000, 3) and n.dtype == torch.float32 and not n.requires_grad
        assert torch.equal(bits(n), bits(ra["normals"]))
        nn = GN.estimate_pointcloud_normals(torch.stack([a, b]), K, dis)
        assert nn.shape == (2, 5000, 3) and torch.equal(bits(nn[0]), bits(ra["normals"])) and torch.equal(bits(nn[1]), bits(rb["normals"]))
        cur, fr = GN.estimate_pointcloud_local_coord_frames(torch.stack([a, b]), K, dis)
        assert cur.shape == (2, 5000, 3) and fr.shape == (2, 5000, 3, 3)
        assert torch.equal(bits(cur[1]), bits(rb["curvature"])) and torch.equal(bits(fr[0]), bits(ra["frames"]))
        cur1, fr1 = GN.estimate_pointcloud_local_coord_frames(a, K, dis)  # one cloud without the batch axis
        assert torch.equal(bits(cur1), bits(ra["curvature"])) and torch.equal(bits(fr1), bits(ra["frames"]))
        only = GN.normals_raw(a, K, dis, want=("curvature",))
        assert list(only) == ["curvature"] and torch.equal(bits(only["curvature"]), bits(ra["curvature"]))
    d = GN.estimate_normal(a.double().requires_grad_(), 8)  # (made float32; no graph)
    assert d.dtype == torch.float32 and not d.requires_grad
    assert torch.equal(bits(GN.estimate_normal(a)), bits(GN.normals_raw(a, 50)["normals"]))  # pytorch3d's default neighbourhood


def test_errors():
    from gsgen_amd import normals as GN
    _, t, _ = case("shell")
    small = t[:30].contiguous()
    msg = "The neighborhood_size argument has to be >= size of each of the point clouds."
    for call in (lambda: GN.estimate_normal(small, 30), lambda: GN.estimate_normal(small),
                 lambda: GN.estimate_pointcloud_normals(small[None], 31),
                 lambda: GN.estimate_pointcloud_local_coord_frames(small[None], 50), lambda: GN.normals_raw(small, 64)):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == msg
    assert GN.estimate_normal(small, 29).shape == (30, 3)
    with pytest.raises(NotImplementedError, match="gsgen_amd.normals"):
        GN.estimate_normal(t, 65)
    with pytest.raises(NotImplementedError, match="gsgen_amd.normals"):
        GN.estimate_normal(t, 2)
    with pytest.raises(ValueError, match="gsgen_amd.normals.*CUDA"):
        GN.estimate_normal(t.cpu(), 8)
    with pytest.raises(ValueError, match="gsgen_amd.normals"):
        GN.estimate_normal(t[:, :2], 8)
    with pytest.raises(ValueError, match="gsgen_amd.normals"):
        GN.estimate_pointcloud_normals(t[None, None], 8)
    with pytest.raises(ValueError, match="gsgen_amd.normals.*want"):
        GN.normals_raw(t, 8, want=())
    with pytest.raises(ValueError, match="gsgen_amd.normals.*want"):
        GN.normals_raw(t, 8, want=("normal",))


def test_estimate_normal_replays_in_a_captured_graph():
    """one linear chain of launches on the capturing stream; a replay reads the point values then in the tensor"""
    from gsgen_amd.normals import estimate_normal
    _, t, _ = case("cfg2+outliers")
    pts = t.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        estimate_normal(pts, 30)  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = estimate_normal(pts, 30)
    before = got.clone()
    pts.copy_(t.flip(0) * 0.8 + 0.01)
    graph.replay()
    eager = estimate_normal(pts, 30)
    torch.cuda.synchronize()
    assert torch.equal(bits(got), bits(eager)) and not torch.equal(bits(got), bits(before))
    assert bool((eager.norm(dim=1) - 1).abs().max() < 1e-5)
