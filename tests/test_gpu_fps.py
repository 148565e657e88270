"""gsgen_amd.fps on the MI355X against the fp32 NumPy reference of tests/fps_cases.py: the whole index array, exactly."""
import numpy as np
import pytest
import torch

from fps_cases import CLOUDS, NAMES, fps_reference, reference, with_rgb

pytestmark = pytest.mark.gpu

from gsgen_amd import fps  # noqa: E402
from gsgen_amd.fps import AUTO_BUCKET_MIN_POINTS, BRUTE_REG_POINTS, BRUTE_THREADS, farthest_point_sampling, sample_farthest_points  # noqa: E402

DEV = "cuda"
K_CLOUD = 256


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def starts(*s):
    return torch.tensor(s, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("method", ["auto", "brute", "bucket"])
@pytest.mark.parametrize("name", NAMES)
def test_fps_is_the_reference_on_every_cloud(name, method):
    pts, s0 = CLOUDS[name]
    K = min(K_CLOUD, pts.shape[0])
    p = dev(pts)
    got_pts, got = farthest_point_sampling(p, K, start_idx=starts(s0)[0], method=method)
    want = reference(name, K)
    assert got.dtype == torch.int64 and got.shape == (K,) and got_pts.shape == (K, 3)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    pad = want < 0
    exp = pts[np.maximum(want, 0)]
    exp[pad] = 0
    assert got_pts.cpu().numpy().tobytes() == exp.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_fps_brute_with_six_coordinates(name):
    pts, s0 = with_rgb(name)
    K = min(K_CLOUD, pts.shape[0])
    _, got = sample_farthest_points(dev(pts)[None], K=K, start_idx=starts(s0), method="auto")
    np.testing.assert_array_equal(got[0].cpu().numpy(), reference(name, K, 6))


REG_EDGE = BRUTE_REG_POINTS * BRUTE_THREADS


@pytest.mark.parametrize("D", [3, 6])
@pytest.mark.parametrize("L", [1, 2, 1023, 1024, 1025, REG_EDGE - 1, REG_EDGE, REG_EDGE + 1])
def test_fps_sizes_around_the_kernel_boundaries(L, D):
    rng = np.random.default_rng(L + D)
    pts = rng.uniform(-1, 1, (L, D)).astype(np.float32)
    K, s0 = min(L, 8), L // 2
    want = fps_reference(pts, K, s0)
    for method in ("brute", "bucket") if D == 3 else ("brute",):
        _, got = farthest_point_sampling(dev(pts), K, start_idx=starts(s0)[0], method=method)
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=method)


@pytest.mark.parametrize("L", [AUTO_BUCKET_MIN_POINTS - 1, AUTO_BUCKET_MIN_POINTS, AUTO_BUCKET_MIN_POINTS + 1])
def test_fps_auto_around_the_crossover(L):
    rng = np.random.default_rng(L)
    pts = rng.normal(size=(L, 3)).astype(np.float32)
    _, got = farthest_point_sampling(dev(pts), 16, start_idx=starts(L - 1)[0], method="auto")
    np.testing.assert_array_equal(got.cpu().numpy(), fps_reference(pts, 16, L - 1))


@pytest.mark.parametrize("method", ["brute", "bucket"])
def test_fps_batch_of_different_lengths_is_padded(method):
    a, b, c = CLOUDS["uniform"][0][:1200], CLOUDS["clustered"][0][:1200], CLOUDS["nan_rows"][0][:1200]
    pts = np.stack([a, b, c])
    lengths, s = [1200, 333, 20], [5, 400, 0]
    sampled, idx = sample_farthest_points(dev(pts), torch.tensor(lengths, device=DEV), K=64, start_idx=starts(*s), method=method)
    for r in range(3):
        want = fps_reference(pts[r], 64, s[r], lengths[r])
        np.testing.assert_array_equal(idx[r].cpu().numpy(), want)
        exp = pts[r][np.maximum(want, 0)]
        exp[want < 0] = 0
        assert sampled[r].cpu().numpy().tobytes() == exp.tobytes()
    assert (idx[2] == -1).sum() > 44 and (sampled[2][idx[2] < 0] == 0).all()  # 20 rows, some of them not finite


@pytest.mark.parametrize("method", ["brute", "bucket"])
def test_fps_expanded_batch_is_the_shared_cloud_is_three_single_calls(method):
    pts, _ = CLOUDS["outliers"]
    p = dev(pts)
    s = starts(11, 2000, 977)
    e_pts, e_idx = farthest_point_sampling(p[None].expand(3, -1, -1), 48, start_idx=s, method=method)
    s_pts, s_idx = farthest_point_sampling(p, 48, start_idx=s, method=method)
    c_pts, c_idx = farthest_point_sampling(p[None].repeat(3, 1, 1), 48, start_idx=s, method=method)
    assert s_idx.shape == (3, 48) and s_pts.shape == (3, 48, 3)
    for r in range(3):
        one_pts, one_idx = farthest_point_sampling(p, 48, start_idx=s[r], method=method)
        np.testing.assert_array_equal(one_idx.cpu().numpy(), fps_reference(pts, 48, int(s[r])))
        for other_pts, other_idx in ((e_pts, e_idx), (s_pts, s_idx), (c_pts, c_idx)):
            assert torch.equal(other_idx[r], one_idx) and torch.equal(other_pts[r], one_pts)


def test_fps_gradients_reach_points_through_the_gather():
    pts = dev(CLOUDS["nan_rows"][0][:60]).requires_grad_(True)
    sampled, idx = sample_farthest_points(pts[None], K=64, start_idx=starts(3))  # (padded: fewer than 64 finite rows)
    assert (idx < 0).any()
    sampled.sum().backward()
    want = torch.zeros_like(pts)
    want.index_put_((idx[0][idx[0] >= 0],), torch.ones(3, device=DEV), accumulate=True)
    assert torch.equal(pts.grad, want)
    shared = dev(CLOUDS["uniform"][0]).requires_grad_(True)
    s_pts, s_idx = farthest_point_sampling(shared, 16, start_idx=starts(1, 2))
    s_pts.sum().backward()
    want = torch.zeros_like(shared)
    want.index_put_((s_idx.reshape(-1),), torch.ones(3, device=DEV), accumulate=True)
    assert torch.equal(shared.grad, want)


@pytest.mark.parametrize("method", ["brute", "bucket"])
def test_fps_captured_shared_cloud_replays_on_new_points_and_starts(method):
    a, b = CLOUDS["uniform"][0], CLOUDS["clustered"][0][:3000]
    b = np.concatenate([b, CLOUDS["planar"][0][:3000 - b.shape[0]]])
    p = dev(a)
    s = starts(1, 2, 3)
    farthest_point_sampling(p, 32, start_idx=s, method=method)  # (loads the library outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _, idx = farthest_point_sampling(p, 32, start_idx=s, method=method)
    p.copy_(dev(b))
    s.copy_(starts(2999, -1, 70))
    g.replay()
    torch.cuda.synchronize()
    got = idx.cpu().numpy()
    _, eager = farthest_point_sampling(p, 32, start_idx=s, method=method)
    assert torch.equal(idx, eager)
    for r, s0 in enumerate((2999, -1, 70)):
        np.testing.assert_array_equal(got[r], fps_reference(b, 32, s0))


def test_fps_random_start():
    p = dev(CLOUDS["uniform"][0])[None].expand(4, -1, -1)
    torch.manual_seed(7)
    _, i1 = sample_farthest_points(p, K=8, random_start_point=True)
    torch.manual_seed(7)
    _, i2 = sample_farthest_points(p, K=8, random_start_point=True)
    assert torch.equal(i1, i2) and len(set(i1[:, 0].tolist())) > 1
    torch.manual_seed(7)
    drawn = [int(torch.randint(3000, ())) for _ in range(4)]
    assert i1[:, 0].tolist() == drawn
    g = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="random_start_point"):
        with torch.cuda.graph(g):
            sample_farthest_points(p, K=8, random_start_point=True)


def test_fps_argument_checks():
    p = dev(CLOUDS["uniform"][0])
    with pytest.raises(ValueError):
        farthest_point_sampling(p.cpu(), 4)
    with pytest.raises(NotImplementedError):
        farthest_point_sampling(p[:, :2].contiguous(), 4)
    with pytest.raises(NotImplementedError):
        farthest_point_sampling(torch.cat([p, p], 1), 4, method="bucket")
    with pytest.raises(ValueError):
        farthest_point_sampling(p, 0)
    with pytest.raises(ValueError):
        farthest_point_sampling(p, 4, method="fast")
    with pytest.raises(ValueError):
        sample_farthest_points(p[None], K=4, start_idx=starts(1, 2))
    assert fps.BUCKETS_MAX == 4096
