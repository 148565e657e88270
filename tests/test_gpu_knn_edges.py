"""The kNN index and its three consumers (gsgen_amd/csrc/knn_index.hpp, knn.hip) on the MI355X through gsgen_amd.knn /
gsgen_amd.density, at every list length, size edge and degenerate cloud: tests/knn_cases.py's clouds (clustered, planar, heavy
duplicates, far outliers, NaN rows, a fine cloud at a large offset, one position, a line, N = 1, N = K, N < 64, few distinct
positions) x K_MATRIX (every instantiation L = 1 .. 32 and a K below each L > 1) for the self and the query search, against the
NumPy brute force bit for bit; repeated runs where the bucket order differs from run to run; the scan at its tile boundary and in
its second chunk of 256 tiles; the density lattice at every list length; a captured query search at K = 16."""
import numpy as np
import pytest
import torch

import density_cases as DC
import knn_cases as KC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def search(pts, K, query=None):
    """knn_raw on device tensors -> (dist2, idx) as NumPy arrays"""
    from gsgen_amd.knn import knn_raw
    d, i = knn_raw(pts, K, query=query)
    assert d.dtype == torch.float32 and i.dtype == torch.int32 and d.shape == i.shape == ((pts if query is None else query).shape[0], K)
    return d.cpu().numpy(), i.cpu().numpy()


def torch_brute(pts, qs, K, chunk=256):
    """tests/test_gpu_knn.py's brute force for the rows qs (d = p_j - q; for rows of pts itself that is its d = p_j - p_i), in chunks
    of `chunk` rows: dx*dx + dy*dy + dz*dz, then topk on (float bits << 32 | j)"""
    j = torch.arange(pts.shape[0], device=pts.device, dtype=torch.int64)
    out_d, out_i = [], []
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
        out_i.append((k & 0xFFFFFFFF).to(torch.int32))
    return torch.cat(out_d).cpu().numpy(), torch.cat(out_i).cpu().numpy()


@pytest.mark.parametrize("name", sorted(KC.CLOUDS))
def test_self_and_query_search_over_the_K_matrix(name):
    pts, qs = dev(KC.CLOUDS[name]), dev(KC.QUERIES[name])
    (sd, si), (qd, qi) = KC.brute_self(name), KC.brute_queries(name)
    ran = 0
    for K in KC.K_MATRIX:
        if K > pts.shape[0]:
            continue
        d, i = search(pts, K)
        KC.same_bits(d, i, sd[:, :K], si[:, :K], f"{name} self K={K}")
        d, i = search(pts, K, qs)
        KC.same_bits(d, i, qd[:, :K], qi[:, :K], f"{name} query K={K}")
        ran += 1
    assert ran == sum(K <= pts.shape[0] for K in KC.K_MATRIX) and ran >= 1


@pytest.mark.parametrize("name", KC.DEGENERATE)
def test_degenerate_clouds(name):
    pts, qs = KC.CLOUDS[name], KC.QUERIES[name]
    K = min(4, pts.shape[0])
    d, i = search(dev(pts), K)
    bd, bi = KC.brute(pts, K)
    KC.same_bits(d, i, bd, bi, f"{name} self")
    assert (i >= 0).all() and np.isfinite(d).all()  # (N >= K finite points: no padded entry)
    if name == "same":  # forty copies of one point: the four lowest indices, whoever asks
        assert (i == np.arange(4)).all()
    d, i = search(dev(pts), K, dev(qs))
    bd, bi = DC.brute_query(pts, qs, K)
    KC.same_bits(d, i, bd, bi, f"{name} query")
    assert (i >= 0).all() and np.isfinite(d).all()
    if name == "same":
        assert (i == np.arange(4)).all()


def test_clouds_of_exactly_K_points():
    for K in KC.K_MATRIX:
        pts = KC.n_eq_k(K)
        d, i = search(dev(pts), K)
        bd, bi = KC.brute(pts, K)
        KC.same_bits(d, i, bd, bi, f"N = K = {K} self")
        assert (np.sort(i, axis=1) == np.arange(K)).all()  # every row lists the whole cloud
        qs = KC.queries_for(pts, 64, seed=K)
        d, i = search(dev(pts), K, dev(qs))
        bd, bi = DC.brute_query(pts, qs, K)
        KC.same_bits(d, i, bd, bi, f"N = K = {K} query")


@pytest.mark.parametrize("name,Ks", [("few_distinct", (4, 16)), ("duplicates", (8,))])
def test_tied_clouds_give_the_same_bytes_twice(name, Ks):
    """the in-bucket order k_knn_scatter's atomics leave differs from run to run on hardware; the result must not"""
    pts, qs = dev(KC.CLOUDS[name]), dev(KC.QUERIES[name])
    on_top = pts[:300].clone()  # (queries on top of the positions: ties of the query search)
    for K in Ks:
        for q in (None, qs, on_top):
            a, b = search(pts, K, q), search(pts, K, q)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (name, K)
        if name == "few_distinct":  # every tie set is larger than K: the K lowest indices at the position, distance 0
            _, inv, cnt = np.unique(KC.CLOUDS[name], axis=0, return_inverse=True, return_counts=True)
            inv = inv.reshape(-1)
            assert cnt.size == 50 and cnt.min() > K
            lowest = np.stack([np.nonzero(inv == g)[0][:K] for g in range(50)])
            d, i = search(pts, K)
            np.testing.assert_array_equal(i, lowest[inv])
            assert (d == 0).all()
            np.testing.assert_array_equal(search(pts, K, on_top)[1], lowest[inv[:300]])


@pytest.mark.parametrize("N", KC.SCAN_SMALL)
def test_scan_at_the_tile_boundary(N):
    """K = 2: cap = N / 2 cells, cap + 3 scanned entries = 1024 (one full tile) and 1025 (a second tile of one entry)"""
    assert N // 2 + 3 in (1024, 1025)
    pts = KC.scan_cloud(N)
    d, i = search(dev(pts), 2)
    bd, bi = KC.brute(pts, 2)
    KC.same_bits(d, i, bd, bi, f"N = {N}")


def test_scan_carries_into_a_second_chunk_of_tiles():
    """N = 524 328, K = 2: cap + 3 = 262 167 entries = 257 scan tiles, so k_knn_scan_sums takes its second chunk of 256 with the carry
    of the first.  4 096 seeded rows against the torch brute force, and every row against what holds without exact duplicates."""
    N = KC.SCAN_LARGE
    assert (N // 2 + 3 + 1023) // 1024 == 257
    pts = KC.scan_cloud(N)
    assert KC.no_exact_duplicates(pts)
    p = dev(pts)
    d, i = search(p, 2)
    KC.check_whole_array(pts, d, i)
    rows = np.sort(np.random.default_rng(7).choice(N, 4096, replace=False))
    bd, bi = torch_brute(p, p[dev(rows)], 2, chunk=256)
    KC.same_bits(d[rows], i[rows], bd, bi, f"N = {N}, 4 096 rows")


# What the lattice may differ from the fp64 sum by, in units of density_cases.density64's bound.  1: the host rule, unloosened (the
# device's expf did not need more: see the measurement in test_density_grid_at_every_list_length).
DENSITY_ALLOWANCE = 1.0


@pytest.fixture(scope="module")
def golden_scene():
    z = DC.load_golden()
    g = {k: z[k] for k in ("mean", "qvec", "scale", "opacity")}
    return g, {k: dev(v) for k, v in g.items()}


@pytest.mark.parametrize("K,skip", KC.DENSITY_KS)
def test_density_grid_at_every_list_length(golden_scene, K, skip):
    """k_density_grid<L> for L = 1, 2, 2, 16, 16, 32, 32, 32 on three lattice shapes with three different axes each.  The kept
    neighbours are exact: knn_raw(query=lattice) with K + skip is the brute force's.  The value lies within DENSITY_ALLOWANCE x
    the bound density_cases.density64 returns against the fp64 sum on those neighbours; that allowance is at least 10 x below the
    change that dropping the kept neighbour of the largest term causes, at every lattice point with mass (value > 1e-3), so a
    dropped or swapped neighbour cannot hide in it.
    MEASURED on the MI355X over the whole matrix (8 (K, skip) x 3 shapes): worst err / bound 0.29 (the emulator's: 0.29, at the
    same lattice point), so the host rule holds on the device as it stands and DENSITY_ALLOWANCE stays 1; the smallest drop /
    bound at a point with mass is 1 460."""
    from gsgen_amd.density import density_grid_axes
    g, t = golden_scene
    for shape in KC.DENSITY_SHAPES:
        ax, ay, az = KC.density_axes(g, shape)
        pts = DC.lattice(ax, ay, az)
        out = density_grid_axes(t["mean"], t["qvec"], t["scale"], t["opacity"], dev(ax), dev(ay), dev(az), K, bool(skip))
        assert tuple(out.shape) == shape and out.dtype == torch.float32
        out = out.cpu().numpy().reshape(-1)
        _, qi = search(t["mean"], K + skip, dev(pts))
        _, bi = DC.brute_query(g["mean"], pts, K + skip)
        np.testing.assert_array_equal(qi, bi)
        kept = DC.kept(qi, K, skip)
        val, bound = DC.density64(g["mean"], g["qvec"], g["scale"], g["opacity"], pts, kept)
        err = np.abs(out.astype(np.float64) - val)
        w = int(np.argmax(err / bound))
        mass = val > 1e-3
        # the largest single term of the sum: what the value changes by when that kept neighbour is dropped (>= value / K)
        terms = np.stack([DC.density64(g["mean"], g["qvec"], g["scale"], g["opacity"], pts, kept[:, k:k + 1])[0] for k in range(K)], 1)
        drop = terms.max(1)
        print(f"density {shape} K={K} skip={skip}: mass at {int(mass.sum())}/{val.size}; worst err/bound {err[w] / bound[w]:.4f} "
              f"(err {err[w]:.3e}); smallest drop / (allowance x bound) at mass {float((drop[mass] / (DENSITY_ALLOWANCE * bound[mass])).min()):.1f}")
        assert mass.sum() >= 1  # (the comparison is not one of zeros)
        assert (err <= DENSITY_ALLOWANCE * bound).all(), (shape, w, err[w], bound[w])
        assert (drop[mass] >= 10 * DENSITY_ALLOWANCE * bound[mass]).all()
        if skip:  # the other choice of skip is far outside the bound where there is mass
            other, _ = DC.density64(g["mean"], g["qvec"], g["scale"], g["opacity"], pts, DC.kept(qi, K, 0))
            assert (np.abs(out - other) > 10 * DENSITY_ALLOWANCE * bound).sum() >= 1


def test_query_search_at_K_16_replays_in_a_captured_graph():
    """test_gpu_knn_query's capture test at the list length it does not reach: captured on the uniform cloud, replayed on the planar
    one (same N) with other queries"""
    from gsgen_amd.knn import knn_raw
    a, b = KC.CLOUDS["uniform"], KC.CLOUDS["planar"]
    assert a.shape == b.shape
    qa, qb = KC.QUERIES["uniform"], KC.QUERIES["planar"]
    sp, sq = dev(a), dev(qa)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        knn_raw(sp, 16, query=sq)  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gd, gi = knn_raw(sp, 16, query=sq)
    sp.copy_(dev(b))
    sq.copy_(dev(qb))
    graph.replay()
    ed, ei = knn_raw(sp, 16, query=sq)
    torch.cuda.synchronize()
    assert torch.equal(gi, ei) and torch.equal(gd.view(torch.int32), ed.view(torch.int32))
    bd, bi = KC.brute_queries("planar")
    KC.same_bits(gd.cpu().numpy(), gi.cpu().numpy(), bd[:, :16], bi[:, :16], "replayed on planar")
