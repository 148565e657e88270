"""The kNN index and its three consumers (gsgen_amd/csrc/knn_index.hpp, knn.hip) on the CPU SIMT emulator at every list length,
size edge and degenerate cloud: the self and the query search over tests/knn_cases.py's clouds x K_MATRIX (every instantiation
L = 1 .. 32 and a K below each L > 1), the degenerate extents (one position, a line, N = 1, N = K, N < 64), a cloud of few
distinct positions, the scan at its tile boundary and in its second chunk of 256 tiles, and the density lattice at every list
length.  The searches against the fp32 brute force bit for bit; the lattice by test_knn_query_host's rule."""
import numpy as np
import pytest

import density_cases as DC
import knn_cases as KC
from test_knn_query_host import knn_emu, run_density, run_query, run_self  # noqa: F401  (knn_emu: the emulator build fixture)


@pytest.mark.parametrize("name", sorted(KC.CLOUDS))
def test_emulated_self_and_query_search_over_the_K_matrix(knn_emu, name):  # noqa: F811
    pts, qs = KC.CLOUDS[name], KC.QUERIES[name]
    (sd, si), (qd, qi) = KC.brute_self(name), KC.brute_queries(name)
    ran = 0
    for K in KC.K_MATRIX:
        if K > pts.shape[0]:
            continue
        d, i = run_self(knn_emu, pts, K)
        KC.same_bits(d, i, sd[:, :K], si[:, :K], f"{name} self K={K}")
        d, i = run_query(knn_emu, pts, qs, K)
        KC.same_bits(d, i, qd[:, :K], qi[:, :K], f"{name} query K={K}")
        ran += 1
    assert ran == (len(KC.K_MATRIX) if pts.shape[0] >= 32 else sum(K <= pts.shape[0] for K in KC.K_MATRIX)) and ran >= 1


@pytest.mark.parametrize("name", KC.DEGENERATE)
def test_emulated_degenerate_clouds(knn_emu, name):  # noqa: F811
    pts, qs = KC.CLOUDS[name], KC.QUERIES[name]
    K = min(4, pts.shape[0])
    d, i = run_self(knn_emu, pts, K)
    bd, bi = KC.brute(pts, K)
    KC.same_bits(d, i, bd, bi, f"{name} self")
    assert (i >= 0).all() and np.isfinite(d).all()  # (N >= K finite points: no padded entry)
    d, i = run_query(knn_emu, pts, qs, K)
    bd, bi = DC.brute_query(pts, qs, K)
    KC.same_bits(d, i, bd, bi, f"{name} query")
    assert (i >= 0).all() and np.isfinite(d).all()
    if name == "same":  # forty copies of one point: the four lowest indices, whoever asks
        assert (i == np.arange(4)).all() and (run_self(knn_emu, pts, 4)[1] == np.arange(4)).all()


@pytest.mark.parametrize("K", KC.K_MATRIX)
def test_emulated_cloud_of_exactly_K_points(knn_emu, K):  # noqa: F811
    pts = KC.n_eq_k(K)
    d, i = run_self(knn_emu, pts, K)
    bd, bi = KC.brute(pts, K)
    KC.same_bits(d, i, bd, bi, f"N = K = {K} self")
    assert (np.sort(i, axis=1) == np.arange(K)).all()  # every row lists the whole cloud
    qs = KC.queries_for(pts, 64, seed=K)
    d, i = run_query(knn_emu, pts, qs, K)
    bd, bi = DC.brute_query(pts, qs, K)
    KC.same_bits(d, i, bd, bi, f"N = K = {K} query")


@pytest.mark.parametrize("K", [4, 16])
def test_emulated_few_distinct_positions_are_decided_by_the_index(knn_emu, K):  # noqa: F811
    pts = KC.CLOUDS["few_distinct"]
    _, inv, cnt = np.unique(pts, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    assert cnt.size == 50 and cnt.min() > K  # every tie set is larger than K
    d, i = run_self(knn_emu, pts, K)
    KC.same_bits(d, i, KC.brute_self("few_distinct")[0][:, :K], KC.brute_self("few_distinct")[1][:, :K], "few_distinct self")
    lowest = np.stack([np.nonzero(inv == g)[0][:K] for g in range(50)])  # the K lowest indices at each position
    np.testing.assert_array_equal(i, lowest[inv])
    assert (d == 0).all()
    d, i = run_query(knn_emu, pts, pts[:300] + np.float32(0), K)  # (queries on top of the positions)
    np.testing.assert_array_equal(i, lowest[inv[:300]])


@pytest.mark.parametrize("N", KC.SCAN_SMALL)
def test_emulated_scan_at_the_tile_boundary(knn_emu, N):  # noqa: F811
    """K = 2: cap = N / 2 cells, cap + 3 scanned entries = 1024 (one full tile) and 1025 (a second tile of one entry)"""
    assert N // 2 + 3 in (1024, 1025)
    pts = KC.scan_cloud(N)
    d, i = run_self(knn_emu, pts, 2)
    bd, bi = KC.brute(pts, 2)
    KC.same_bits(d, i, bd, bi, f"N = {N}")


def test_emulated_scan_carries_into_a_second_chunk_of_tiles(knn_emu):  # noqa: F811
    """N = 524 328, K = 2: cap + 3 = 262 167 entries = 257 scan tiles, so k_knn_scan_sums takes its second chunk of 256 with the carry
    of the first, and the bbox / histogram kernels (256 blocks of 256 threads at most) take nine grid-stride iterations"""
    N = KC.SCAN_LARGE
    assert (N // 2 + 3 + 1023) // 1024 == 257
    pts = KC.scan_cloud(N)
    assert KC.no_exact_duplicates(pts)  # no exact duplicates: every point is its own first neighbour
    d, i = run_self(knn_emu, pts, 2)
    KC.check_whole_array(pts, d, i)
    rows = np.random.default_rng(7).choice(N, 300, replace=False)
    bd, bi = KC.brute_rows(pts, rows, 2)
    KC.same_bits(d[rows], i[rows], bd, bi, f"N = {N}, 300 rows")


@pytest.fixture(scope="module")
def golden_scene():
    z = DC.load_golden()
    return {k: z[k] for k in ("mean", "qvec", "scale", "opacity")}


@pytest.mark.parametrize("shape", KC.DENSITY_SHAPES)
@pytest.mark.parametrize("K,skip", KC.DENSITY_KS)
def test_emulated_density_grid_at_every_list_length(knn_emu, golden_scene, shape, K, skip):  # noqa: F811
    """the rule of test_emulated_density_grid_against_its_neighbours_and_fp64: the kept neighbours are the brute force's, the value
    lies within density_cases.density64's bound of the fp64 sum"""
    g = golden_scene
    ax, ay, az = KC.density_axes(g, shape)
    pts = DC.lattice(ax, ay, az)
    out = run_density(knn_emu, g, ax, ay, az, K, skip)
    assert out.shape == shape
    out = out.reshape(-1)
    _, qi = run_query(knn_emu, g["mean"], pts, K + skip)
    _, bi = DC.brute_query(g["mean"], pts, K + skip)
    np.testing.assert_array_equal(qi, bi)
    val, bound = DC.density64(g["mean"], g["qvec"], g["scale"], g["opacity"], pts, DC.kept(qi, K, skip))
    err = np.abs(out.astype(np.float64) - val)
    w = int(np.argmax(err / bound))
    print(f"{shape} K={K} skip={skip}: mass at {int((val > 1e-3).sum())}/{val.size}, max value {val.max():.3e}; worst err/bound "
          f"{err[w] / bound[w]:.3f} (err {err[w]:.3e})")
    assert (val > 1e-3).sum() >= 1  # (the comparison is not one of zeros)
    assert (err <= bound).all(), (w, err[w], bound[w])
    if skip:  # the other choice of skip is far outside the bound where there is mass
        other, _ = DC.density64(g["mean"], g["qvec"], g["scale"], g["opacity"], pts, DC.kept(qi, K, 0))
        assert (np.abs(out - other) > bound).sum() >= 1
