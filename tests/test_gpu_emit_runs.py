"""The push binning's emit pass -- a chunk's keys grouped by tile in LDS, stored in runs (gsgen_amd/csrc/binning.hip) -- on the GPU,
against the oracle's lists bit for bit: the shapes at which the staging can go wrong (tests/emit_runs.py).  The library takes the
push form from 32 (chunk, view) workgroups on in a batch and from 128 chunks on for a lone camera, so the small scenes are
batches of up to 32 views (three cameras, repeated) and the per-camera push form gets one scene of 129 chunks."""
import pytest

import emit_runs as E

pytestmark = pytest.mark.gpu

BATCH_PUSH, SINGLE_PUSH = 32, 128   # binning.hip: kPushMinWorkgroupsBatch, kPushMinWorkgroups


@pytest.fixture(scope="module")
def be():
    from gsgen_amd import _capi
    return E.GpuBackend(_capi.load())


@pytest.fixture(scope="module")
def capacity(be):
    cap = be.lib.emit_stage_capacity()
    assert cap >= 64 and cap % 64 == 0 and cap < 64 * E.CHUNK
    return cap


@pytest.mark.parametrize("N", E.SIZES)
@pytest.mark.parametrize("W,H", E.IMAGES)
def test_size_boundaries(be, W, H, N):
    E.case_sizes(be, W, H, N, BATCH_PUSH)


def test_mixed_rectangles(be):
    E.case_mixed(be, BATCH_PUSH)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_capacity_edge(be, capacity, delta):
    E.case_capacity(be, capacity + delta, BATCH_PUSH)


def test_far_beyond_capacity(be, capacity):
    """2 048 image-sized splats on a 128 x 128 image: 64 tiles x 2 048 keys in one chunk"""
    assert 64 * E.CHUNK >= 4 * capacity
    E.case_capacity(be, 64 * E.CHUNK, BATCH_PUSH)


def test_empty_view_in_a_batch(be):
    E.case_empty_view(be, 11 * E.CHUNK + 1)     # 12 chunks x 3 views: the push form


def test_single_view(be):
    E.case_single_view(be, SINGLE_PUSH * E.CHUNK + 1, single=True)   # 129 chunks: push form for B = 1 and for the per-camera call


def test_largest_tile_grid_with_lds_counters(be):
    """2 048 x 1 024 pixels are 8 192 tiles, the most the push form takes: counters and staging words fill the workgroup's LDS"""
    import scenes
    cam = scenes.Camera(2048, 1024, fx=1500.0, c2w=scenes.orbit(2.2, 20, 100))
    assert cam.tiles[0] * cam.tiles[1] == 8192
    sc = scenes.random_scene(4 * E.CHUNK + 1, seed=13, svec=0.03, spread=0.5)
    sc["svec"][::1000] *= 30.0
    g = scenes.oracle_geometry(sc, cam)
    E.run_batch(be, sc, [cam] * 7, [g] * 7)    # 5 chunks x 7 views


def test_overflow_writes_nothing(be):
    E.case_overflow(be, 2500, BATCH_PUSH)
