"""The push binning's emit pass -- a chunk's keys grouped by tile in LDS, stored in runs (gsgen_amd/csrc/binning.hip) -- on the CPU
emulator, against the oracle's lists bit for bit: the shapes at which the staging can go wrong (tests/emit_runs.py).  The
emulator build reads GSGEN_BIN_PUSH_MIN_WORKGROUPS at every call: 1 sends every call, per camera and batched, through the push form."""
import ctypes
import os
import subprocess

import pytest

import emit_runs as E

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def be():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "emu"])
    from gsgen_amd import _capi
    before = os.environ.get("GSGEN_BIN_PUSH_MIN_WORKGROUPS")
    os.environ["GSGEN_BIN_PUSH_MIN_WORKGROUPS"] = "1"
    yield E.HostBackend(_capi.Lib(os.path.join(ROOT, "oracle", "_build", "libgsgen_emu.so")))
    if before is None:
        del os.environ["GSGEN_BIN_PUSH_MIN_WORKGROUPS"]
    else:
        os.environ["GSGEN_BIN_PUSH_MIN_WORKGROUPS"] = before


@pytest.fixture(scope="module")
def capacity(be):
    cap = be.lib.emit_stage_capacity()
    assert cap >= 64 and cap % 64 == 0 and cap < 64 * E.CHUNK   # (the capacity cases below build K from 64-tile splats)
    return cap


@pytest.mark.parametrize("N", E.SIZES)
@pytest.mark.parametrize("W,H", E.IMAGES)
def test_size_boundaries(be, W, H, N):
    E.case_sizes(be, W, H, N, 1)


def test_mixed_rectangles(be):
    E.case_mixed(be, 1)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_capacity_edge(be, capacity, delta):
    E.case_capacity(be, capacity + delta, 1)


@pytest.mark.parametrize("which", ["single", "batch"])
def test_far_beyond_capacity(be, capacity, which):
    """2 048 image-sized splats on a 128 x 128 image: 64 tiles x 2 048 keys in one chunk"""
    assert 64 * E.CHUNK >= 4 * capacity
    E.case_capacity(be, 64 * E.CHUNK, 1, which=(which,))


def test_empty_view_in_a_batch(be):
    E.case_empty_view(be, 2500)


def test_single_view_batch(be):
    E.case_single_view(be, 4500, single=True)


def test_overflow_writes_nothing(be):
    E.case_overflow(be, 2500, 1)


@pytest.mark.parametrize("K", ["capacity - 1", "capacity", "capacity + 1", "64 * 2048", "mixed"])
def test_keys_really_go_through_the_staging_array(be, capacity, K):
    """the lists are the same whether a key was staged or stored directly, so a build that quietly staged nothing would pass
    every comparison above: the emulator build tallies the keys its flush loops store (gsgen_emu_emit_staged_keys), and the
    tally is what the oracle's rectangles say -- all of a chunk's keys up to the capacity, the leading tiles that fit beyond"""
    import scenes
    tally = ctypes.c_ulonglong.in_dll(be.lib.cdll, "gsgen_emu_emit_staged_keys")
    if K == "mixed":
        cam = E.front_camera(200, 120)
        sc = E.cover_scene(cam, 1, list(range(104)) * 5, seed=5)
    else:
        cam = E.front_camera(128, 128)
        sc = E.capacity_scene(cam, eval(K, {"capacity": capacity}))
    N = sc["mean"].shape[0]
    g = scenes.oracle_geometry(sc, cam)
    want = E.expected_staged_keys(g, N, cam, capacity)
    assert want == {"capacity - 1": capacity - 1, "capacity": capacity, "64 * 2048": capacity // E.CHUNK * E.CHUNK}.get(K, want)
    assert 0 < want <= capacity
    before = tally.value
    E.run_batch(be, sc, [cam], [g])
    assert tally.value - before == want
    E.run_batch(be, sc, [cam], [g], caps=[g["D"] - 1])      # an overflowing frame stages nothing
    assert tally.value - before == want
