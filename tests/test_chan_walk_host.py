"""The designed tile lists of tests/chan_cases.py -- list lengths around the staging rounds, saturation at every place in a round,
unseen batches, the threshold guard, degenerate records, empty and partial tiles, the clamp -- through every launch form of the
post-activation channel kernels on the CPU host build (`emu`), against the fp64 reference.  Without a GPU this proves that the
cases, their margins and the bars are satisfiable by the kernels' arithmetic; the same checks run on the device in
tests/test_gpu_chan_walk.py.

Worst ratio of scenes.per_gaussian_grad_error(rtol 1e-3, atol 1e-5) over every tensor and launch form, CPU host build (<= 1
passes): len_1 .. len_200 0.004 .. 0.031 (corner tile 0.002 .. 0.029), sat_last_of_batch 0.156, sat_first_of_next 0.086,
sat_in_first_batch 0.154, sat_partial 0.067, unseen_batch 0.016, guard_trip 0.002, bad_records 0.008, empty_tiles 0.002,
clamp_straddle 0.037; the oracle's fp32 chain on the same lists: 0.018 at most.  behind_opaque: 2.79 (the alpha gradient of the
near-opaque layers, moment form with z_var; the oracle's chain 0.010) -- held instead to |got - ref| <= 1e-3 max |ref| + FUZZ_ATOL
per tensor, of which it uses 0.062 ("The single suffix behind near-opaque layers")."""
import os
import subprocess

import pytest

import chan_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "emu"])
    from gsgen_amd import _capi
    return CC.HostArrays(_capi.Lib(os.path.join(ROOT, "oracle", "_build", "libgsgen_emu.so")))


@pytest.mark.parametrize("name", list(CC.CASES))
def test_emulated_chan_walk_case(emu, name):
    CC.check_case(emu, name)
