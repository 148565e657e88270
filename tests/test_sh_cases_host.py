"""The designed tile lists of tests/sh_cases.py -- list lengths around the staging rounds of 32 and 64, saturation at every place in
a round and a segment, unseen rounds, the threshold guard, indefinite covariances, dropped records, empty and partial tiles, the
clamp, large higher bands, tiles crowded with splats beyond the coefficient bound -- through the SH entry points on the CPU host
build (`emu`), against the fp64 reference.  Without a GPU this proves that the cases, their margins and the bars are satisfiable by
the kernels' arithmetic; the same checks run on the device in tests/test_gpu_sh_cases.py.

Worst ratio over every tensor, image and launch form against the exact reference (polynomial launches against the poly model), CPU
host build (<= 1 passes; the oracle's fp32 chain on the same lists 0.089 at most): len_* 0.116 (0.041), sat_entry_* 0.118 (0.113),
sat_in_first_round 0.058 (0.057), sat_partial 0.067 (0.070), unseen_round 0.116 (0.024), guard_trip 0.109 (0.019), non_psd 0.068
(0.025), clamp_straddle 0.034 (0.020), bad_records 0.116 (0.028), empty_tiles 0.109 (0.018), big_bands 0.061 (0.024), taylor_edge
0.068 (0.019), flagged_tile_7 0.092 (0.026), flagged_tile_9 0.084 (0.024), C = 1..3 0.064.  0.116 is the polynomial basis itself:
the sh gradient of the polynomial launches against the EXACT reference, which the poly model reproduces on the references alone."""
import os
import subprocess

import pytest

import sh_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "emu"])
    from gsgen_amd import _capi
    return SC.HostArrays(_capi.Lib(os.path.join(ROOT, "oracle", "_build", "libgsgen_emu.so")))


@pytest.mark.parametrize("name", list(SC.CASES))
def test_emulated_sh_case(emu, name):
    SC.check_case(emu, name)


@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("name", SC.LOW_BAND_CASES)
def test_emulated_sh_case_low_bands(emu, name, C):
    SC.check_case(emu, name, C)
