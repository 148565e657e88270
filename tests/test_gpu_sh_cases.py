"""The designed tile lists of tests/sh_cases.py through the SH entry points on the device, against the fp64 reference: the checks of
tests/test_sh_cases_host.py, where v_rcp_f32 and the hardware exponential add their own ulp.  Every launch is 9 tiles x 2 views.

Worst ratio over every tensor, image and launch form against the exact reference (polynomial launches against the poly model) on
an MI355X (<= 1 passes): len_* 0.116 (0.043), sat_entry_* 0.150 (0.150), sat_in_first_round 0.055 (0.025), sat_partial 0.055
(0.058), unseen_round 0.116 (0.024), guard_trip 0.110 (0.019), non_psd 0.068 (0.025), clamp_straddle 0.034 (0.020), bad_records
0.116 (0.030), empty_tiles 0.110 (0.019), big_bands 0.061 (0.024), taylor_edge 0.069 (0.019), flagged_tile_7 0.092 (0.026),
flagged_tile_9 0.084 (0.024), C = 1..3 0.069.  0.116 is the polynomial basis itself: the sh gradient of the polynomial launches
against the EXACT reference, which the poly model reproduces on the references alone."""
import pytest

import sh_cases as SC


@pytest.fixture(scope="module")
def gpu():
    return SC.DeviceArrays()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SC.CASES))
def test_gpu_sh_case(gpu, name):
    SC.check_case(gpu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("name", SC.LOW_BAND_CASES)
def test_gpu_sh_case_low_bands(gpu, name, C):
    SC.check_case(gpu, name, C)
