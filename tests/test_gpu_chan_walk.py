"""The designed tile lists of tests/chan_cases.py through every launch form of the post-activation channel kernels on the device,
against the fp64 reference: the checks of tests/test_chan_walk_host.py, where v_rcp_f32 and the hardware exponential add their own
ulp.  Every launch is 9 tiles x 2 views; the file takes about four seconds.

Worst ratio of scenes.per_gaussian_grad_error(rtol 1e-3, atol 1e-5) over every tensor and launch form on an MI355X (<= 1 passes):
len_1 .. len_200 0.003 .. 0.029 (corner tile 0.003 .. 0.032), sat_last_of_batch 0.120, sat_first_of_next 0.076, sat_in_first_batch
0.203, sat_partial 0.069, unseen_batch 0.017, guard_trip 0.003, bad_records 0.004, empty_tiles 0.003, clamp_straddle 0.026.
behind_opaque: 2.54 (the alpha gradient of the near-opaque layers, plain form with z_var; moment form 2.12; the oracle's fp32 chain
0.010) -- held instead to |got - ref| <= 1e-3 max |ref| + FUZZ_ATOL per tensor, of which it uses 0.057."""
import pytest

import chan_cases as CC


@pytest.fixture(scope="module")
def gpu():
    return CC.DeviceArrays()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CC.CASES))
def test_gpu_chan_walk_case(gpu, name):
    CC.check_case(gpu, name)
