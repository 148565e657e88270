"""The separable reduce-scatter of the polynomial SH backward on the GPU (-m gpu): the helper alone (v_permlane swaps + DPP), and the
routed polynomial backward through it against the exact-basis backward of the same inputs, both forms of the geometric gradients.  The
emulator twin is tests/test_sep16_host.py; the checks are tests/sep16_chain.py."""
import numpy as np
import pytest
import torch

import sep16_chain

pytestmark = pytest.mark.gpu


class DeviceArrays:
    class Arr:
        def __init__(self, a):
            self.t = torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0"); self.p = self.t.data_ptr()

        def get(self):
            return self.t.cpu().numpy()

    def __init__(self):
        from gsgen_amd import _capi
        self.lib, self.stream = _capi.load(), torch.cuda.current_stream().cuda_stream

    def to_dev(self, a):
        return self.Arr(a)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_separable_reduce_scatter(seed):
    sep16_chain.helper_check(DeviceArrays(), seed, sync=torch.cuda.synchronize)


@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("shape", list(sep16_chain.SHAPES))
def test_routed_polynomial_backward_against_the_exact_basis(shape, moments):
    sep16_chain.routed_poly_backward_vs_exact(DeviceArrays(), shape, moments, sync=torch.cuda.synchronize)
