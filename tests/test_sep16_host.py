"""The separable reduce-scatter of the polynomial SH backward on the CPU emulator (rows before columns: wave_reduce_scatter_sep16,
gsgen_amd/csrc/common.hpp): the helper alone, and the routed polynomial backward through it against the exact-basis backward of the
same inputs, both forms of the geometric gradients.  The GPU twin is tests/test_gpu_sep16.py; the checks are tests/sep16_chain.py."""
import os
import subprocess

import numpy as np
import pytest

import sep16_chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "emu"])
    from gsgen_amd import _capi
    return _capi.Lib(os.path.join(ROOT, "oracle", "_build", "libgsgen_emu.so"))


class HostArrays:
    """the emulator works on host memory: "device" arrays are numpy arrays"""

    class Arr:
        def __init__(self, a):
            self.a = np.ascontiguousarray(a).copy(); self.p = self.a.ctypes.data

        def get(self):
            return self.a

    def __init__(self, lib):
        self.lib, self.stream = lib, None

    def to_dev(self, a):
        return self.Arr(a)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_emulated_separable_reduce_scatter(emu, seed):
    sep16_chain.helper_check(HostArrays(emu), seed)


@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("shape", list(sep16_chain.SHAPES))
def test_emulated_routed_polynomial_backward_against_the_exact_basis(emu, shape, moments):
    sep16_chain.routed_poly_backward_vs_exact(HostArrays(emu), shape, moments)
