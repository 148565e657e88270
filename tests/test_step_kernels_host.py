"""The cases of tests/step_cases.py -- the fused Adam step, the SH coefficient bounds, the densify / prune statistics -- on the CPU
emulator: without a GPU this proves that the cases and their derived bounds are satisfiable by the kernels' arithmetic.  The same
cases run on the device in tests/test_gpu_step_kernels.py."""
import os
import subprocess

import pytest

import step_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "emu"])
    from gsgen_amd import _capi
    return S.HostBackend(_capi.Lib(os.path.join(ROOT, "oracle", "_build", "libgsgen_emu.so")))


@pytest.mark.parametrize("n,ends", S.ADAM_CASES, ids=[f"n{n}" for n, _ in S.ADAM_CASES])
def test_emulated_adam_step_within_rounding_bounds(emu, n, ends):
    worst, moved = [0.0, 0.0, 0.0], float("inf")
    for step in S.ADAM_STEPS:
        fr, mv = S.adam_check(emu, n, ends, step)
        worst, moved = [max(a, b) for a, b in zip(worst, fr)], min(moved, mv)
    print(f"[adam emu] n={n}: worst fraction of tol_p / tol_m / tol_v = {worst[0]:.3f} / {worst[1]:.3f} / {worst[2]:.3f}; "
          f"a boundary moved by one leaves tol_p by a factor >= {moved:.3g}")


@pytest.mark.parametrize("N,C,skew", S.SH_CASES, ids=[f"N{N}-C{C}-{'skew4' if k else 'aligned'}" for N, C, k in S.SH_CASES])
def test_emulated_sh_bounds_against_fp64(emu, N, C, skew):
    frac = S.sh_check(emu, N, C, skew)
    print(f"[sh bound emu] N={N} C={C} base%16={4 * skew}: worst fraction of C^2 E rows64 = {frac:.3f}")


@pytest.mark.parametrize("null_view", [True, False])
@pytest.mark.parametrize("n_views", S.DENSIFY_VIEWS)
@pytest.mark.parametrize("N", S.DENSIFY_NS)
def test_emulated_densify_statistics_against_the_oracle(emu, N, n_views, null_view):
    frac = S.densify_check(emu, N, n_views, null_view)
    print(f"[densify emu] N={N} views={n_views} null_view={null_view}: worst fraction of the grad_accum bound = {frac:.3f}")
