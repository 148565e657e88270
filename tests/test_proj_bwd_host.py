"""The cases of tests/proj_bwd_cases.py -- every batched form of the projection backward and its single-view forms against the fp64
autograd reference at per-entry rounding bounds -- on the CPU emulator: without a GPU this proves that the cases and their derived
bounds are satisfiable by the kernel's arithmetic (the lane split, the LDS exchange, the accumulating launches all run as written).
The same cases run on the device in tests/test_gpu_proj_bwd.py."""
import os
import subprocess

import pytest

import proj_bwd_cases as P
import step_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [f"B{b}-N{n}" for b, n in P.SHAPES]


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "emu"])
    from gsgen_amd import _capi
    return S.HostBackend(_capi.Lib(os.path.join(ROOT, "oracle", "_build", "libgsgen_emu.so")))


@pytest.mark.parametrize("B,N", P.SHAPES, ids=IDS)
def test_emulated_plain_form_against_fp64(emu, B, N):
    fr = [P.plain_check(emu, B, N, detach) for detach in (0, 1)]
    print(f"[proj bwd emu] plain B={B} N={N}: worst fraction of the bound = {max(fr):.3f}")


def test_emulated_plain_form_with_isotropic_scales_on_a_third(emu):
    fr = P.plain_check(emu, 17, 130, 0, iso_third=True)
    print(f"[proj bwd emu] plain, a third isotropic, B=17 N=130: worst fraction of the bound = {fr:.3f}")


@pytest.mark.parametrize("B,N", P.SHAPES, ids=IDS)
def test_emulated_heads_form_against_fp64(emu, B, N):
    fr = [P.heads_check(emu, B, N, detach) for detach in (0, 1)]
    print(f"[proj bwd emu] heads B={B} N={N}: worst fraction of the bound = {max(f[0] for f in fr):.3f}, "
          f"of the colour bound = {max(f[1] for f in fr):.3f}")


@pytest.mark.parametrize("form", ["heads", "sh"])
@pytest.mark.parametrize("B,N", P.SHAPES, ids=IDS)
def test_emulated_moment_forms_against_fp64(emu, B, N, form):
    for detach in (0, 1):
        fr = P.moments_check(emu, B, N, form, detach)
        print(f"[proj bwd emu] {form} moments B={B} N={N} detach_depth={detach}: worst fraction of the bound = {fr['g']:.3f}, of the "
              f"in-place d mean2d bound = {fr['m2d']:.3f}, of the statistics bound = {fr['stat']:.3f}"
              + (f", of the colour bound = {fr['colour']:.3f}" if form == "heads" else "")
              + f"; median EPS (B + K + 8 kappa) = {fr['median_factor']:.2e}")


def test_emulated_empty_batch_zero_fills(emu):
    P.empty_batch_check(emu)


@pytest.mark.parametrize("N", [1, 63, 257])
def test_emulated_single_view_forms_against_fp64(emu, N):
    fr = [P.single_view_check(emu, N, detach) for detach in (0, 1)]
    print(f"[proj bwd emu] single view N={N}: worst fraction of the bound = {max(fr):.3f}")


def test_emulated_bad_arguments_return_einval(emu):
    n = P.bad_arguments_check(emu)
    print(f"[proj bwd emu] {n} malformed calls refused before any launch")
