"""The projection backward on the device, each batched form at its edges: the cases of tests/proj_bwd_cases.py (the same inputs, the same
fp64 autograd reference and the same per-entry bounds that tests/test_proj_bwd_host.py runs on the emulator) through the C ABI on
device tensors.  The RGB + heads moment form also takes the records gsgen_frame_geometry_batch leaves in gsgen_geometry_view::chol for
the same scene and cameras, which must equal common.hpp:chol_prep restated in NumPy bit for bit."""
import numpy as np
import pytest
import torch

import proj_bwd_cases as P
from test_gpu_step_kernels import GpuBackend, dev

pytestmark = pytest.mark.gpu
IDS = [f"B{b}-N{n}" for b, n in P.SHAPES]
W, H = 64, 48


@pytest.fixture(scope="module")
def gpu():
    return GpuBackend()


def device_records(gpu):
    """-> callable(case) -> (handles of the views' chol records [N,4] as the batched projection launch left them, frustum masks)"""
    from gsgen_amd import _capi, renderer as R

    def make(case):
        B, N = case["B"], case["N"]
        lib, p = gpu.lib, gpu.ptr
        mean, qvec, svec = (gpu.put(case[k]) for k in ("mean", "qvec", "svec"))
        ci = R.CameraInfo(float(W), float(W), W / 2.0, H / 2.0, W, H)
        cams = [gpu.put(ci.pack(c)) for c in case["c2w"]]
        nth, ntw = R.n_tiles(H, W)
        D_cap, T = 1 << 16, nth * ntw
        ws_bytes = lib.frame_workspace_bytes(N, D_cap, T)
        z = lambda shape, dt: gpu.put(np.zeros(shape, dt))  # noqa: E731
        bufs = [dict(mean2d=z((N, 2), np.float32), cov2d=z((N, 4), np.float32), depth=z(N, np.float32), mask=z(N, np.uint8),
                     ids=z(D_cap, np.int32), start=z(T, np.int32), end=z(T, np.int32), total=z(1, np.uint32), ws=z(ws_bytes, np.uint8),
                     chol=gpu.put(np.full((N, 4), 9.0, np.float32))) for _ in range(B)]
        arr = (_capi.GeometryView * B)()
        for a, b_, cd in zip(arr, bufs, cams):
            a.cam, a.mean2d, a.cov2d, a.depth, a.mask = p(cd), p(b_["mean2d"]), p(b_["cov2d"]), p(b_["depth"]), p(b_["mask"])
            a.gaussian_ids, a.start, a.end, a.total = p(b_["ids"]), p(b_["start"]), p(b_["end"]), p(b_["total"])
            a.workspace, a.workspace_bytes, a.D_cap = p(b_["ws"]), ws_bytes, D_cap
            a.chol = p(b_["chol"])
        bws = torch.empty(lib.frame_batch_workspace_bytes(B), device=dev(), dtype=torch.uint8)
        lib.frame_geometry_batch(B, arr, N, p(mean), p(qvec), p(svec), W, H, bws.data_ptr(), gpu.stream)
        torch.cuda.synchronize()
        masks = [gpu.get(b_["mask"]) for b_ in bufs]
        for v, b_ in enumerate(bufs):   # the launch's cov2d is the oracle's, bit for bit, where the Gaussian is in the frustum
            seen = masks[v].astype(bool)
            assert int(gpu.get(b_["total"])[0]) <= D_cap
            assert np.array_equal(P.bits(gpu.get(b_["cov2d"])[seen]), P.bits(case["cov2d"][v][seen]))
        return [b_["chol"] for b_ in bufs], masks
    return make


@pytest.mark.parametrize("B,N", P.SHAPES, ids=IDS)
def test_plain_form_against_fp64(gpu, B, N):
    fr = [P.plain_check(gpu, B, N, detach) for detach in (0, 1)]
    print(f"[proj bwd gpu] plain B={B} N={N}: worst fraction of the bound = {max(fr):.3f}")


def test_plain_form_with_isotropic_scales_on_a_third(gpu):
    fr = P.plain_check(gpu, 17, 130, 0, iso_third=True)
    print(f"[proj bwd gpu] plain, a third isotropic, B=17 N=130: worst fraction of the bound = {fr:.3f}")


@pytest.mark.parametrize("B,N", P.SHAPES, ids=IDS)
def test_heads_form_against_fp64(gpu, B, N):
    fr = [P.heads_check(gpu, B, N, detach) for detach in (0, 1)]
    print(f"[proj bwd gpu] heads B={B} N={N}: worst fraction of the bound = {max(f[0] for f in fr):.3f}, "
          f"of the colour bound = {max(f[1] for f in fr):.3f}")


@pytest.mark.parametrize("form", ["heads", "sh"])
@pytest.mark.parametrize("B,N", P.SHAPES, ids=IDS)
def test_moment_forms_against_fp64(gpu, B, N, form):
    records = device_records(gpu) if form == "heads" else None
    for detach in (0, 1):
        fr = P.moments_check(gpu, B, N, form, detach, device_chol=records)
        print(f"[proj bwd gpu] {form} moments B={B} N={N} detach_depth={detach}: worst fraction of the bound = {fr['g']:.3f}, of the "
              f"in-place d mean2d bound = {fr['m2d']:.3f}, of the statistics bound = {fr['stat']:.3f}"
              + (f", of the colour bound = {fr['colour']:.3f}" if form == "heads" else "")
              + f"; median EPS (B + K + 8 kappa) = {fr['median_factor']:.2e}")


def test_empty_batch_zero_fills(gpu):
    P.empty_batch_check(gpu)


@pytest.mark.parametrize("N", [1, 63, 257])
def test_single_view_forms_against_fp64(gpu, N):
    fr = [P.single_view_check(gpu, N, detach) for detach in (0, 1)]
    print(f"[proj bwd gpu] single view N={N}: worst fraction of the bound = {max(fr):.3f}")


def test_bad_arguments_return_einval(gpu):
    n = P.bad_arguments_check(gpu)
    print(f"[proj bwd gpu] {n} malformed calls refused before any launch")
