// depth_loss.hip -- the Pearson depth loss of the image-conditioned training step and its gradients, for gfx950 (compiled with
// -ffp-contract=off).
//
// Replaces utils/loss.py:50-66 of the reference (trainer.py:424-440, :659-689),
//   loss = (1 / B) sum_b (1 - torchmetrics.PearsonCorrCoef()(nan_to_num(pred_b)[m_b], gt_b[m_b])),
// a Python loop over the batch with a boolean-mask gather (a host synchronisation and a data-dependent shape) per image.
// DESIGN.md ("Depth loss") has the definition; in short, per image b of P pixels, over the pixels with m_i true (n of them):
//   x_i = nan_to_num(pred_i) (NaN -> 0, +-Inf -> +-FLT_MAX),  y_i = gt_i,  xm = sum x / n,  ym = sum y / n,
//   Sxx = sum (x - xm)^2,  Syy = sum (y - ym)^2,  Sxy = sum (x - xm)(y - ym),  r = clamp(Sxy / sqrt(Sxx Syy), -1, 1),
//   d loss / d x_i = -(g / B) ((y_i - ym) / sqrt(Sxx Syy) - r (x_i - xm) / Sxx)   (and x <-> y for d loss / d y_i)
// zero outside the mask, where pred_i was not finite (pred only), and where the clamp is active (strictly outside [-1, 1]: the
// bounds pass the gradient, as torch.clamp does).  An image with n < 2, or whose masked x are all equal, or whose masked y are all
// equal, is DEGENERATE: torchmetrics returns 0 / 0 = NaN there; here it contributes 1 (r = 0) and a zero gradient, and its entry of
// the per-image correlations is NaN.  A NaN in gt under the mask is not sanitised: the loss is NaN.
//
// Kernels (a workgroup = kThreads = 256 threads owns one chunk of kChunk = 4096 consecutive pixels of one image; grid = chunks x B):
//   k_depth_fwd    reads pred, gt and mask once, 16 pixels per thread held in registers.  The chunk's moments are taken about a
//                  SHIFT, the values (Kx, Ky) of the chunk's first masked pixel: with d = x - Kx (exact in fp64 for fp32 inputs)
//                    mean = Kx + sum d / n,  M2 = sum d^2 - (sum d)^2 / n,  C = sum dx dy - sum dx sum dy / n
//                  in fp64, so the subtraction cancels digits of the spread about a value INSIDE the data, never of the offset (the
//                  fp32 form sum x^2 - (sum x)^2 / n is wrong in the second digit on a depth map at offset 100).  Beside them the
//                  exact minimum and maximum of x and of y (NaN-propagating): "all equal" is min == max, decided exactly and not by
//                  comparing a rounded variance with zero.  Wave shuffles, then the waves in order; one partial of ten doubles
//                  {n, xm, ym, M2x, M2y, C, xmin, xmax, ymin, ymax} per workgroup goes to the workspace.
//   k_depth_final  one workgroup; a wave per image merges that image's partials in a fixed order with the pairwise update
//                    n = na + nb, d = mb - ma, m = ma + d nb / n, M2 = M2a + M2b + d^2 na nb / n, C = Ca + Cb + dx dy na nb / n
//                  -> r, loss_out[1 + b] = r (NaN: degenerate) and the per-image moments {xm, ym, 1 / sqrt(Sxx Syy), r / Sxx, r / Syy,
//                  live} saved in the workspace for the backward; then the waves' sums of (1 - r) in order -> loss_out[0].
//   k_depth_bwd    one elementwise pass over pred, gt and mask with the saved moments, in fp64 per pixel, one rounding to fp32.
//                  The upstream scalar is read from device memory: no host synchronisation, and a captured replay sees its new value.
// Two pixels need no special case: with the shift on the first of them every sum above has one rounding, the same as the centred
// two-pass form's.  No float atomics, no fill: the workspace may arrive dirty and unaligned (every word read was written by the
// launch before).  Loss and gradients are bit-identical from run to run.  Launch shapes depend on B and P alone.
//
// -ffp-contract=off: nothing is fused, so the g++ build of this file on the CPU emulator (tests/test_depth_loss_host.py) performs
// the GPU's operations in the GPU's order.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsgen_hip.h"

namespace gs_depth {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPer = 16;                    // pixels of a chunk one thread holds
constexpr int kChunk = kThreads * kPer;     // pixels of one image a workgroup reduces
constexpr int kPartial = 10, kMoments = 6;  // doubles per workgroup partial / per image for the backward

// torch.nan_to_num in fp32
__device__ __forceinline__ float sanitize(float v) { return v != v ? 0.0f : (v > FLT_MAX ? FLT_MAX : (v < -FLT_MAX ? -FLT_MAX : v)); }
__device__ __forceinline__ bool is_finite(float v) { return fabsf(v) <= FLT_MAX; }  // (false for a NaN)
// a NaN on either side stays: min == max is then false and the NaN reaches the loss through the sums
__device__ __forceinline__ double nan_min(double a, double b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

__device__ __forceinline__ double wave_sum(double v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

struct Part { double n, xm, ym, m2x, m2y, c, xmin, xmax, ymin, ymax; };

__device__ __forceinline__ Part empty_part() { return Part{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, (double)INFINITY, -(double)INFINITY, (double)INFINITY, -(double)INFINITY}; }

__device__ __forceinline__ Part load_part(const double *p) { return Part{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9]}; }

// a, then b (no branch: it is called between wave shuffles)
__device__ __forceinline__ Part merge(const Part &a, const Part &b) {
  const double n = a.n + b.n, inv = n > 0.0 ? 1.0 / n : 0.0;
  const double dx = b.xm - a.xm, dy = b.ym - a.ym, w = a.n * b.n * inv, fb = b.n * inv;
  Part r;
  r.n = n;
  r.xm = a.xm + dx * fb;
  r.ym = a.ym + dy * fb;
  r.m2x = a.m2x + b.m2x + (dx * dx) * w;
  r.m2y = a.m2y + b.m2y + (dy * dy) * w;
  r.c = a.c + b.c + (dx * dy) * w;
  if (a.n == 0.0) { r.xm = b.xm; r.ym = b.ym; r.m2x = b.m2x; r.m2y = b.m2y; r.c = b.c; }  // (an empty side has no mean: keep the other's bits)
  if (b.n == 0.0) { r.xm = a.xm; r.ym = a.ym; r.m2x = a.m2x; r.m2y = a.m2y; r.c = a.c; }
  r.xmin = nan_min(a.xmin, b.xmin); r.xmax = nan_max(a.xmax, b.xmax);
  r.ymin = nan_min(a.ymin, b.ymin); r.ymax = nan_max(a.ymax, b.ymax);
  return r;
}

__device__ __forceinline__ Part shfl_down_part(const Part &p, int d) {
  return Part{__shfl_down(p.n, d), __shfl_down(p.xm, d), __shfl_down(p.ym, d), __shfl_down(p.m2x, d), __shfl_down(p.m2y, d),
              __shfl_down(p.c, d), __shfl_down(p.xmin, d), __shfl_down(p.xmax, d), __shfl_down(p.ymin, d), __shfl_down(p.ymax, d)};
}

__global__ void __launch_bounds__(kThreads) k_depth_fwd(const float *__restrict__ pred, const float *__restrict__ gt, size_t gt_stride,
                                                         const uint8_t *__restrict__ mask, size_t mask_stride, uint32_t P,
                                                         double *__restrict__ partials) {
  __shared__ int sFirst[kWaves];
  __shared__ double sRed[kWaves][kPartial];
  const int t = threadIdx.x;
  const uint32_t b = blockIdx.y;
  const size_t c0 = (size_t)blockIdx.x * kChunk;
  const float *px = pred + (size_t)b * P, *py = gt + (size_t)b * gt_stride;
  const uint8_t *pm = mask ? mask + (size_t)b * mask_stride : nullptr;

  float x[kPer], y[kPer];
  uint32_t live = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const size_t i = c0 + (size_t)(j * kThreads + t);
    const bool in = i < (size_t)P;
    x[j] = sanitize(in ? px[i] : 0.0f);
    y[j] = in ? py[i] : 0.0f;
    if (in && (pm ? pm[i] != 0 : true)) live |= 1u << j;
  }
  // the shift: the chunk's first masked pixel (in the order j * kThreads + t), read again by every thread (one address: a broadcast)
  int first = live ? (__ffsll((long long)live) - 1) * kThreads + t : kChunk;
  for (int d = 32; d > 0; d >>= 1) first = min(first, __shfl_xor(first, d));
  if ((t & 63) == 0) sFirst[t >> 6] = first;
  __syncthreads();
  first = sFirst[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) first = min(first, sFirst[w]);
  double Kx = 0.0, Ky = 0.0;
  if (first < kChunk) { Kx = (double)sanitize(px[c0 + first]); Ky = (double)py[c0 + first]; }

  double sdx = 0.0, sdy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
  double xmin = (double)INFINITY, xmax = -(double)INFINITY, ymin = (double)INFINITY, ymax = -(double)INFINITY;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    if (live >> j & 1u) {
      const double vx = (double)x[j], vy = (double)y[j], dx = vx - Kx, dy = vy - Ky;
      sdx += dx; sdy += dy;
      sxx += dx * dx; syy += dy * dy; sxy += dx * dy;
      xmin = nan_min(xmin, vx); xmax = nan_max(xmax, vx);
      ymin = nan_min(ymin, vy); ymax = nan_max(ymax, vy);
    }
  }
  double n = (double)__popcll((unsigned long long)live);
  n = wave_sum(n);
  sdx = wave_sum(sdx); sdy = wave_sum(sdy);
  sxx = wave_sum(sxx); syy = wave_sum(syy); sxy = wave_sum(sxy);
  for (int d = 32; d > 0; d >>= 1) {
    xmin = nan_min(xmin, __shfl_xor(xmin, d)); xmax = nan_max(xmax, __shfl_xor(xmax, d));
    ymin = nan_min(ymin, __shfl_xor(ymin, d)); ymax = nan_max(ymax, __shfl_xor(ymax, d));
  }
  if ((t & 63) == 0) {
    double *r = sRed[t >> 6];
    r[0] = n; r[1] = sdx; r[2] = sdy; r[3] = sxx; r[4] = syy; r[5] = sxy; r[6] = xmin; r[7] = xmax; r[8] = ymin; r[9] = ymax;
  }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < kWaves; ++w) {
      const double *r = sRed[w];
      n += r[0]; sdx += r[1]; sdy += r[2]; sxx += r[3]; syy += r[4]; sxy += r[5];
      xmin = nan_min(xmin, r[6]); xmax = nan_max(xmax, r[7]); ymin = nan_min(ymin, r[8]); ymax = nan_max(ymax, r[9]);
    }
    double *o = partials + (size_t)kPartial * ((size_t)b * gridDim.x + blockIdx.x);
    const double inv = n > 0.0 ? 1.0 / n : 0.0;
    const double m2x = sxx - sdx * sdx * inv, m2y = syy - sdy * sdy * inv;
    o[0] = n;
    o[1] = Kx + sdx * inv;
    o[2] = Ky + sdy * inv;
    o[3] = m2x < 0.0 ? 0.0 : m2x;  // (a rounding below zero; a NaN stays)
    o[4] = m2y < 0.0 ? 0.0 : m2y;
    o[5] = sxy - sdx * sdy * inv;
    o[6] = xmin; o[7] = xmax; o[8] = ymin; o[9] = ymax;
  }
}

__global__ void __launch_bounds__(kThreads) k_depth_final(const double *__restrict__ partials, uint32_t n_chunks, uint32_t B,
                                                           double *__restrict__ moments, float *__restrict__ loss_out) {
  __shared__ double sSum[kWaves];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double sum = 0.0;  // (lane 0: this wave's images, in order)
  for (uint32_t b = wave; b < B; b += kWaves) {
    const double *p = partials + (size_t)kPartial * (size_t)b * n_chunks;
    Part acc = empty_part();
    for (uint32_t c = lane; c < n_chunks; c += 64) acc = merge(acc, load_part(p + (size_t)kPartial * c));
    for (int d = 32; d > 0; d >>= 1) acc = merge(acc, shfl_down_part(acc, d));  // (lane 0 reads lanes below 2 d only: whole merges)
    if (lane == 0) {
      const bool degenerate = !(acc.n >= 2.0) || acc.xmin == acc.xmax || acc.ymin == acc.ymax;
      double *m = moments + (size_t)kMoments * b;
      if (degenerate) {
        for (int k = 0; k < kMoments; ++k) m[k] = 0.0;
        loss_out[1 + b] = __uint_as_float(0x7fc00000u);
        sum += 1.0;
      } else {
        const double inv = 1.0 / sqrt(acc.m2x * acc.m2y), raw = acc.c * inv;
        const double r = raw < -1.0 ? -1.0 : (raw > 1.0 ? 1.0 : raw);  // (a NaN stays a NaN)
        m[0] = acc.xm; m[1] = acc.ym; m[2] = inv; m[3] = r / acc.m2x; m[4] = r / acc.m2y;
        m[5] = (raw < -1.0 || raw > 1.0) ? 0.0 : 1.0;  // (the clamp passes the gradient on its bounds)
        loss_out[1 + b] = (float)r;
        sum += 1.0 - r;
      }
    }
  }
  if (lane == 0) sSum[wave] = sum;
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < kWaves; ++w) sum += sSum[w];
    loss_out[0] = (float)(sum / (double)B);
  }
}

__global__ void __launch_bounds__(kThreads) k_depth_bwd(const float *__restrict__ pred, const float *__restrict__ gt, size_t gt_stride,
                                                         const uint8_t *__restrict__ mask, size_t mask_stride, uint32_t P, double inv_B,
                                                         const double *__restrict__ moments, const float *__restrict__ grad_scale,
                                                         float *__restrict__ grad_pred, float *__restrict__ grad_gt) {
  const int t = threadIdx.x;
  const uint32_t b = blockIdx.y;
  const size_t c0 = (size_t)blockIdx.x * kChunk;
  const float *px = pred + (size_t)b * P, *py = gt + (size_t)b * gt_stride;
  const uint8_t *pm = mask ? mask + (size_t)b * mask_stride : nullptr;
  const double *m = moments + (size_t)kMoments * b;
  const double xm = m[0], ym = m[1], inv = m[2], rox = m[3], roy = m[4];
  const bool live = m[5] != 0.0;
  const double k = -(double)grad_scale[0] * inv_B;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const size_t i = c0 + (size_t)(j * kThreads + t);
    if (i < (size_t)P) {
      float gx = 0.0f, gy = 0.0f;
      if (live && (pm ? pm[i] != 0 : true)) {
        const float xr = px[i];
        const double dx = (double)sanitize(xr) - xm, dy = (double)py[i] - ym;
        gx = is_finite(xr) ? (float)(k * (dy * inv - dx * rox)) : 0.0f;  // (torch's nan_to_num passes no gradient where it replaced)
        gy = (float)(k * (dx * inv - dy * roy));
      }
      if (grad_pred) grad_pred[(size_t)b * P + i] = gx;
      if (grad_gt) grad_gt[(size_t)b * gt_stride + i] = gy;
    }
  }
}

// --- host side ---------------------------------------------------------------------------------------------------------
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct DepthWs {
  double *partials;  // [B][n_chunks][kPartial]
  double *moments;   // [B][kMoments]
  uint32_t n_chunks;
  size_t bytes;
};

inline DepthWs carve_depth(void *base, uint32_t B, uint32_t P) {
  char *p0 = (char *)base, *p = p0 + ((256 - ((uintptr_t)p0 & 255)) & 255);
  DepthWs w;
  w.n_chunks = (uint32_t)(((uint64_t)P + kChunk - 1) / kChunk);
  size_t off = 0;
  auto take = [&](size_t b) { char *r = p + off; off += align256(b); return r; };
  w.partials = (double *)take(sizeof(double) * kPartial * (size_t)B * w.n_chunks);
  w.moments = (double *)take(sizeof(double) * kMoments * (size_t)B);
  w.bytes = off + 256;
  return w;
}

}  // namespace gs_depth

using namespace gs_depth;

extern "C" {

size_t gsgen_depth_loss_workspace_bytes(uint32_t B, uint32_t n_pixels) {
  if (B > 65535u) return 0;  // (grid.y)
  return carve_depth(nullptr, B, n_pixels).bytes;
}

int gsgen_depth_loss_forward(const float *pred, const float *gt, size_t gt_image_stride, const uint8_t *mask, size_t mask_image_stride,
                             uint32_t B, uint32_t n_pixels, float *loss_out, void *workspace, size_t workspace_bytes,
                             gsgen_stream_t stream) {
  if (B > 65535u) return GSGEN_EUNSUPPORTED;
  if ((uint64_t)B * n_pixels == 0) return 0;
  if (!pred || !gt || !loss_out || !workspace) return GSGEN_EINVAL;
  const DepthWs w = carve_depth(workspace, B, n_pixels);
  if (w.bytes > workspace_bytes) return GSGEN_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_depth_fwd, dim3(w.n_chunks, B), dim3(kThreads), 0, s, pred, gt, gt_image_stride, mask, mask_image_stride, n_pixels,
                     w.partials);
  hipLaunchKernelGGL(k_depth_final, dim3(1), dim3(kThreads), 0, s, (const double *)w.partials, w.n_chunks, B, w.moments, loss_out);
  return (int)hipGetLastError();
}

int gsgen_depth_loss_backward(const float *pred, const float *gt, size_t gt_image_stride, const uint8_t *mask, size_t mask_image_stride,
                              uint32_t B, uint32_t n_pixels, const float *grad_scale_dev, float *grad_pred, float *grad_gt, void *workspace,
                              size_t workspace_bytes, gsgen_stream_t stream) {
  if (B > 65535u) return GSGEN_EUNSUPPORTED;
  if ((uint64_t)B * n_pixels == 0) return 0;
  if (!pred || !gt || !grad_scale_dev || !workspace) return GSGEN_EINVAL;
  if (grad_gt && gt_image_stride == 0 && B > 1) return GSGEN_EINVAL;  // (B images' gradients would land on one)
  const DepthWs w = carve_depth(workspace, B, n_pixels);
  if (w.bytes > workspace_bytes) return GSGEN_EWORKSPACE;
  if (!grad_pred && !grad_gt) return 0;
  hipLaunchKernelGGL(k_depth_bwd, dim3(w.n_chunks, B), dim3(kThreads), 0, (hipStream_t)stream, pred, gt, gt_image_stride, mask,
                     mask_image_stride, n_pixels, 1.0 / (double)B, (const double *)w.moments, grad_scale_dev, grad_pred, grad_gt);
  return (int)hipGetLastError();
}

#if defined(GSGEN_EMU_KNOBS)  // the CPU emulator build of tests/test_depth_loss_host.py only
void gsgen_depth_loss_emu_constants(uint32_t *out) { out[0] = kChunk; out[1] = kThreads; out[2] = kPartial; out[3] = kMoments; }
#endif

}  // extern "C"
