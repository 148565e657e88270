// background.hip -- the learned MLP background (gs/backgrounds.py:88-114, conf/renderer/mlp_bg.yaml) fused with its composite, for
// gfx950 (compiled with -ffp-contract=off; every fused multiply-add below is an explicit fmaf).
//
// The reference builds tcnn.NetworkWithInputEncoding(3, 3, SphericalHarmonics degree 3, FullyFusedMLP ReLU 16 x 2): tinycudann,
// CUDA only.  DESIGN.md ("MLP background") has the definition this file follows -- a reading of tcnn that no reference run pins.
// Per pixel (x, y) of view b, all in fp32:
//   d = R_b ((x - cx) / fx, (y - cy) / fy, 1)       (utils/camera.py:327-346, not normalised; or d = dirs[p], the call bg(rays_d))
//   e = 2 d - 1,  u[0..8] = sh_basis<3>(e) (composite_common.hpp),  u[9..15] = 1
//   h1 = relu(W0 u),  h2 = relu(W1 h1),  o = (W2 h2)[0..2],  bg = nan_to_num(1 / (1 + exp(-o)))      (a NaN becomes 0)
//   out = bg,  or  out = rgb_in + (1 - opacity) bg  (the composite form)
// params: 768 floats W0 | W1 | W2, each [16 out][16 in] row-major; rows 3..15 of W2 are never read, their gradient is exactly 0.
// Every dot product is a fmaf chain from 0 in the order of the input index.  A pixel whose o is not finite in all three channels
// contributes nothing to grad_params (its operands below are zeros); its grad_opacity is still -sum_c g_c bg_c with the bg the
// forward wrote.
//
// Kernels:
//   k_bg_fwd    a pixel per lane, weights through uniform (scalar) loads, every activation in registers.
//   k_bg_bwd    a workgroup of kThreads = 256 owns a run of iters * 256 consecutive pixels (of the flat [B H W] index: a run may
//               cross views).  Per pass a lane recomputes its pixel's forward, takes the upstream gradient, writes grad_opacity and
//               forms delta_o, delta_2 = relu'(W2^T delta_o), delta_1 = relu'(W1^T delta_2) in registers.  The weight gradient
//                 dW_l[out][in] = sum_p delta_l[p][out] act_{l-1}[p][in]        ([16 x P] . [P x 16], 464 live outputs)
//               does not fit a per-lane accumulator file, and summing 464 values across lanes per pixel batch would cost more
//               than the network.  It is the exact-fp32 MFMA's shape instead: __builtin_amdgcn_mfma_f32_16x16x4f32 with the PIXEL
//               as K.  A wave writes its 64 pixels' rows [pixel][16] of delta and of act to LDS; read back flat, word 64 s + lane is
//               element (lane & 15) of pixel 4 s + (lane >> 4), which is at once the A operand (delta^T: row = out, k = pixel) and
//               the B operand (act: k = pixel, column = in) of step s: sixteen MFMAs per layer per pass, no bank conflict on the read.
//               The MFMA is bit-for-bit a k-ordered fmaf chain, so a wave's accumulator (4 VGPRs per layer) is the fmaf chain over
//               its pixels in order.  After the last pass the four waves' accumulators are added in wave order and the workgroup
//               stores one partial [768].
//   k_bg_final  sums the partials: 8 slices per output (slice s takes partials s, s + 8, ... in order), then the slices in order.
// No float atomics, nothing is filled: the workspace may arrive dirty and unaligned.  Results are bit-identical from run to run.
// Nothing synchronises with the host, nothing is allocated, launch shapes depend on B, H, W alone: capturable; a replay reads the
// parameters, the camera blocks and the upstream gradient that are in the buffers then.
//
// The CPU emulator (oracle/emu) has no MFMA: under GSGEN_EMU_KNOBS mfma16x16x4 below gathers the four products of every output
// with __shfl and chains them with fmaf in k order -- the GPU's operations in the GPU's order.  Only expf differs between the two
// builds (libm against the device library).
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "composite_common.hpp"

namespace gs_bg {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kWidth = 16;                        // neurons per layer = padded encoding width
constexpr int kLayer = kWidth * kWidth;           // floats of one weight matrix
constexpr int kParams = 3 * kLayer;               // 768
constexpr int kMinIters = 4;                      // passes of a backward workgroup, at least
constexpr uint32_t kMaxGroups = 1024;             // backward workgroups (= partials), at most
constexpr int kSlices = 8, kFinalElems = 32;      // k_bg_final: 32 outputs x 8 slices per workgroup
constexpr uint32_t kMaxPixels = 1u << 31;

#if defined(GSGEN_EMU_KNOBS)
struct f32x4 {
  float v[4];
  float &operator[](int i) { return v[i]; }
  float operator[](int i) const { return v[i]; }
};
// D = A B + C of v_mfma_f32_16x16x4_f32: lane l holds A[l & 15][l >> 4], B[l >> 4][l & 15] and D[4 (l >> 4) + r][l & 15] in
// element r; each output is fma(a_3, b_3, fma(a_2, b_2, fma(a_1, b_1, fma(a_0, b_0, C))))
__device__ __forceinline__ f32x4 mfma16x16x4(float a, float b, f32x4 c) {
  const int lane = (int)(threadIdx.x & 63u), col = lane & 15, row0 = (lane >> 4) * 4;
  float bk[4];
  for (int k = 0; k < 4; ++k) bk[k] = __shfl(b, col + 16 * k);
  for (int r = 0; r < 4; ++r)
    for (int k = 0; k < 4; ++k) c[r] = fmaf(__shfl(a, row0 + r + 16 * k), bk[k], c[r]);
  return c;
}
#else
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 mfma16x16x4(float a, float b, f32x4 c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
#else
  return c;
#endif
}
#endif

struct Rays {
  const char *cams;   // per-view camera blocks (floats 0..11 c2w rows, 12..15 fx fy cx cy), cam_stride bytes apart; or
  size_t cam_stride;
  const float *dirs;  // [P][3]
  uint32_t HW, W;
};

__device__ __forceinline__ bool is_finite(float v) { return fabsf(v) <= FLT_MAX; }  // (false for a NaN)
__device__ __forceinline__ float relu(float z) { return z < 0.0f ? 0.0f : z; }      // (a NaN stays, as torch's does)

__device__ __forceinline__ void ray_dir(const Rays &r, uint32_t p, float (&d)[3]) {
  if (r.dirs) {
    const float *q = r.dirs + (size_t)p * 3;
    d[0] = q[0]; d[1] = q[1]; d[2] = q[2];
    return;
  }
  const uint32_t b = p / r.HW, i = p - b * r.HW, y = i / r.W, x = i - y * r.W;
  const float *c = (const float *)(r.cams + (size_t)b * r.cam_stride);
  const float qx = ((float)x - c[14]) / c[12], qy = ((float)y - c[15]) / c[13];
  d[0] = c[0] * qx + c[1] * qy + c[2];
  d[1] = c[4] * qx + c[5] * qy + c[6];
  d[2] = c[8] * qx + c[9] * qy + c[10];
}

__device__ __forceinline__ void encode(const float (&d)[3], float (&u)[kWidth]) {
  float Y[9];
  gs::sh_basis<3>(2.0f * d[0] - 1.0f, 2.0f * d[1] - 1.0f, 2.0f * d[2] - 1.0f, Y);
#pragma unroll
  for (int k = 0; k < 9; ++k) u[k] = Y[k];
#pragma unroll
  for (int k = 9; k < kWidth; ++k) u[k] = 1.0f;
}

// z[j] = sum_i Wm[j][i] in[i], j < NOUT
template <int NOUT>
__device__ __forceinline__ void matvec(const float *__restrict__ Wm, const float (&in)[kWidth], float (&z)[NOUT]) {
#pragma unroll
  for (int j = 0; j < NOUT; ++j) {
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < kWidth; ++i) acc = fmaf(Wm[kWidth * j + i], in[i], acc);
    z[j] = acc;
  }
}

// z[i] = sum_j Wm[j][i] in[j], j < NIN
template <int NIN>
__device__ __forceinline__ void matvec_t(const float *__restrict__ Wm, const float (&in)[NIN], float (&z)[kWidth]) {
#pragma unroll
  for (int i = 0; i < kWidth; ++i) {
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < NIN; ++j) acc = fmaf(Wm[kWidth * j + i], in[j], acc);
    z[i] = acc;
  }
}

// the network on one pixel: u, h1, h2, the raw outputs o and s = 1 / (1 + exp(-o))
__device__ __forceinline__ void network(const float *__restrict__ params, const float (&d)[3], float (&u)[kWidth], float (&h1)[kWidth],
                                        float (&h2)[kWidth], float (&o)[3], float (&s)[3]) {
  encode(d, u);
  matvec<kWidth>(params, u, h1);
#pragma unroll
  for (int j = 0; j < kWidth; ++j) h1[j] = relu(h1[j]);
  matvec<kWidth>(params + kLayer, h1, h2);
#pragma unroll
  for (int j = 0; j < kWidth; ++j) h2[j] = relu(h2[j]);
  matvec<3>(params + 2 * kLayer, h2, o);
#pragma unroll
  for (int c = 0; c < 3; ++c) s[c] = 1.0f / (1.0f + expf(-o[c]));
}

__device__ __forceinline__ float nan_to_zero(float v) { return v != v ? 0.0f : v; }  // (a sigmoid is never infinite)

__global__ void __launch_bounds__(kThreads) k_bg_fwd(Rays rays, const float *__restrict__ params, const float *__restrict__ rgb_in,
                                                      const float *__restrict__ opacity, uint32_t P, float *__restrict__ out) {
  const uint32_t p = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
  if (p >= P) return;
  float d[3], u[kWidth], h1[kWidth], h2[kWidth], o[3], s[3];
  ray_dir(rays, p, d);
  network(params, d, u, h1, h2, o, s);
  float *q = out + (size_t)p * 3;
  if (rgb_in) {
    const float k = 1.0f - opacity[p];
    const float *rgb = rgb_in + (size_t)p * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = rgb[c] + k * nan_to_zero(s[c]);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = nan_to_zero(s[c]);
  }
}

// a lane's row [16] of one operand into its wave's stage: word 16 lane + i
__device__ __forceinline__ void stage_row(float *__restrict__ stage, int lane, const float (&v)[kWidth]) {
  float4 *q = reinterpret_cast<float4 *>(stage + kWidth * lane);
#pragma unroll
  for (int i = 0; i < kWidth / 4; ++i) q[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
}

// acc += delta^T act over the wave's 64 pixels, four per step, in pixel order
__device__ __forceinline__ f32x4 wave_outer(const float *__restrict__ sa, const float *__restrict__ sb, int lane, f32x4 acc) {
#pragma unroll
  for (int s = 0; s < 16; ++s) acc = mfma16x16x4(sa[64 * s + lane], sb[64 * s + lane], acc);
  return acc;
}

__global__ void __launch_bounds__(kThreads) k_bg_bwd(Rays rays, const float *__restrict__ params, const float *__restrict__ opacity,
                                                      const float *__restrict__ grad_out, uint32_t P, uint32_t iters,
                                                      float *__restrict__ grad_opacity, float *__restrict__ partials) {
  __shared__ __attribute__((aligned(16))) float sStage[kWaves][2][64 * kWidth];  // per wave: delta rows | activation rows (32 KB; the epilogue reuses it)
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  float *sa = sStage[wave][0], *sb = sStage[wave][1];
  f32x4 acc0, acc1, acc2;
#pragma unroll
  for (int r = 0; r < 4; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; acc2[r] = 0.0f; }

  for (uint32_t it = 0; it < iters; ++it) {
    const uint32_t p = (blockIdx.x * iters + it) * (uint32_t)kThreads + (uint32_t)t;
    const bool in = p < P;
    float d[3] = {0.0f, 0.0f, 0.0f}, u[kWidth], h1[kWidth], h2[kWidth], o[3], s[3], g[3] = {0.0f, 0.0f, 0.0f};
    if (in) ray_dir(rays, p, d);
    network(params, d, u, h1, h2, o, s);
    float k = 1.0f;
    if (in) {
      const float *q = grad_out + (size_t)p * 3;
      g[0] = q[0]; g[1] = q[1]; g[2] = q[2];
      if (opacity) k = 1.0f - opacity[p];
      if (grad_opacity) {
        const float b0 = nan_to_zero(s[0]), b1 = nan_to_zero(s[1]), b2 = nan_to_zero(s[2]);
        grad_opacity[p] = -fmaf(g[2], b2, fmaf(g[1], b1, g[0] * b0));
      }
    }
    const bool live = in && is_finite(o[0]) && is_finite(o[1]) && is_finite(o[2]);
    float dl[kWidth], dn[kWidth];  // the layer's delta, and the next one down
#pragma unroll
    for (int c = 0; c < 3; ++c) dl[c] = live ? (g[c] * k) * (s[c] * (1.0f - s[c])) : 0.0f;
#pragma unroll
    for (int c = 3; c < kWidth; ++c) dl[c] = 0.0f;
    if (!live) {
#pragma unroll
      for (int i = 0; i < kWidth; ++i) { u[i] = 0.0f; h1[i] = 0.0f; h2[i] = 0.0f; }
    }
    // layer 2: dW2 += delta_o^T h2 (rows 3..15 of the operand are zeros)
    stage_row(sa, lane, dl);
    stage_row(sb, lane, h2);
    __syncthreads();
    acc2 = wave_outer(sa, sb, lane, acc2);
    {
      const float d3[3] = {dl[0], dl[1], dl[2]};
      matvec_t<3>(params + 2 * kLayer, d3, dn);
    }
#pragma unroll
    for (int j = 0; j < kWidth; ++j) dl[j] = h2[j] > 0.0f ? dn[j] : 0.0f;
    __syncthreads();
    // layer 1: dW1 += delta_2^T h1
    stage_row(sa, lane, dl);
    stage_row(sb, lane, h1);
    __syncthreads();
    acc1 = wave_outer(sa, sb, lane, acc1);
    matvec_t<kWidth>(params + kLayer, dl, dn);
#pragma unroll
    for (int j = 0; j < kWidth; ++j) dl[j] = h1[j] > 0.0f ? dn[j] : 0.0f;
    __syncthreads();
    // layer 0: dW0 += delta_1^T u
    stage_row(sa, lane, dl);
    stage_row(sb, lane, u);
    __syncthreads();
    acc0 = wave_outer(sa, sb, lane, acc0);
    __syncthreads();
  }

  // the waves' accumulators, in wave order: element r of lane l is dW[4 (l >> 4) + r][l & 15]
  float *sRed = &sStage[0][0][0];  // [kWaves][kParams] = 12 KB of the 32
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int e = kWidth * (4 * (lane >> 4) + r) + (lane & 15);
    sRed[kParams * wave + e] = acc0[r];
    sRed[kParams * wave + kLayer + e] = acc1[r];
    sRed[kParams * wave + 2 * kLayer + e] = acc2[r];
  }
  __syncthreads();
  float *o = partials + (size_t)kParams * blockIdx.x;
#pragma unroll
  for (int j = 0; j < kParams / kThreads; ++j) {
    const int e = kThreads * j + t;
    float v = sRed[e];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v += sRed[kParams * w + e];
    o[e] = e < 2 * kLayer + 3 * kWidth ? v : 0.0f;  // (W2's padding rows: exactly 0)
  }
}

__global__ void __launch_bounds__(kSlices * kFinalElems) k_bg_final(const float *__restrict__ partials, uint32_t n_groups,
                                                                    float *__restrict__ grad_params) {
  __shared__ float sSum[kSlices][kFinalElems];
  const int t = threadIdx.x, x = t % kFinalElems, slice = t / kFinalElems;
  const uint32_t e = blockIdx.x * (uint32_t)kFinalElems + (uint32_t)x;
  float v = 0.0f;
  for (uint32_t j = slice; j < n_groups; j += kSlices) v += partials[(size_t)kParams * j + e];
  sSum[slice][x] = v;
  __syncthreads();
  if (slice == 0) {
#pragma unroll
    for (int s = 1; s < kSlices; ++s) v += sSum[s][x];
    grad_params[e] = v;
  }
}

// --- host side ---------------------------------------------------------------------------------------------------------
struct BgPlan {
  uint32_t P, iters, n_groups;
  size_t bytes;
};

// P = 0: empty or unsupported (the caller tells them apart)
inline BgPlan plan_bg(uint32_t B, uint32_t H, uint32_t W) {
  BgPlan pl{0, 0, 0, 0};
  const uint64_t P = (uint64_t)B * H * W;
  if (P == 0 || P > kMaxPixels) return pl;
  pl.P = (uint32_t)P;
  const uint64_t per = (uint64_t)kThreads * kMaxGroups;
  pl.iters = (uint32_t)((P + per - 1) / per);
  if (pl.iters < (uint32_t)kMinIters) pl.iters = kMinIters;
  const uint64_t run = (uint64_t)pl.iters * kThreads;
  pl.n_groups = (uint32_t)((P + run - 1) / run);
  pl.bytes = sizeof(float) * kParams * (size_t)pl.n_groups + 512;  // (256 to align the base, 256 spare)
  return pl;
}

inline float *align_ws(void *base) {
  char *p = (char *)base;
  return (float *)(p + ((256 - ((uintptr_t)p & 255)) & 255));
}

inline bool too_big(uint32_t B, uint32_t H, uint32_t W) { return (uint64_t)B * H * W > kMaxPixels; }

// exactly one source of directions; camera blocks at least 16 floats, a whole number of floats apart
inline bool rays_ok(const void *cams, size_t cam_stride, const float *dirs, uint32_t B) {
  if ((cams != nullptr) == (dirs != nullptr)) return false;
  if (cams && ((cam_stride & 3) != 0 || (B > 1 && cam_stride < 64) || ((uintptr_t)cams & 3) != 0)) return false;
  return true;
}

}  // namespace gs_bg

using namespace gs_bg;

extern "C" {

size_t gsgen_mlp_background_workspace_bytes(uint32_t B, uint32_t H, uint32_t W) { return plan_bg(B, H, W).bytes; }

int gsgen_mlp_background_forward(const float *params, const void *cams, size_t cam_stride_bytes, const float *dirs, uint32_t B,
                                 uint32_t H, uint32_t W, const float *rgb_in, const float *opacity, float *out, gsgen_stream_t stream) {
  if (too_big(B, H, W)) return GSGEN_EUNSUPPORTED;
  const BgPlan pl = plan_bg(B, H, W);
  if (pl.P == 0) return 0;
  if (!params || !out || !rays_ok(cams, cam_stride_bytes, dirs, B)) return GSGEN_EINVAL;
  if ((rgb_in != nullptr) != (opacity != nullptr)) return GSGEN_EINVAL;
  const Rays rays{(const char *)cams, cam_stride_bytes, dirs, H * W, W};
  hipLaunchKernelGGL(k_bg_fwd, dim3((pl.P + kThreads - 1) / kThreads), dim3(kThreads), 0, (hipStream_t)stream, rays, params, rgb_in, opacity,
                     pl.P, out);
  return (int)hipGetLastError();
}

int gsgen_mlp_background_backward(const float *params, const void *cams, size_t cam_stride_bytes, const float *dirs, uint32_t B,
                                  uint32_t H, uint32_t W, const float *opacity, const float *grad_out, float *grad_params,
                                  float *grad_opacity, void *workspace, size_t workspace_bytes, gsgen_stream_t stream) {
  if (too_big(B, H, W)) return GSGEN_EUNSUPPORTED;
  const BgPlan pl = plan_bg(B, H, W);
  if (pl.P == 0) return 0;
  if (!params || !grad_out || !grad_params || !workspace || !rays_ok(cams, cam_stride_bytes, dirs, B)) return GSGEN_EINVAL;
  if (grad_opacity && !opacity) return GSGEN_EINVAL;
  if (pl.bytes > workspace_bytes) return GSGEN_EWORKSPACE;
  float *partials = align_ws(workspace);
  const Rays rays{(const char *)cams, cam_stride_bytes, dirs, H * W, W};
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_bg_bwd, dim3(pl.n_groups), dim3(kThreads), 0, s, rays, params, opacity, grad_out, pl.P, pl.iters, grad_opacity,
                     partials);
  hipLaunchKernelGGL(k_bg_final, dim3(kParams / kFinalElems), dim3(kSlices * kFinalElems), 0, s, (const float *)partials, pl.n_groups,
                     grad_params);
  return (int)hipGetLastError();
}

#if defined(GSGEN_EMU_KNOBS)  // the CPU emulator build of tests/test_background_host.py only
void gsgen_mlp_background_emu_constants(uint32_t *out) { out[0] = kThreads; out[1] = kMinIters; out[2] = kMaxGroups; out[3] = kSlices; }
#endif

}  // extern "C"
