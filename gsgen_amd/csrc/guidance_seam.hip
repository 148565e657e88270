// guidance_seam.hip -- the seam between the rendered batch and the diffusion guidance of the text-to-3D step, for gfx950 (compiled with
// -ffp-contract=off): the guidance's input image from the render, and the SDS loss from the UNet's gradient.
//
// Going in it replaces (guidance/stable_diffusion.py:274-284 with encode_images at :143-149, stable_diffusion_vsd.py:419, :586-590,
// make_it_3d.py:124-128, deep_floyd.py:196-201, trainer.py:661-673)
//   rgb.permute(0, 3, 1, 2) -> F.interpolate(.., (OH, OW), mode="bilinear", align_corners=False) -> * 2.0 -> - 1.0 -> .to(fp16)
// and coming out (stable_diffusion.py:298-312)
//   nan_to_num -> clamp -> latents - grad -> mse_loss(reduction="sum") -> * 0.5 -> / bs, with loss_sds_each and grad.norm().
// DESIGN.md ("Guidance seam") has the definitions; in short:
//
// Guidance input.  x [B][H][W][C] fp32 channels last, C in {1, 3} -> out = scale * bilinear(x) + shift at OH x OW, planar
// [B][C][OH][OW] or channels last [B][OH][OW][C], fp16 (round to nearest even) or fp32.  Per axis, torch's upsample_bilinear2d map
// with align_corners=False and no antialiasing, in fp32:
//   src = max((float)in / (float)out * (o + 0.5f) - 0.5f, 0),  i0 = min((int)src, in - 1),  i1 = min(i0 + 1, in - 1),
//   l1 = src - i0,  l0 = 1 - l1,   v = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11),   out = scale * v + shift.
//   k_guidance_tables     the per-axis tables, in the workspace: (i0, l1) per output index, and per input index i the range
//                         [o_begin, o_end) of the outputs with i0 in {i - 1, i} -- every output that read i, as i0 or as i1.  i0 is
//                         non-decreasing in o, so that set is one contiguous range, found by bisection on the same fp32 map.
//   k_guidance_input_fwd  one lane = kPix = 4 horizontally adjacent output pixels of one row, all channels: a planar fp16 row gets 8 B
//                         per lane and channel, an fp32 one 16 B, a channels-last run 24 / 48 B, each in the widest stores the
//                         address allows (with fp16 and an odd OH * OW every second plane starts 2 B off a 4 B boundary: store_run
//                         falls back to 2 B / 4 B stores there).
//   k_guidance_input_bwd  a GATHER: one lane per input pixel sums, output row ascending, then output column ascending, in fp32
//                           grad_x = scale * sum_oy wy(oy) * (sum_ox wx(ox) * g[oy][ox]),   w(o) = (i0 == i ? l0 : 0) + (i1 == i ? l1 : 0)
//                         with the weights from the forward's own table: the exact adjoint of the forward.  No float atomics, no
//                         fill; every input pixel is written once, an input pixel no output read as an exact zero.  The upstream
//                         gradient is fp16 or fp32 in either layout.
//
// SDS loss.  grad [B][n] fp32 -> g' = clamp(nan_to_num(grad), -clip, clip) (NaN -> 0, +-Inf -> +-FLT_MAX; the clip is optional),
//   loss = 0.5 sum g'^2 / B,  loss_each[b] = 0.5 sum_b g'^2,  grad_norm = sqrt(sum g'^2),  saved = g' / B.
// The reference forms latents - (latents - g'), which is g' up to one rounding of latents: summing g'^2 is the more accurate value
// of the same quantity, and it does not read latents at all.
//   k_sds_loss_fwd    a workgroup = 256 threads owns kChunk = 1024 consecutive elements of one image: writes saved, sums g'^2 in fp64
//                     (wave shuffles, then the waves in order through LDS), one partial per workgroup.
//   k_sds_loss_final  one workgroup; a wave per image sums that image's partials in a fixed order, then the waves in order.
//   k_sds_loss_bwd    d loss / d latents = upstream * saved, the upstream 0-dim scalar read from device memory.
// No float atomics anywhere: bit-identical from run to run.  Launch shapes depend on the sizes alone, nothing synchronises with the
// host: capturable.  The workspaces may arrive dirty and unaligned.
//
// -ffp-contract=off: nothing is fused, so the g++ build of this file on the CPU emulator (tests/test_guidance_host.py) performs the
// GPU's operations in the GPU's order.  The emulator has no half type: there the fp16 conversions are the bit-level routines below;
// on the device they are the hardware's.
#include <hip/hip_runtime.h>
#if defined(__HIPCC__)
#include <hip/hip_fp16.h>
#define GSGEN_HW_FP16 1
#endif
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/gsgen_hip.h"

namespace gs_guidance {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPix = 4;                     // horizontally adjacent output pixels of one lane
constexpr int kPer = 4;                     // SDS: elements of a chunk one thread holds
constexpr int kChunk = kThreads * kPer;     // SDS: elements of one image a workgroup reduces
constexpr uint32_t kMaxSide = 1u << 16;     // image sides (the tables index with 32 bits; the limit keeps every product below 2^64)

// ---- fp16 <-> fp32 ---------------------------------------------------------------------------------------------------------
#if !defined(GSGEN_HW_FP16)
// round to nearest even, bit level (the host build: no half type there)
inline uint16_t f32_to_f16_bits(float f) {
  uint32_t x;
  memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u, a = x & 0x7fffffffu;
  if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u | ((a >> 13) & 0x1ffu));  // NaN: quiet, the payload's top bits kept
  if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                         // >= 65520 rounds to infinity
  if (a < 0x38800000u) {                                                            // below 2^-14: a subnormal half, or zero
    const uint32_t e = a >> 23;
    if (e < 101u) return (uint16_t)sign;                                            // below 2^-26
    const uint32_t mant = (a & 0x7fffffu) | 0x800000u, shift = 126u - e;            // 14..25; the result in units of 2^-24
    uint32_t r = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rem > half || (rem == half && (r & 1u))) ++r;
    return (uint16_t)(sign | r);
  }
  uint32_t r = (a - 0x38000000u) >> 13;
  const uint32_t rem = a & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) ++r;
  return (uint16_t)(sign | r);
}
inline float f16_bits_to_f32(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
  uint32_t x;
  if (e == 31u) x = sign | 0x7f800000u | (m << 13);
  else if (e != 0u) x = sign | ((e + 112u) << 23) | (m << 13);
  else {
    const float v = (float)m * 5.9604644775390625e-08f;  // m * 2^-24, exact
    memcpy(&x, &v, 4);
    x |= sign;
  }
  float f;
  memcpy(&f, &x, 4);
  return f;
}
#else
__device__ __forceinline__ uint16_t f32_to_f16_bits(float f) { return __half_as_ushort(__float2half_rn(f)); }
__device__ __forceinline__ float f16_bits_to_f32(uint16_t h) { return __half2float(__ushort_as_half(h)); }
#endif

template <typename T> __device__ __forceinline__ T to_out(float v);
template <> __device__ __forceinline__ float to_out<float>(float v) { return v; }
template <> __device__ __forceinline__ uint16_t to_out<uint16_t>(float v) { return f32_to_f16_bits(v); }

// ---- the per-axis tables -----------------------------------------------------------------------------------------------------
struct AxisOut { int32_t i0; float l1; };     // per output index
struct AxisIn { uint32_t begin, end; };       // per input index: the outputs that read it

__device__ __forceinline__ AxisOut axis_map(uint32_t o, uint32_t n_in, uint32_t n_out) {
  const float rs = (float)n_in / (float)n_out;
  float src = rs * ((float)o + 0.5f) - 0.5f;
  if (src < 0.0f) src = 0.0f;
  int32_t i0 = (int32_t)src;
  if (i0 > (int32_t)n_in - 1) i0 = (int32_t)n_in - 1;
  return AxisOut{i0, src - (float)i0};
}

// the first output index whose i0 is at least `key` (n_out: none); i0 is non-decreasing in o
__device__ __forceinline__ uint32_t first_output_from(int32_t key, uint32_t n_in, uint32_t n_out) {
  uint32_t lo = 0, hi = n_out;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (axis_map(mid, n_in, n_out).i0 >= key) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__global__ void __launch_bounds__(kThreads) k_guidance_tables(AxisOut *__restrict__ fy, AxisOut *__restrict__ fx, AxisIn *__restrict__ by,
                                                               AxisIn *__restrict__ bx, uint32_t H, uint32_t W, uint32_t OH, uint32_t OW) {
  uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i < OH) { fy[i] = axis_map(i, H, OH); return; }
  i -= OH;
  if (i < OW) { fx[i] = axis_map(i, W, OW); return; }
  i -= OW;
  if (i < H) { by[i] = AxisIn{first_output_from((int32_t)i - 1, H, OH), first_output_from((int32_t)i + 1, H, OH)}; return; }
  i -= H;
  if (i < W) bx[i] = AxisIn{first_output_from((int32_t)i - 1, W, OW), first_output_from((int32_t)i + 1, W, OW)};
}

// ---- stores of a lane's run of n <= N adjacent elements, in the widest pieces the address allows ---------------------------------
template <typename T, int N> __device__ __forceinline__ uint32_t word_at(const T (&v)[N], int e) {
  if constexpr (sizeof(T) == 4) {
    return __float_as_uint(v[e < N ? e : N - 1]);
  } else {
    return (uint32_t)v[e < N ? e : N - 1] | ((uint32_t)v[e + 1 < N ? e + 1 : N - 1] << 16);
  }
}

template <typename T, int N> __device__ __forceinline__ void store_run(T *p, const T (&v)[N], int n) {
  constexpr int E16 = 16 / (int)sizeof(T), E8 = 8 / (int)sizeof(T), E4 = 4 / (int)sizeof(T), EW = 4 / (int)sizeof(T);  // elements per piece / word
  int next = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if (i == next && i < n) {
      const uintptr_t a = (uintptr_t)(p + i);
      const int left = n - i;
      if (i + E16 <= N && left >= E16 && (a & 15) == 0) {
        *reinterpret_cast<uint4 *>(p + i) = uint4{word_at(v, i), word_at(v, i + EW), word_at(v, i + 2 * EW), word_at(v, i + 3 * EW)};
        next = i + E16;
      } else if (i + E8 <= N && left >= E8 && (a & 7) == 0) {
        *reinterpret_cast<uint2 *>(p + i) = uint2{word_at(v, i), word_at(v, i + EW)};
        next = i + E8;
      } else if (E4 > 1 && i + E4 <= N && left >= E4 && (a & 3) == 0) {
        *reinterpret_cast<uint32_t *>(p + i) = word_at(v, i);
        next = i + E4;
      } else {
        p[i] = v[i];
        next = i + 1;
      }
    }
  }
}

// ---- guidance input, forward -------------------------------------------------------------------------------------------------
template <int C, typename T, bool PLANAR>
__global__ void __launch_bounds__(kThreads) k_guidance_input_fwd(const float *__restrict__ x, uint32_t B, uint32_t H, uint32_t W, uint32_t OH,
                                                                  uint32_t OW, float scale, float shift, const AxisOut *__restrict__ fy,
                                                                  const AxisOut *__restrict__ fx, T *__restrict__ out) {
  const uint32_t groups = (OW + kPix - 1) / kPix;
  const size_t gid = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (gid >= (size_t)B * OH * groups) return;
  const uint32_t gx = (uint32_t)(gid % groups);
  const size_t row = gid / groups;
  const uint32_t oy = (uint32_t)(row % OH), b = (uint32_t)(row / OH);
  const AxisOut ay = fy[oy];
  const int32_t y0 = ay.i0, y1 = min(y0 + 1, (int32_t)H - 1);
  const float ly1 = ay.l1, ly0 = 1.0f - ly1;
  const float *r0 = x + ((size_t)b * H + (size_t)y0) * W * C, *r1 = x + ((size_t)b * H + (size_t)y1) * W * C;
  const uint32_t ox0 = gx * kPix;
  const int n = (int)min((uint32_t)kPix, OW - ox0);

  T v[C][kPix];
#pragma unroll
  for (int j = 0; j < kPix; ++j) {
    if (j < n) {
      const AxisOut ax = fx[ox0 + j];
      const int32_t x0 = ax.i0, x1 = min(x0 + 1, (int32_t)W - 1);
      const float lx1 = ax.l1, lx0 = 1.0f - lx1;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const float v00 = r0[(size_t)x0 * C + c], v01 = r0[(size_t)x1 * C + c], v10 = r1[(size_t)x0 * C + c], v11 = r1[(size_t)x1 * C + c];
        const float val = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
        v[c][j] = to_out<T>(scale * val + shift);
      }
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) v[c][j] = T(0);
    }
  }
  if (PLANAR || C == 1) {
#pragma unroll
    for (int c = 0; c < C; ++c) store_run<T, kPix>(out + (((size_t)b * C + c) * OH + oy) * OW + ox0, v[c], n);
  } else {
    T run[C * kPix];
#pragma unroll
    for (int j = 0; j < kPix; ++j)
#pragma unroll
      for (int c = 0; c < C; ++c) run[j * C + c] = v[c][j];
    store_run<T, C * kPix>(out + (((size_t)b * OH + oy) * OW + ox0) * C, run, n * C);
  }
}

// ---- guidance input, backward: the gather ---------------------------------------------------------------------------------------
template <int C, typename T, bool PLANAR>
__global__ void __launch_bounds__(kThreads) k_guidance_input_bwd(const T *__restrict__ g, uint32_t B, uint32_t H, uint32_t W, uint32_t OH,
                                                                  uint32_t OW, float scale, const AxisOut *__restrict__ fy,
                                                                  const AxisOut *__restrict__ fx, const AxisIn *__restrict__ by,
                                                                  const AxisIn *__restrict__ bx, float *__restrict__ grad_x) {
  const size_t gid = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (gid >= (size_t)B * H * W) return;
  const int32_t ix = (int32_t)(gid % W), iy = (int32_t)((gid / W) % H);
  const uint32_t b = (uint32_t)(gid / ((size_t)W * H));
  const AxisIn ry = by[iy], rx = bx[ix];
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.0f;
  for (uint32_t oy = ry.begin; oy < ry.end; ++oy) {
    const AxisOut ay = fy[oy];
    const int32_t y1 = min(ay.i0 + 1, (int32_t)H - 1);
    const float wy = (ay.i0 == iy ? 1.0f - ay.l1 : 0.0f) + (y1 == iy ? ay.l1 : 0.0f);
    float rsum[C];
#pragma unroll
    for (int c = 0; c < C; ++c) rsum[c] = 0.0f;
    for (uint32_t ox = rx.begin; ox < rx.end; ++ox) {
      const AxisOut ax = fx[ox];
      const int32_t x1 = min(ax.i0 + 1, (int32_t)W - 1);
      const float wx = (ax.i0 == ix ? 1.0f - ax.l1 : 0.0f) + (x1 == ix ? ax.l1 : 0.0f);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const size_t at = PLANAR ? (((size_t)b * C + c) * OH + oy) * OW + ox : (((size_t)b * OH + oy) * OW + ox) * C + c;
        float gv;
        if constexpr (sizeof(T) == 4) gv = g[at]; else gv = f16_bits_to_f32(g[at]);
        rsum[c] = rsum[c] + wx * gv;
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = acc[c] + wy * rsum[c];
  }
#pragma unroll
  for (int c = 0; c < C; ++c) grad_x[gid * C + c] = scale * acc[c];
}

// ---- SDS loss ------------------------------------------------------------------------------------------------------------------
// torch.nan_to_num in fp32
__device__ __forceinline__ float sanitize(float v) { return v != v ? 0.0f : (v > FLT_MAX ? FLT_MAX : (v < -FLT_MAX ? -FLT_MAX : v)); }

__device__ __forceinline__ double wave_sum(double v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

__global__ void __launch_bounds__(kThreads) k_sds_loss_fwd(const float *__restrict__ grad, uint32_t n, float clip, int use_clip, float batch,
                                                            float *__restrict__ saved, double *__restrict__ partials) {
  __shared__ double sRed[kWaves];
  const int t = threadIdx.x;
  const uint32_t b = blockIdx.y;
  const size_t c0 = (size_t)blockIdx.x * kChunk;
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const size_t i = c0 + (size_t)(j * kThreads + t);
    if (i < (size_t)n) {
      float v = sanitize(grad[(size_t)b * n + i]);
      if (use_clip) v = fminf(fmaxf(v, -clip), clip);
      saved[(size_t)b * n + i] = v / batch;
      s += (double)v * (double)v;
    }
  }
  s = wave_sum(s);
  if ((t & 63) == 0) sRed[t >> 6] = s;
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < kWaves; ++w) s += sRed[w];
    partials[(size_t)b * gridDim.x + blockIdx.x] = s;
  }
}

// loss_out: float[2 + B] = loss, grad_norm, loss_each[B]
__global__ void __launch_bounds__(kThreads) k_sds_loss_final(const double *__restrict__ partials, uint32_t n_chunks, uint32_t B,
                                                              float *__restrict__ loss_out) {
  __shared__ double sSum[kWaves];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  double sum = 0.0;  // (lane 0: this wave's images, in order)
  for (uint32_t b = wave; b < B; b += kWaves) {
    const double *p = partials + (size_t)b * n_chunks;
    double acc = 0.0;
    for (uint32_t c = lane; c < n_chunks; c += 64) acc += p[c];
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d);
    if (lane == 0) {
      loss_out[2 + b] = (float)(0.5 * acc);
      sum += acc;
    }
  }
  if (lane == 0) sSum[wave] = sum;
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < kWaves; ++w) sum += sSum[w];
    loss_out[0] = (float)(0.5 * sum / (double)B);
    loss_out[1] = (float)sqrt(sum);
  }
}

__global__ void __launch_bounds__(kThreads) k_sds_loss_bwd(const float *__restrict__ saved, const float *__restrict__ grad_scale, size_t total,
                                                            float *__restrict__ grad_latents) {
  const float k = grad_scale[0];
  const size_t c0 = (size_t)blockIdx.x * kChunk;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const size_t i = c0 + (size_t)(j * kThreads + threadIdx.x);
    if (i < total) grad_latents[i] = k * saved[i];
  }
}

// --- host side ---------------------------------------------------------------------------------------------------------
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct TablesWs {
  AxisOut *fy, *fx;
  AxisIn *by, *bx;
  size_t bytes;
};

inline TablesWs carve_tables(void *base, uint32_t H, uint32_t W, uint32_t OH, uint32_t OW) {
  char *p0 = (char *)base, *p = p0 + ((256 - ((uintptr_t)p0 & 255)) & 255);
  TablesWs w;
  size_t off = 0;
  auto take = [&](size_t b) { char *r = p + off; off += align256(b); return r; };
  w.fy = (AxisOut *)take(sizeof(AxisOut) * OH);
  w.fx = (AxisOut *)take(sizeof(AxisOut) * OW);
  w.by = (AxisIn *)take(sizeof(AxisIn) * H);
  w.bx = (AxisIn *)take(sizeof(AxisIn) * W);
  w.bytes = off + 256;
  return w;
}

struct SdsWs {
  float *saved;      // [B][n]
  double *partials;  // [B][n_chunks]
  uint32_t n_chunks;
  size_t bytes;
};

inline SdsWs carve_sds(void *base, uint32_t B, uint32_t n) {
  char *p0 = (char *)base, *p = p0 + ((256 - ((uintptr_t)p0 & 255)) & 255);
  SdsWs w;
  w.n_chunks = (uint32_t)(((uint64_t)n + kChunk - 1) / kChunk);
  size_t off = 0;
  auto take = [&](size_t b) { char *r = p + off; off += align256(b); return r; };
  w.saved = (float *)take(sizeof(float) * (size_t)B * n);
  w.partials = (double *)take(sizeof(double) * (size_t)B * w.n_chunks);
  w.bytes = off + 256;
  return w;
}

inline uint64_t blocks_for(uint64_t threads) { return (threads + kThreads - 1) / kThreads; }

// 0, or the error code of a guidance-input call's sizes
inline int check_sizes(uint32_t B, uint32_t H, uint32_t W, uint32_t C, uint32_t OH, uint32_t OW) {
  if (B == 0 || H == 0 || W == 0 || C == 0 || OH == 0 || OW == 0) return GSGEN_EINVAL;
  if (C != 1 && C != 3) return GSGEN_EUNSUPPORTED;
  if (H > kMaxSide || W > kMaxSide || OH > kMaxSide || OW > kMaxSide) return GSGEN_EUNSUPPORTED;
  if (blocks_for((uint64_t)B * OH * OW) > 0x7fffffffull || blocks_for((uint64_t)B * H * W) > 0x7fffffffull) return GSGEN_EUNSUPPORTED;  // (grid.x)
  return 0;
}

inline int check_sds(uint32_t B, uint32_t n) {
  if (B == 0 || n == 0) return GSGEN_EINVAL;
  if (B > 65535u || ((uint64_t)B * n + kChunk - 1) / kChunk > 0x7fffffffull) return GSGEN_EUNSUPPORTED;  // (grid.y, grid.x)
  return 0;
}

template <int C, typename T>
inline void launch_fwd(bool planar, dim3 grid, hipStream_t s, const float *x, uint32_t B, uint32_t H, uint32_t W, uint32_t OH, uint32_t OW,
                       float scale, float shift, const TablesWs &w, void *out) {
  const AxisOut *fy = w.fy, *fx = w.fx;
  T *o = (T *)out;
  if (planar) hipLaunchKernelGGL((k_guidance_input_fwd<C, T, true>), grid, dim3(kThreads), 0, s, x, B, H, W, OH, OW, scale, shift, fy, fx, o);
  else hipLaunchKernelGGL((k_guidance_input_fwd<C, T, false>), grid, dim3(kThreads), 0, s, x, B, H, W, OH, OW, scale, shift, fy, fx, o);
}

template <int C, typename T>
inline void launch_bwd(bool planar, dim3 grid, hipStream_t s, const void *g, uint32_t B, uint32_t H, uint32_t W, uint32_t OH, uint32_t OW,
                       float scale, const TablesWs &w, float *grad_x) {
  const AxisOut *fy = w.fy, *fx = w.fx;
  const AxisIn *by = w.by, *bx = w.bx;
  const T *gp = (const T *)g;
  if (planar) hipLaunchKernelGGL((k_guidance_input_bwd<C, T, true>), grid, dim3(kThreads), 0, s, gp, B, H, W, OH, OW, scale, fy, fx, by, bx, grad_x);
  else hipLaunchKernelGGL((k_guidance_input_bwd<C, T, false>), grid, dim3(kThreads), 0, s, gp, B, H, W, OH, OW, scale, fy, fx, by, bx, grad_x);
}

}  // namespace gs_guidance

using namespace gs_guidance;

extern "C" {

size_t gsgen_guidance_input_workspace_bytes(uint32_t H, uint32_t W, uint32_t OH, uint32_t OW) {
  if (check_sizes(1, H, W, 1, OH, OW) != 0) return 0;
  return carve_tables(nullptr, H, W, OH, OW).bytes;
}

int gsgen_guidance_input_forward(const float *x, uint32_t B, uint32_t H, uint32_t W, uint32_t C, uint32_t OH, uint32_t OW, float scale,
                                 float shift, int out_half, int out_planar, void *out, int build_tables, void *workspace,
                                 size_t workspace_bytes, gsgen_stream_t stream) {
  const int bad = check_sizes(B, H, W, C, OH, OW);
  if (bad) return bad;
  if (!x || !out || !workspace) return GSGEN_EINVAL;
  const TablesWs w = carve_tables(workspace, H, W, OH, OW);
  if (w.bytes > workspace_bytes) return GSGEN_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  if (build_tables)
    hipLaunchKernelGGL(k_guidance_tables, dim3((uint32_t)blocks_for((uint64_t)OH + OW + H + W)), dim3(kThreads), 0, s, w.fy, w.fx, w.by, w.bx, H, W,
                       OH, OW);
  const dim3 grid((uint32_t)blocks_for((uint64_t)B * OH * ((OW + kPix - 1) / kPix)));
  const bool planar = out_planar != 0;
  if (C == 3) {
    if (out_half) launch_fwd<3, uint16_t>(planar, grid, s, x, B, H, W, OH, OW, scale, shift, w, out);
    else launch_fwd<3, float>(planar, grid, s, x, B, H, W, OH, OW, scale, shift, w, out);
  } else {
    if (out_half) launch_fwd<1, uint16_t>(true, grid, s, x, B, H, W, OH, OW, scale, shift, w, out);
    else launch_fwd<1, float>(true, grid, s, x, B, H, W, OH, OW, scale, shift, w, out);
  }
  return (int)hipGetLastError();
}

int gsgen_guidance_input_backward(const void *grad_out, int grad_half, int grad_planar, uint32_t B, uint32_t H, uint32_t W, uint32_t C,
                                  uint32_t OH, uint32_t OW, float scale, float *grad_x, void *workspace, size_t workspace_bytes,
                                  gsgen_stream_t stream) {
  const int bad = check_sizes(B, H, W, C, OH, OW);
  if (bad) return bad;
  if (!grad_out || !grad_x || !workspace) return GSGEN_EINVAL;
  const TablesWs w = carve_tables(workspace, H, W, OH, OW);
  if (w.bytes > workspace_bytes) return GSGEN_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((uint32_t)blocks_for((uint64_t)B * H * W));
  const bool planar = grad_planar != 0;
  if (C == 3) {
    if (grad_half) launch_bwd<3, uint16_t>(planar, grid, s, grad_out, B, H, W, OH, OW, scale, w, grad_x);
    else launch_bwd<3, float>(planar, grid, s, grad_out, B, H, W, OH, OW, scale, w, grad_x);
  } else {
    if (grad_half) launch_bwd<1, uint16_t>(true, grid, s, grad_out, B, H, W, OH, OW, scale, w, grad_x);
    else launch_bwd<1, float>(true, grid, s, grad_out, B, H, W, OH, OW, scale, w, grad_x);
  }
  return (int)hipGetLastError();
}

size_t gsgen_sds_loss_workspace_bytes(uint32_t B, uint32_t n) {
  if (check_sds(B, n) != 0) return 0;
  return carve_sds(nullptr, B, n).bytes;
}

int gsgen_sds_loss_forward(const float *grad, uint32_t B, uint32_t n, int use_clip, float clip, float *loss_out, void *workspace,
                           size_t workspace_bytes, gsgen_stream_t stream) {
  const int bad = check_sds(B, n);
  if (bad) return bad;
  if (!grad || !loss_out || !workspace) return GSGEN_EINVAL;
  if (use_clip && !(clip >= 0.0f)) return GSGEN_EINVAL;  // (a negative or NaN clip)
  const SdsWs w = carve_sds(workspace, B, n);
  if (w.bytes > workspace_bytes) return GSGEN_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_sds_loss_fwd, dim3(w.n_chunks, B), dim3(kThreads), 0, s, grad, n, clip, use_clip, (float)B, w.saved, w.partials);
  hipLaunchKernelGGL(k_sds_loss_final, dim3(1), dim3(kThreads), 0, s, (const double *)w.partials, w.n_chunks, B, loss_out);
  return (int)hipGetLastError();
}

int gsgen_sds_loss_backward(uint32_t B, uint32_t n, const float *grad_scale_dev, float *grad_latents, void *workspace, size_t workspace_bytes,
                            gsgen_stream_t stream) {
  const int bad = check_sds(B, n);
  if (bad) return bad;
  if (!grad_scale_dev || !grad_latents || !workspace) return GSGEN_EINVAL;
  const SdsWs w = carve_sds(workspace, B, n);
  if (w.bytes > workspace_bytes) return GSGEN_EWORKSPACE;
  const size_t total = (size_t)B * n;
  hipLaunchKernelGGL(k_sds_loss_bwd, dim3((uint32_t)((total + kChunk - 1) / kChunk)), dim3(kThreads), 0, (hipStream_t)stream,
                     (const float *)w.saved, grad_scale_dev, total, grad_latents);
  return (int)hipGetLastError();
}

#if defined(GSGEN_EMU_KNOBS) && !defined(GSGEN_HW_FP16)  // the CPU emulator build of tests/test_guidance_host.py only
void gsgen_guidance_emu_constants(uint32_t *out) { out[0] = kPix; out[1] = kThreads; out[2] = kChunk; }
void gsgen_guidance_emu_f32_to_f16(const float *in, uint16_t *out, size_t count) {
  for (size_t i = 0; i < count; ++i) out[i] = f32_to_f16_bits(in[i]);
}
void gsgen_guidance_emu_f16_to_f32(const uint16_t *in, float *out, size_t count) {
  for (size_t i = 0; i < count; ++i) out[i] = f16_bits_to_f32(in[i]);
}
#endif

}  // extern "C"
