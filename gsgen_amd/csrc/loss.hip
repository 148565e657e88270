// loss.hip -- the fused SSIM + L1 / L2 image loss and its gradient to the rendered image, for gfx950 (compiled with
// -ffp-contract=off).
//
// Replaces utils/loss.py:7-47 of the reference,
//   ssim_weight * kornia.losses.ssim_loss(out, gt, window, reduction="mean") + (1 - ssim_weight) * {mse | l1}_loss(out, gt),
// which on the reference's side is five 11 x 11 conv2d calls and some twenty elementwise kernels forward and as many backward.
// kornia 0.6.0 is restated in DESIGN.md ("Image loss"); in short, with a = out, b = gt [B,H,W,C] fp32 channels last, p = (ws - 1) / 2:
//   g[i] = exp(-(i - ws/2)^2 / (2 * 1.5^2)) / sum;  filt(x) = per-channel correlation of reflect-padded x with g (x) g
//   mu1 = filt(a), mu2 = filt(b), e11 = filt(a a), e22 = filt(b b), e12 = filt(a b)
//   s1 = e11 - mu1^2, s2 = e22 - mu2^2, s12 = e12 - mu1 mu2, C1 = 1e-4, C2 = 9e-4
//   A1 = 2 mu1 mu2 + C1, A2 = 2 s12 + C2, B1 = mu1^2 + mu2^2 + C1, B2 = s1 + s2 + C2, s = A1 A2 / (B1 B2 + 1e-12)
//   loss = w * mean(clamp((1 - s) / 2, 0, 1)) + (1 - w) * mean((a - b)^2 | |a - b|)
//
// Kernels (a workgroup = kThreads = 512 threads owns one kTileH x kTileW = 32 x 32 pixel tile of one image, all channels; the
// shape was chosen by measurement among 32x32 / 16x64 / 16x32 tiles and 256 / 512 threads: DESIGN.md "Image loss"):
//   k_loss_fwd   stages a and b with a p-wide halo in LDS, the reflection resolved when the halo is loaded (so the filter loops have
//                no border case), then per channel: the five quantities filtered along rows into LDS, then along columns in
//                registers (every thread owns one column and kRows consecutive rows: kRows + ws - 1 LDS reads per quantity for
//                kRows outputs), s and the loss terms.  With want_grad it SAVES three derivative maps [B,H,W,C] (recomputing them in
//                the backward would repeat the whole forward, halo included, three pixels deep: 3 stores + 3 loads are cheaper):
//                  M1 = dL/dmu1 (total: with e11, e12 held fixed, i.e. including the paths through s1 and s12)
//                       = 2 k / D * (mu2 (A2 - A1) - s mu1 (B2 - B1)),  D = B1 B2 + 1e-12,  k = dL/ds = -w / (2 N) inside the clamp
//                  M2 = dL/de11 = -k s B1 / D
//                  M3 = dL/de12 + 2 dL/de11 = 2 k / D * (A1 - s B1)
//                M3 is stored in this combined form because the image gradient is
//                  filtT(M1) + 2 a filtT(dL/de11) + b filtT(dL/de12)  =  filtT(M1) + 2 (a - b) filtT(M2) + b filtT(M3):
//                for out == gt every bracket above is zero term by term (A1 == B1, A2 == B2 bit for bit), where the plain form
//                leaves the rounding of two cancelling products of the size of the gradient itself.
//                Per-workgroup sums of the two loss terms go to the workspace in fp64 (wave shuffles, then the waves in order).
//   k_loss_final one workgroup adds the partial sums in a fixed order in fp64 -> loss_out[3] = total, ssim term, base term (means).
//   k_loss_bwd   stages the three maps with a p-wide halo, ZERO outside the image, and applies filtT, the adjoint of
//                reflect-pad-then-correlate, separably: along an axis of n samples
//                  filtT(M)[u] = sum_k g[k] Mz[u + k - p]                       (Mz: M extended by zeros)
//                              + [1 <= u <= p]          sum_{m=0}^{p-u} g[p + u + m] M[m]            (taps the forward read at -1..-p)
//                              + [1 <= d <= p, d=n-1-u] sum_{m=0}^{p-d} g[p + d + m] M[n - 1 - m]    (taps read at n..n-1+p)
//                (n >= p + 1: a reflected index never bounces twice; both folds hit one u when n <= 2 p).  The folded sources lie
//                within p of the border and of u, so they are inside the tile's ordinary halo.  Then
//                  grad = *grad_scale * (F1 + 2 (a - b) F2 + b F3 + (1 - w) / N * (2 (a - b) | sign(a - b))).
//                The upstream scalar is read from device memory: no host synchronisation, and a captured replay sees its new value.
// No float atomics anywhere: loss and gradient are bit-identical from run to run.  Launch shapes depend on the sizes alone.
//
// -ffp-contract=off: every multiply-add of the filters is an explicit fmaf and nothing else is fused, so the g++ build of this
// file on the CPU emulator (tests/test_loss_host.py) performs the same fp32 operations in the same order as the GPU and its
// measured error against the fp64 definition is the GPU's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gsgen_hip.h"

#ifndef GSGEN_LOSS_TILE_H  // (tile and workgroup size are build constants: the A/B of DESIGN.md "Image loss" compiled this file five times)
#define GSGEN_LOSS_TILE_H 32
#endif
#ifndef GSGEN_LOSS_TILE_W
#define GSGEN_LOSS_TILE_W 32
#endif
#ifndef GSGEN_LOSS_THREADS
#define GSGEN_LOSS_THREADS 512
#endif

namespace gs_loss {

constexpr int kThreads = GSGEN_LOSS_THREADS;
constexpr int kWaves = kThreads / 64;
constexpr int kTileH = GSGEN_LOSS_TILE_H, kTileW = GSGEN_LOSS_TILE_W;
constexpr int kRows = kTileH * kTileW / kThreads;  // rows of one column a thread owns in the column pass
constexpr int kWsMax = 11;
static_assert(kTileH * kTileW % kThreads == 0 && kThreads % kTileW == 0 && kRows >= 1, "a thread owns kRows whole rows of one column");
static_assert(kTileH >= (kWsMax - 1) / 2 && kTileW >= (kWsMax - 1) / 2, "the folds assume a border tile holds its own reflected sources");

struct Taps { float g[kWsMax]; };

enum { kL2 = 0, kL1 = 1 };

// torch's reflect padding (the edge sample is not repeated), then clamped: a partial tile's halo reaches further out than p, where
// nothing that is used reads it
__device__ __forceinline__ int reflect_clamp(int t, int n) {
  t = t < 0 ? -t : t;
  t = t > n - 1 ? 2 * (n - 1) - t : t;
  return t < 0 ? 0 : (t > n - 1 ? n - 1 : t);
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

template <int WS, int C>
__global__ void __launch_bounds__(kThreads) k_loss_fwd(const float *__restrict__ a, const float *__restrict__ b, int H, int W, Taps taps,
                                                        float k_ssim, int base_kind, int want_grad, float *__restrict__ m1,
                                                        float *__restrict__ m2, float *__restrict__ m3, double *__restrict__ partials) {
  constexpr int P = (WS - 1) / 2, HR = kTileH + 2 * P, HW = (kTileW + 2 * P) * C;
  __shared__ float sA[HR][HW], sB[HR][HW];
  __shared__ float sH[5][HR][kTileW];
  __shared__ double sRed[kWaves][2];
  const int t = threadIdx.x, x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const size_t img = (size_t)blockIdx.z * H * W * C;
  float g[WS];
#pragma unroll
  for (int k = 0; k < WS; ++k) g[k] = taps.g[k];

  for (int i = t; i < HR * HW; i += kThreads) {
    const int ty = i / HW, tj = i % HW, tx = tj / C, c = tj % C;
    const size_t at = img + ((size_t)reflect_clamp(y0 - P + ty, H) * W + reflect_clamp(x0 - P + tx, W)) * C + c;
    sA[ty][tj] = a[at];
    sB[ty][tj] = b[at];
  }
  __syncthreads();

  const int x = t % kTileW, yy0 = (t / kTileW) * kRows, gx = x0 + x;
  float o1[kRows][C], o2[kRows][C], o3[kRows][C];
  double sum_ssim = 0.0, sum_base = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    // rows: the five filtered quantities of every halo row
    for (int i = t; i < HR * kTileW; i += kThreads) {
      const int r = i / kTileW, xx = i % kTileW;
      float f1 = 0.0f, f2 = 0.0f, f11 = 0.0f, f22 = 0.0f, f12 = 0.0f;
#pragma unroll
      for (int k = 0; k < WS; ++k) {
        const float va = sA[r][(xx + k) * C + c], vb = sB[r][(xx + k) * C + c];
        f1 = fmaf(g[k], va, f1);
        f2 = fmaf(g[k], vb, f2);
        f11 = fmaf(g[k], va * va, f11);
        f22 = fmaf(g[k], vb * vb, f22);
        f12 = fmaf(g[k], va * vb, f12);
      }
      sH[0][r][xx] = f1; sH[1][r][xx] = f2; sH[2][r][xx] = f11; sH[3][r][xx] = f22; sH[4][r][xx] = f12;
    }
    __syncthreads();
    // columns: kRows outputs of one column from kRows + WS - 1 rows
    float acc[kRows][5];
#pragma unroll
    for (int j = 0; j < kRows; ++j)
#pragma unroll
      for (int q = 0; q < 5; ++q) acc[j][q] = 0.0f;
#pragma unroll
    for (int r = 0; r < WS + kRows - 1; ++r) {
      float v[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) v[q] = sH[q][yy0 + r][x];
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        const int k = r - j;
        if (k >= 0 && k < WS) {
#pragma unroll
          for (int q = 0; q < 5; ++q) acc[j][q] = fmaf(g[k], v[q], acc[j][q]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      o1[j][c] = 0.0f; o2[j][c] = 0.0f; o3[j][c] = 0.0f;
      if (y0 + yy0 + j < H && gx < W) {
        const float mu1 = acc[j][0], mu2 = acc[j][1];
        const float mu1s = mu1 * mu1, mu2s = mu2 * mu2, mu12 = mu1 * mu2;
        const float s1 = acc[j][2] - mu1s, s2 = acc[j][3] - mu2s, s12 = acc[j][4] - mu12;
        const float A1 = 2.0f * mu12 + 1e-4f, A2 = 2.0f * s12 + 9e-4f, B1 = mu1s + mu2s + 1e-4f, B2 = s1 + s2 + 9e-4f;
        const float D = B1 * B2 + 1e-12f;
        const float s = A1 * A2 / D;
        const float l = (1.0f - s) * 0.5f;
        sum_ssim += (double)(l < 0.0f ? 0.0f : (l > 1.0f ? 1.0f : l));  // (a NaN stays a NaN: neither comparison holds)
        const float va = sA[yy0 + j + P][(x + P) * C + c], vb = sB[yy0 + j + P][(x + P) * C + c], d = va - vb;
        sum_base += (double)(base_kind == kL2 ? d * d : fabsf(d));
        const float k2 = (l < 0.0f || l > 1.0f) ? 0.0f : 2.0f * k_ssim / D;  // (torch's clamp passes the gradient on its bounds, and a NaN)
        o1[j][c] = k2 * (mu2 * (A2 - A1) - s * mu1 * (B2 - B1));
        o2[j][c] = -0.5f * k2 * (s * B1);
        o3[j][c] = k2 * (A1 - s * B1);
      }
    }
    __syncthreads();  // (sH is rewritten by the next channel)
  }
  if (want_grad) {
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      const int gy = y0 + yy0 + j;
      if (gy < H && gx < W) {
        const size_t at = img + ((size_t)gy * W + gx) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) { m1[at + c] = o1[j][c]; m2[at + c] = o2[j][c]; m3[at + c] = o3[j][c]; }
      }
    }
  }
  sum_ssim = wave_sum(sum_ssim);
  sum_base = wave_sum(sum_base);
  if ((t & 63) == 0) { sRed[t >> 6][0] = sum_ssim; sRed[t >> 6][1] = sum_base; }
  __syncthreads();
  if (t == 0) {
    double s0 = 0.0, s1 = 0.0;
    for (int w = 0; w < kWaves; ++w) { s0 += sRed[w][0]; s1 += sRed[w][1]; }
    const size_t wg = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partials[2 * wg] = s0;
    partials[2 * wg + 1] = s1;
  }
}

__global__ void __launch_bounds__(kThreads) k_loss_final(const double *__restrict__ partials, uint32_t n_wg, double inv_n, float ssim_weight,
                                                          float *__restrict__ loss_out) {
  __shared__ double sRed[kThreads][2];
  const int t = threadIdx.x;
  double s0 = 0.0, s1 = 0.0;
  for (uint32_t i = t; i < n_wg; i += kThreads) { s0 += partials[2 * (size_t)i]; s1 += partials[2 * (size_t)i + 1]; }
  sRed[t][0] = s0; sRed[t][1] = s1;
  __syncthreads();
  for (int d = kThreads / 2; d > 0; d >>= 1) {
    if (t < d) { sRed[t][0] += sRed[t + d][0]; sRed[t][1] += sRed[t + d][1]; }
    __syncthreads();
  }
  if (t == 0) {
    const double ssim = sRed[0][0] * inv_n, base = sRed[0][1] * inv_n, w = (double)ssim_weight;
    loss_out[0] = (float)(w * ssim + (1.0 - w) * base);
    loss_out[1] = (float)ssim;
    loss_out[2] = (float)base;
  }
}

template <int WS, int C>
__global__ void __launch_bounds__(kThreads) k_loss_bwd(const float *__restrict__ a, const float *__restrict__ b, int H, int W, Taps taps,
                                                        const float *__restrict__ m1, const float *__restrict__ m2,
                                                        const float *__restrict__ m3, float base_coef, int base_kind,
                                                        const float *__restrict__ grad_scale, float *__restrict__ grad) {
  constexpr int P = (WS - 1) / 2, HR = kTileH + 2 * P, HW = (kTileW + 2 * P) * C;
  __shared__ float sM[3][HR][HW];
  __shared__ float sH[3][HR][kTileW];
  __shared__ float sG[WS];
  const int t = threadIdx.x, x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const size_t img = (size_t)blockIdx.z * H * W * C;
  float g[WS];
#pragma unroll
  for (int k = 0; k < WS; ++k) g[k] = taps.g[k];
#pragma unroll
  for (int k = 0; k < WS; ++k)
    if (t == k) sG[k] = g[k];  // (the folds index the taps by position: from LDS, not from registers)

  for (int i = t; i < HR * HW; i += kThreads) {
    const int ty = i / HW, tj = i % HW, tx = tj / C, c = tj % C;
    const int gy = y0 - P + ty, gx = x0 - P + tx;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    const size_t at = in ? img + ((size_t)gy * W + gx) * C + c : 0;
    sM[0][ty][tj] = in ? m1[at] : 0.0f;
    sM[1][ty][tj] = in ? m2[at] : 0.0f;
    sM[2][ty][tj] = in ? m3[at] : 0.0f;
  }
  __syncthreads();

  const int x = t % kTileW, yy0 = (t / kTileW) * kRows, gx = x0 + x;
  const float scale = grad_scale[0];
  float og[kRows][C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    // rows
    for (int i = t; i < HR * kTileW; i += kThreads) {
      const int r = i / kTileW, xx = i % kTileW, u = x0 + xx;
      float f[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int k = 0; k < WS; ++k)
#pragma unroll
        for (int q = 0; q < 3; ++q) f[q] = fmaf(g[k], sM[q][r][(xx + k) * C + c], f[q]);
      if (u < W) {
        if (u >= 1 && u <= P)
          for (int m = 0; m <= P - u; ++m) {
            const float wt = sG[P + u + m];
            const int col = (m + P - x0) * C + c;
#pragma unroll
            for (int q = 0; q < 3; ++q) f[q] = fmaf(wt, sM[q][r][col], f[q]);
          }
        const int d = W - 1 - u;
        if (d >= 1 && d <= P)
          for (int m = 0; m <= P - d; ++m) {
            const float wt = sG[P + d + m];
            const int col = (W - 1 - m - x0 + P) * C + c;
#pragma unroll
            for (int q = 0; q < 3; ++q) f[q] = fmaf(wt, sM[q][r][col], f[q]);
          }
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) sH[q][r][xx] = f[q];
    }
    __syncthreads();
    // columns
    float acc[kRows][3];
#pragma unroll
    for (int j = 0; j < kRows; ++j)
#pragma unroll
      for (int q = 0; q < 3; ++q) acc[j][q] = 0.0f;
#pragma unroll
    for (int r = 0; r < WS + kRows - 1; ++r) {
      float v[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) v[q] = sH[q][yy0 + r][x];
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        const int k = r - j;
        if (k >= 0 && k < WS) {
#pragma unroll
          for (int q = 0; q < 3; ++q) acc[j][q] = fmaf(g[k], v[q], acc[j][q]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      const int u = y0 + yy0 + j;
      og[j][c] = 0.0f;
      if (u < H && gx < W) {
        if (u >= 1 && u <= P)
          for (int m = 0; m <= P - u; ++m) {
            const float wt = sG[P + u + m];
#pragma unroll
            for (int q = 0; q < 3; ++q) acc[j][q] = fmaf(wt, sH[q][m + P - y0][x], acc[j][q]);
          }
        const int d = H - 1 - u;
        if (d >= 1 && d <= P)
          for (int m = 0; m <= P - d; ++m) {
            const float wt = sG[P + d + m];
#pragma unroll
            for (int q = 0; q < 3; ++q) acc[j][q] = fmaf(wt, sH[q][H - 1 - m - y0 + P][x], acc[j][q]);
          }
        const size_t at = img + ((size_t)u * W + gx) * C + c;
        const float va = a[at], vb = b[at], df = va - vb;
        const float db = base_kind == kL2 ? 2.0f * df : (df > 0.0f ? 1.0f : (df < 0.0f ? -1.0f : df));  // (sign(0) = 0; a NaN stays)
        og[j][c] = scale * (acc[j][0] + 2.0f * df * acc[j][1] + vb * acc[j][2] + base_coef * db);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < kRows; ++j) {
    const int gy = y0 + yy0 + j;
    if (gy < H && gx < W) {
      const size_t at = img + ((size_t)gy * W + gx) * C;
#pragma unroll
      for (int c = 0; c < C; ++c) grad[at + c] = og[j][c];
    }
  }
}

// --- host side ---------------------------------------------------------------------------------------------------------
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// 0: fine
inline int check_sizes(uint32_t B, uint32_t H, uint32_t W, uint32_t C, uint32_t ws) {
  if (ws > (uint32_t)kWsMax || (C != 1 && C != 3)) return GSGEN_EUNSUPPORTED;
  if (ws < 3 || ws % 2 == 0) return GSGEN_EINVAL;
  if ((uint64_t)B * H * W == 0) return 0;
  const uint32_t p = (ws - 1) / 2;
  if (H < p + 1 || W < p + 1 || H > 0x3fffffffu || W > 0x3fffffffu) return GSGEN_EINVAL;
  if (B > 65535u || (H + kTileH - 1) / kTileH > 65535u) return GSGEN_EUNSUPPORTED;  // (grid.z, grid.y)
  return 0;
}

struct LossWs {
  double *partials;  // [n_wg][2]
  float *m1, *m2, *m3;  // [B,H,W,C] each (want_grad)
  uint32_t n_wg, tiles_x, tiles_y;
  size_t bytes;
};

inline LossWs carve_loss(void *base, uint32_t B, uint32_t H, uint32_t W, uint32_t C, bool want_grad) {
  char *p0 = (char *)base, *p = p0 + ((256 - ((uintptr_t)p0 & 255)) & 255);
  LossWs w;
  w.tiles_x = (W + kTileW - 1) / kTileW;
  w.tiles_y = (H + kTileH - 1) / kTileH;
  w.n_wg = w.tiles_x * w.tiles_y * B;
  size_t off = 0;
  auto take = [&](size_t b) { char *r = p + off; off += align256(b); return r; };
  w.partials = (double *)take(sizeof(double) * 2 * (size_t)w.n_wg);
  const size_t map = want_grad ? sizeof(float) * (size_t)B * H * W * C : 0;
  w.m1 = (float *)take(map); w.m2 = (float *)take(map); w.m3 = (float *)take(map);
  w.bytes = off + 256;
  return w;
}

inline Taps make_taps(uint32_t ws) {
  Taps t;
  double e[kWsMax], sum = 0.0;
  for (uint32_t i = 0; i < (uint32_t)kWsMax; ++i) t.g[i] = 0.0f;
  for (uint32_t i = 0; i < ws; ++i) {
    const double d = (double)i - (double)(ws / 2);
    e[i] = exp(-d * d / (2.0 * 1.5 * 1.5));
    sum += e[i];
  }
  for (uint32_t i = 0; i < ws; ++i) t.g[i] = (float)(e[i] / sum);
  return t;
}

template <int WS, int C>
inline void launch_fwd(dim3 grid, hipStream_t s, const float *a, const float *b, int H, int W, const Taps &taps, float k_ssim, int base_kind,
                       int want_grad, const LossWs &w) {
  hipLaunchKernelGGL((k_loss_fwd<WS, C>), grid, dim3(kThreads), 0, s, a, b, H, W, taps, k_ssim, base_kind, want_grad, w.m1, w.m2, w.m3,
                     w.partials);
}

template <int WS, int C>
inline void launch_bwd(dim3 grid, hipStream_t s, const float *a, const float *b, int H, int W, const Taps &taps, const LossWs &w,
                       float base_coef, int base_kind, const float *grad_scale, float *grad) {
  hipLaunchKernelGGL((k_loss_bwd<WS, C>), grid, dim3(kThreads), 0, s, a, b, H, W, taps, (const float *)w.m1, (const float *)w.m2,
                     (const float *)w.m3, base_coef, base_kind, grad_scale, grad);
}

#define GS_LOSS_DISPATCH(FN, ...)                                                      \
  do {                                                                                 \
    if (C == 3) {                                                                      \
      switch (ws) {                                                                    \
        case 3: FN<3, 3>(__VA_ARGS__); break;                                          \
        case 5: FN<5, 3>(__VA_ARGS__); break;                                          \
        case 7: FN<7, 3>(__VA_ARGS__); break;                                          \
        case 9: FN<9, 3>(__VA_ARGS__); break;                                          \
        default: FN<11, 3>(__VA_ARGS__); break;                                        \
      }                                                                                \
    } else {                                                                           \
      switch (ws) {                                                                    \
        case 3: FN<3, 1>(__VA_ARGS__); break;                                          \
        case 5: FN<5, 1>(__VA_ARGS__); break;                                          \
        case 7: FN<7, 1>(__VA_ARGS__); break;                                          \
        case 9: FN<9, 1>(__VA_ARGS__); break;                                          \
        default: FN<11, 1>(__VA_ARGS__); break;                                        \
      }                                                                                \
    }                                                                                  \
  } while (0)

}  // namespace gs_loss

using namespace gs_loss;

extern "C" {

size_t gsgen_image_loss_workspace_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t C, uint32_t ws, int want_grad) {
  if (check_sizes(B, H, W, C, ws) != 0) return 0;
  return carve_loss(nullptr, B, H, W, C, want_grad != 0).bytes;
}

int gsgen_image_loss_forward(const float *out, const float *gt, uint32_t B, uint32_t H, uint32_t W, uint32_t C, uint32_t ws,
                             float ssim_weight, int base_kind, int want_grad, float *loss_out, void *workspace, size_t workspace_bytes,
                             gsgen_stream_t stream) {
  if (int e = check_sizes(B, H, W, C, ws)) return e;
  if (base_kind != kL2 && base_kind != kL1) return GSGEN_EUNSUPPORTED;
  if ((uint64_t)B * H * W == 0) return 0;
  if (!out || !gt || !loss_out || !workspace) return GSGEN_EINVAL;
  const LossWs w = carve_loss(workspace, B, H, W, C, want_grad != 0);
  if (w.bytes > workspace_bytes) return GSGEN_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const double n = (double)B * H * W * C;
  const Taps taps = make_taps(ws);
  const float k_ssim = (float)(-0.5 * (double)ssim_weight / n);
  const dim3 grid(w.tiles_x, w.tiles_y, B);
  GS_LOSS_DISPATCH(launch_fwd, grid, s, out, gt, (int)H, (int)W, taps, k_ssim, base_kind, want_grad != 0, w);
  hipLaunchKernelGGL(k_loss_final, dim3(1), dim3(kThreads), 0, s, (const double *)w.partials, w.n_wg, 1.0 / n, ssim_weight, loss_out);
  return (int)hipGetLastError();
}

int gsgen_image_loss_backward(const float *out, const float *gt, uint32_t B, uint32_t H, uint32_t W, uint32_t C, uint32_t ws,
                              float ssim_weight, int base_kind, const float *grad_scale_dev, float *grad_out_image, void *workspace,
                              size_t workspace_bytes, gsgen_stream_t stream) {
  if (int e = check_sizes(B, H, W, C, ws)) return e;
  if (base_kind != kL2 && base_kind != kL1) return GSGEN_EUNSUPPORTED;
  if ((uint64_t)B * H * W == 0) return 0;
  if (!out || !gt || !grad_scale_dev || !grad_out_image || !workspace) return GSGEN_EINVAL;
  const LossWs w = carve_loss(workspace, B, H, W, C, true);
  if (w.bytes > workspace_bytes) return GSGEN_EWORKSPACE;
  const double n = (double)B * H * W * C;
  const Taps taps = make_taps(ws);
  const float base_coef = (float)((1.0 - (double)ssim_weight) / n);
  const dim3 grid(w.tiles_x, w.tiles_y, B);
  GS_LOSS_DISPATCH(launch_bwd, grid, (hipStream_t)stream, out, gt, (int)H, (int)W, taps, w, base_coef, base_kind, grad_scale_dev,
                   grad_out_image);
  return (int)hipGetLastError();
}

#if defined(GSGEN_EMU_KNOBS)  // the CPU emulator build of tests/test_loss_host.py only
// filtT alone: grad = filtT(map) for one [H,W,C] map (M2 = M3 = 0, no base term, scale 1); scratch: 2 * H * W * C floats
int gsgen_image_loss_emu_filt_adjoint(const float *map, uint32_t H, uint32_t W, uint32_t C, uint32_t ws, float *grad, float *scratch) {
  if (int e = check_sizes(1, H, W, C, ws)) return e;
  const size_t n = (size_t)H * W * C;
  for (size_t i = 0; i < 2 * n; ++i) scratch[i] = 0.0f;
  LossWs w;
  w.m1 = (float *)map; w.m2 = scratch; w.m3 = scratch;
  const float one = 1.0f;
  const Taps taps = make_taps(ws);
  const dim3 grid((W + kTileW - 1) / kTileW, (H + kTileH - 1) / kTileH, 1);
  GS_LOSS_DISPATCH(launch_bwd, grid, (hipStream_t) nullptr, scratch + n, scratch + n, (int)H, (int)W, taps, w, 0.0f, kL2, &one, grad);
  return 0;
}
void gsgen_image_loss_emu_constants(uint32_t *out) { out[0] = kTileH; out[1] = kTileW; out[2] = kThreads; out[3] = kWsMax; }
#endif

}  // extern "C"
