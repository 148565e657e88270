// map_loss.hip -- the regularisers of the text-to-3D training step on the rendered opacity and depth-variance maps, and their
// gradients, for gfx950 (compiled with -ffp-contract=off).
//
// Replaces trainer.py:345-382 of the reference (with utils/ops.py:51-55 for the second term), three torch expressions of some twenty
// elementwise and reduction launches forward and as many backward:
//   sparsity : mean( sqrt(opacity^2 + 0.01) )
//   opague   : c = clamp(opacity, 1e-3, 1 - 1e-3);  mean( -(c log c + (1 - c) log(1 - c)) )     (binary_cross_entropy(c, c))
//   z_var    : c as above;                          mean( z_var / c * (c > 0.5) )
// DESIGN.md ("Map regularisers") has the definition; in short, per pixel i of the P = B H W pixels, in fp32, o = opacity, v = z_var:
//   lo = float(1e-3), hi = float(1.0 - 1e-3) (the fp32 values torch.clamp compares with),  c = o < lo ? lo : (o > hi ? hi : o) (a NaN
//   stays),  in = (o >= lo) && (o <= hi) (the bounds pass the gradient, as torch.clamp does),  m = c > 0.5f,
//   s = sqrtf(o o + 0.01f)                       ds/do = o / s
//   e = -(c logf(c) + (1 - c) logf(1 - c))       de/do = in (logf(1 - c) - logf(c))     (the derivative through `target`: the one
//                                                                                        through `input` is 1 - 1 = 0 identically)
//   z = (v / c) m  (a product with 0 / 1, not a select: a non-finite v under m == 0 gives NaN, as in torch)
//                                                dz/dv = m / c,  dz/do = -in m v / c^2
//   T_k = (1 / P) sum_i,  total = w_s T_s + w_o T_o + w_z T_z,  d total / d o_i = (g / P)(w_s ds + w_o de + w_z dz),  g the upstream
//   scalar.  Pixels meet only in the means: a non-finite pixel makes the terms that read it non-finite and no other pixel's gradient.
//
// Kernels (a workgroup = kThreads = 256 threads owns one chunk of kChunk = 2048 consecutive pixels; grid = chunks):
//   k_map_fwd    a lane owns kVec = 2 groups of four consecutive pixels, group (j kThreads + t) of the chunk: a wave's load is 1 KB
//                contiguous.  A whole group is ONE 16-byte load from a pointer that need only be 4-byte aligned -- the global load of
//                four dwords takes any dword address, so a view whose data_ptr() sits 4, 8 or 12 bytes off takes the same loads, and
//                pixel -> lane does not move with the base address: the sums, and so the loss, have the same bits at every offset.
//                (A scalar head would shift the groups with the address and the bits with them.)  Only the last, ragged group of
//                the map is read pixel by pixel.  Only the terms of the host's bit mask are evaluated -- the branch is uniform, so
//                with the opague term off no log is issued, and without the z_var term z_var is not read.  Per-pixel arithmetic is
//                fp32; a lane adds its eight values in fp64, then wave shuffles, then the waves in order: one partial of three
//                doubles per workgroup goes to the workspace (a masked-off term's is 0).
//   k_map_final  one workgroup: thread t adds partials t, t + 256, ... in order, then the wave, then the waves, in fp64; T_k = sum / P,
//                total from the weights (three kernel arguments, or float[3] in device memory: a captured step replays with the next
//                step's scheduled weights) -> out[0] = total, out[1..3] = T_s, T_o, T_z (0 for a masked-off term).
//   k_map_bwd    one elementwise pass, recomputing from the inputs (nothing image-sized is saved): grad_opacity and grad_z_var, either
//                may be null.  The upstream scalar and the device weights are read from device memory: no host synchronisation.
// Chunk and occupancy: this is a stream of 8 bytes per pixel with a sqrt, a divide and two logs on it -- at 4 x 512^2 about 2 us of
// HBM time and as much of VALU time, under the launch latency either way.  Two 16-byte loads per map per lane keep four loads in
// flight per lane and amortise the ~40 cross-lane fp64 adds of the block reduction over eight pixels instead of four; 2048 pixels
// per workgroup is 512 workgroups at 4 x 512^2 (two per CU, eight waves per CU) and 2500 at 8 x 800^2, and the kernels need few
// registers (no arrays beyond the eight pixels), so occupancy is limited by the grid alone.  A 4096 chunk would leave one workgroup
// per CU at the flagship size; a 1024 chunk doubles the reduction's share.  The final stage sums at most a few thousand partials.
// No float atomics, no fill: the workspace may arrive dirty and unaligned (every word read was written by the launch before).
// Loss and gradients are bit-identical from run to run.  Launch shapes depend on P alone.
//
// -ffp-contract=off: nothing is fused, so the g++ build of this file on the CPU emulator (tests/test_map_loss_host.py) performs
// the GPU's operations in the GPU's order (logf is each platform's own: both are within an ulp).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsgen_hip.h"

namespace gs_map {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kVec = 2;                         // groups of four pixels a lane owns
constexpr int kChunk = kThreads * kVec * 4;     // pixels a workgroup reduces
constexpr int kTerms = 3;                       // doubles per workgroup partial
constexpr uint32_t kSparsity = 1u, kOpague = 2u, kZVar = 4u;

// four consecutive floats at any dword address: one 16-byte load or store
struct alignas(4) F4 { float v[4]; };

__device__ __forceinline__ F4 load4(const float *__restrict__ p, size_t i, int n) {
  if (n == 4) return *(const F4 *)(p + i);
  F4 r;
#pragma unroll
  for (int k = 0; k < 4; ++k) r.v[k] = k < n ? p[i + k] : 0.0f;
  return r;
}

__device__ __forceinline__ void store4(float *__restrict__ p, size_t i, int n, const F4 &g) {
  if (n == 4) { *(F4 *)(p + i) = g; return; }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < n) p[i + k] = g.v[k];
}

// how many of the four pixels from i on lie inside the map
__device__ __forceinline__ int live_pixels(size_t i, uint32_t P) { return i >= (size_t)P ? 0 : ((size_t)P - i < 4 ? (int)((size_t)P - i) : 4); }

__device__ __forceinline__ float clamp_c(float o, float lo, float hi) { return o < lo ? lo : (o > hi ? hi : o); }  // (a NaN stays)

__device__ __forceinline__ double wave_sum(double v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

__global__ void __launch_bounds__(kThreads) k_map_fwd(const float *__restrict__ opacity, const float *__restrict__ z_var, uint32_t P,
                                                       uint32_t terms, double *__restrict__ partials) {
  __shared__ double sRed[kWaves][kTerms];
  const int t = threadIdx.x;
  const size_t c0 = (size_t)blockIdx.x * kChunk;
  const float lo = (float)1e-3, hi = (float)(1.0 - 1e-3);

  F4 o[kVec], v[kVec] = {};
  int n[kVec];
#pragma unroll
  for (int j = 0; j < kVec; ++j) {
    const size_t i = c0 + (size_t)(j * kThreads + t) * 4;
    n[j] = live_pixels(i, P);
    o[j] = load4(opacity, i, n[j]);
    if (terms & kZVar) v[j] = load4(z_var, i, n[j]);
  }
  double ss = 0.0, se = 0.0, sz = 0.0;
#pragma unroll
  for (int j = 0; j < kVec; ++j) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < n[j]) {
        const float x = o[j].v[k], c = clamp_c(x, lo, hi);
        if (terms & kSparsity) ss += (double)sqrtf(x * x + 0.01f);
        if (terms & kOpague) se += (double)(-(c * logf(c) + (1.0f - c) * logf(1.0f - c)));
        if (terms & kZVar) sz += (double)((v[j].v[k] / c) * (c > 0.5f ? 1.0f : 0.0f));
      }
    }
  }
  ss = wave_sum(ss); se = wave_sum(se); sz = wave_sum(sz);
  if ((t & 63) == 0) {
    double *r = sRed[t >> 6];
    r[0] = ss; r[1] = se; r[2] = sz;
  }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < kWaves; ++w) {
      const double *r = sRed[w];
      ss += r[0]; se += r[1]; sz += r[2];
    }
    double *p = partials + (size_t)kTerms * blockIdx.x;
    p[0] = ss; p[1] = se; p[2] = sz;
  }
}

__global__ void __launch_bounds__(kThreads) k_map_final(const double *__restrict__ partials, uint32_t n_chunks, uint32_t P, uint32_t terms,
                                                         float w_s, float w_o, float w_z, const float *__restrict__ weights_dev,
                                                         float *__restrict__ out) {
  __shared__ double sRed[kWaves][kTerms];
  const int t = threadIdx.x;
  double a[kTerms] = {0.0, 0.0, 0.0};
  for (uint32_t c = t; c < n_chunks; c += kThreads) {
    const double *p = partials + (size_t)kTerms * c;
    a[0] += p[0]; a[1] += p[1]; a[2] += p[2];
  }
#pragma unroll
  for (int k = 0; k < kTerms; ++k) a[k] = wave_sum(a[k]);
  if ((t & 63) == 0) {
    double *r = sRed[t >> 6];
    r[0] = a[0]; r[1] = a[1]; r[2] = a[2];
  }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < kWaves; ++w) {
      const double *r = sRed[w];
      a[0] += r[0]; a[1] += r[1]; a[2] += r[2];
    }
    if (weights_dev) { w_s = weights_dev[0]; w_o = weights_dev[1]; w_z = weights_dev[2]; }
    const double w[kTerms] = {(double)w_s, (double)w_o, (double)w_z};
    double total = 0.0;
    for (int k = 0; k < kTerms; ++k) {
      const bool on = terms >> k & 1u;
      const double T = a[k] / (double)P;
      if (on) total += w[k] * T;
      out[1 + k] = on ? (float)T : 0.0f;
    }
    out[0] = (float)total;
  }
}

__global__ void __launch_bounds__(kThreads) k_map_bwd(const float *__restrict__ opacity, const float *__restrict__ z_var, uint32_t P,
                                                       uint32_t terms, float w_s, float w_o, float w_z,
                                                       const float *__restrict__ weights_dev, const float *__restrict__ grad_scale,
                                                       float *__restrict__ grad_opacity, float *__restrict__ grad_z_var) {
  const int t = threadIdx.x;
  const size_t c0 = (size_t)blockIdx.x * kChunk;
  const float lo = (float)1e-3, hi = (float)(1.0 - 1e-3);
  if (weights_dev) { w_s = weights_dev[0]; w_o = weights_dev[1]; w_z = weights_dev[2]; }
  const double gp = (double)grad_scale[0] / (double)P;
  const float ks = (float)(gp * (double)w_s), ko = (float)(gp * (double)w_o), kz = (float)(gp * (double)w_z);  // (one rounding each)

  F4 o[kVec], v[kVec] = {};
  int n[kVec];
#pragma unroll
  for (int j = 0; j < kVec; ++j) {
    const size_t i = c0 + (size_t)(j * kThreads + t) * 4;
    n[j] = live_pixels(i, P);
    o[j] = load4(opacity, i, n[j]);
    if (terms & kZVar) v[j] = load4(z_var, i, n[j]);
  }
#pragma unroll
  for (int j = 0; j < kVec; ++j) {
    if (n[j] == 0) continue;
    const size_t i = c0 + (size_t)(j * kThreads + t) * 4;
    F4 go, gv;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float x = o[j].v[k], c = clamp_c(x, lo, hi);
      const bool in = x >= lo && x <= hi;
      float g = 0.0f, gz = 0.0f;
      if (terms & kSparsity) g = ks * (x / sqrtf(x * x + 0.01f));
      if (terms & kOpague) g = g + ko * (in ? logf(1.0f - c) - logf(c) : 0.0f);
      if (terms & kZVar) {
        const float m = c > 0.5f ? 1.0f : 0.0f;
        gz = kz * (m / c);
        g = g + kz * (in ? -(m * v[j].v[k]) / (c * c) : 0.0f);
      }
      go.v[k] = g;
      gv.v[k] = gz;
    }
    if (grad_opacity) store4(grad_opacity, i, n[j], go);
    if (grad_z_var) store4(grad_z_var, i, n[j], gv);
  }
}

// --- host side ---------------------------------------------------------------------------------------------------------
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct MapWs {
  double *partials;  // [n_chunks][kTerms]
  uint32_t n_chunks;
  size_t bytes;
};

inline MapWs carve_map(void *base, uint32_t P) {
  char *p0 = (char *)base, *p = p0 + ((256 - ((uintptr_t)p0 & 255)) & 255);
  MapWs w;
  w.n_chunks = (uint32_t)(((uint64_t)P + kChunk - 1) / kChunk);
  w.partials = (double *)p;
  w.bytes = align256(sizeof(double) * kTerms * (size_t)w.n_chunks) + 256;
  return w;
}

// the checks the two entry points share; 1: nothing to do
inline int check_map(const float *opacity, const float *z_var, uint32_t P, uint32_t terms, const float *weights_host,
                     const float *weights_dev, void *workspace, size_t workspace_bytes) {
  if (P == 0) return 1;
  if (!opacity || !workspace || (!weights_host && !weights_dev)) return GSGEN_EINVAL;
  if ((terms & ~7u) || ((terms & kZVar) && !z_var)) return GSGEN_EINVAL;
  if (carve_map(workspace, P).bytes > workspace_bytes) return GSGEN_EWORKSPACE;
  return 0;
}

}  // namespace gs_map

using namespace gs_map;

extern "C" {

size_t gsgen_map_loss_workspace_bytes(uint32_t n_pixels) { return carve_map(nullptr, n_pixels).bytes; }

int gsgen_map_loss_forward(const float *opacity, const float *z_var, uint32_t n_pixels, uint32_t terms_mask, const float *weights_host,
                           const float *weights_dev, float *loss_out, void *workspace, size_t workspace_bytes, gsgen_stream_t stream) {
  const int rc = check_map(opacity, z_var, n_pixels, terms_mask, weights_host, weights_dev, workspace, workspace_bytes);
  if (rc) return rc > 0 ? 0 : rc;
  if (!loss_out) return GSGEN_EINVAL;
  const MapWs w = carve_map(workspace, n_pixels);
  const float ws = weights_host ? weights_host[0] : 0.0f, wo = weights_host ? weights_host[1] : 0.0f, wz = weights_host ? weights_host[2] : 0.0f;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_map_fwd, dim3(w.n_chunks), dim3(kThreads), 0, s, opacity, z_var, n_pixels, terms_mask, w.partials);
  hipLaunchKernelGGL(k_map_final, dim3(1), dim3(kThreads), 0, s, (const double *)w.partials, w.n_chunks, n_pixels, terms_mask, ws, wo, wz,
                     weights_dev, loss_out);
  return (int)hipGetLastError();
}

int gsgen_map_loss_backward(const float *opacity, const float *z_var, uint32_t n_pixels, uint32_t terms_mask, const float *weights_host,
                            const float *weights_dev, const float *grad_scale_dev, float *grad_opacity, float *grad_z_var, void *workspace,
                            size_t workspace_bytes, gsgen_stream_t stream) {
  const int rc = check_map(opacity, z_var, n_pixels, terms_mask, weights_host, weights_dev, workspace, workspace_bytes);
  if (rc) return rc > 0 ? 0 : rc;
  if (!grad_scale_dev) return GSGEN_EINVAL;
  if (!grad_opacity && !grad_z_var) return 0;
  const MapWs w = carve_map(workspace, n_pixels);
  const float ws = weights_host ? weights_host[0] : 0.0f, wo = weights_host ? weights_host[1] : 0.0f, wz = weights_host ? weights_host[2] : 0.0f;
  hipLaunchKernelGGL(k_map_bwd, dim3(w.n_chunks), dim3(kThreads), 0, (hipStream_t)stream, opacity, z_var, n_pixels, terms_mask, ws, wo, wz,
                     weights_dev, grad_scale_dev, grad_opacity, grad_z_var);
  return (int)hipGetLastError();
}

#if defined(GSGEN_EMU_KNOBS)  // the CPU emulator build of tests/test_map_loss_host.py only
void gsgen_map_loss_emu_constants(uint32_t *out) { out[0] = kChunk; out[1] = kThreads; out[2] = kTerms; }  // ([1]: partials per final-stage sweep)
#endif

}  // extern "C"
