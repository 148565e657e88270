// knn_index.hpp -- the spatial index over a point cloud that knn.hip's searches and fps.hip's bucket sampler share: steps 1-3 of
// knn.hip's header (robust box, cubic cells, outlier bucket, non-finite bucket, the sorted float4 (x, y, z, original index) copy).
// Included with quotes from the file beside it.  The kernels are defined in the namespace GSGEN_INDEX_NS (default gs_knn), one
// name per translation unit that includes this file: two objects of one library must not define the same kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef GSGEN_INDEX_NS
#define GSGEN_INDEX_NS gs_knn
#endif

namespace GSGEN_INDEX_NS {

constexpr int kBlock = 256;
constexpr int kBins = 1024;        // histogram bins per axis and pass
constexpr int kMaxBlocks = 256;    // partial-reduction blocks (bbox, histograms)
constexpr int kScanTile = 1024;    // entries per block of the scan (256 threads x 4)
constexpr float kTrim = 0.01f;     // robust box: 1 % / 99 % quantiles per axis ...
constexpr float kWiden = 0.25f;    // ... widened by a quarter of their distance on each side
constexpr uint32_t kMaxDim = 1024; // cells per axis at most
constexpr unsigned long long kPad = (0x7f800000ull << 32) | 0xffffffffull;  // (+inf, index -1)

struct Params {
  float lo[3], hi[3], ext[3];  // grid box: min corner, max corner, extent
  float blo[3], bhi[3];     // bounding box of the finite points
  float h, inv_h;           // cubic cell side
  uint32_t dim[3];          // cells per axis (dim[0] * dim[1] * dim[2] <= cap)
  uint32_t below[3];        // finite points below the first pass's selected range, per axis
  uint32_t n_finite;
  float hlo[3], hhi[3];     // the range the current histogram pass covers, per axis
};

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  // (NaN fails every comparison; |inf| > FLT_MAX)
  return fabsf(x) <= 3.402823466e38f && fabsf(y) <= 3.402823466e38f && fabsf(z) <= 3.402823466e38f;
}

__host__ __device__ inline uint32_t points_per_cell(uint32_t K) { return K <= 8 ? 2u : K / 4u; }
__host__ __device__ inline uint32_t cell_cap(uint32_t N, uint32_t K) {
  const uint32_t c = N / points_per_cell(K);
  return c < 1u ? 1u : c;
}
__host__ __device__ inline uint32_t reduce_blocks(uint32_t N) {
  const uint32_t b = (N + kBlock - 1) / kBlock;
  return b < 1u ? 1u : (b > (uint32_t)kMaxBlocks ? (uint32_t)kMaxBlocks : b);
}

// --- 1. bounding box of the finite points ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock) k_knn_bbox(uint32_t N, const float *__restrict__ pts, float *__restrict__ part) {
  __shared__ float s[6][kBlock];
  __shared__ uint32_t sc[kBlock];
  float mn[3] = {3.402823466e38f, 3.402823466e38f, 3.402823466e38f}, mx[3] = {-3.402823466e38f, -3.402823466e38f, -3.402823466e38f};
  uint32_t cnt = 0;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) {
    const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    if (!finite3(x, y, z)) continue;
    mn[0] = fminf(mn[0], x); mn[1] = fminf(mn[1], y); mn[2] = fminf(mn[2], z);
    mx[0] = fmaxf(mx[0], x); mx[1] = fmaxf(mx[1], y); mx[2] = fmaxf(mx[2], z);
    ++cnt;
  }
  for (int a = 0; a < 3; ++a) { s[a][threadIdx.x] = mn[a]; s[3 + a][threadIdx.x] = mx[a]; }
  sc[threadIdx.x] = cnt;
  __syncthreads();
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      for (int a = 0; a < 3; ++a) {
        s[a][threadIdx.x] = fminf(s[a][threadIdx.x], s[a][threadIdx.x + w]);
        s[3 + a][threadIdx.x] = fmaxf(s[3 + a][threadIdx.x], s[3 + a][threadIdx.x + w]);
      }
      sc[threadIdx.x] += sc[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    for (int a = 0; a < 6; ++a) part[8 * blockIdx.x + a] = s[a][0];
    part[8 * blockIdx.x + 6] = __uint_as_float(sc[0]);
  }
}

// -> params: histogram range of the first pass = the bounding box, n_finite
__global__ void __launch_bounds__(64) k_knn_bbox_final(uint32_t nb, const float *__restrict__ part, Params *__restrict__ P) {
  if (threadIdx.x != 0) return;
  float mn[3] = {3.402823466e38f, 3.402823466e38f, 3.402823466e38f}, mx[3] = {-3.402823466e38f, -3.402823466e38f, -3.402823466e38f};
  uint32_t cnt = 0;
  for (uint32_t b = 0; b < nb; ++b) {
    for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], part[8 * b + a]); mx[a] = fmaxf(mx[a], part[8 * b + 3 + a]); }
    cnt += __float_as_uint(part[8 * b + 6]);
  }
  for (int a = 0; a < 3; ++a) {
    if (cnt == 0) { mn[a] = 0.0f; mx[a] = 0.0f; }
    P->hlo[a] = P->blo[a] = mn[a];
    P->hhi[a] = P->bhi[a] = mx[a];
    P->below[a] = 0;
  }
  P->n_finite = cnt;
}

// --- 2. robust box: histogram of each axis over [hlo, hhi] -----------------------------------------------------------
__device__ __forceinline__ int hist_bin(float v, float lo, float hi) {
  // -1 below the range, kBins above it; the top edge belongs to the last bin
  if (v < lo) return -1;
  if (v > hi) return kBins;
  const float w = hi - lo;
  if (!(w > 0.0f)) return 0;
  const float f = (v - lo) / w * (float)kBins;
  return f >= (float)(kBins - 1) ? kBins - 1 : (int)f;
}

__global__ void __launch_bounds__(kBlock) k_knn_hist(uint32_t N, const float *__restrict__ pts, const Params *__restrict__ P,
                                                      uint32_t *__restrict__ hist) {
  __shared__ uint32_t s[3 * kBins];
  for (int b = threadIdx.x; b < 3 * kBins; b += kBlock) s[b] = 0;
  __syncthreads();
  float lo[3], hi[3];
  for (int a = 0; a < 3; ++a) { lo[a] = P->hlo[a]; hi[a] = P->hhi[a]; }
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < N; i += gridDim.x * kBlock) {
    const float v[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
    if (!finite3(v[0], v[1], v[2])) continue;
    for (int a = 0; a < 3; ++a) {
      const int b = hist_bin(v[a], lo[a], hi[a]);
      if (b >= 0 && b < kBins) atomicAdd(&s[a * kBins + b], 1u);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < 3 * kBins; b += kBlock)
    if (s[b]) atomicAdd(&hist[b], s[b]);
}

// One wave per axis finds the bins of ranks r_lo and r_hi (counted from the lowest finite point: `below` of them lie under the
// histogram's range) and narrows [hlo, hhi] to those bins.  final != 0: that range is the robust box; size the grid.
__global__ void __launch_bounds__(192) k_knn_select(const uint32_t *__restrict__ hist, Params *__restrict__ P, uint32_t cap,
                                                     int final) {
  __shared__ uint32_t lane_sum[3][64];
  __shared__ float box_lo[3], box_hi[3];
  const int a = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t *hb = hist + a * kBins;
  constexpr int per = kBins / 64;
  uint32_t sum = 0;
  for (int k = 0; k < per; ++k) sum += hb[lane * per + k];
  lane_sum[a][lane] = sum;
  __syncthreads();
  if (lane == 0) {
    const uint32_t n = P->n_finite, trim = (uint32_t)((float)n * kTrim);
    const uint32_t below = P->below[a];
    const uint32_t r_lo = trim, r_hi = n > trim ? n - 1 - trim : 0;
    // bin holding rank r (cumulative count from the lowest finite point); clamps to the first / last bin
    int bins[2];
    uint32_t below_lo = below;
    for (int q = 0; q < 2; ++q) {
      const uint32_t r = q ? r_hi : r_lo;
      uint32_t run = below;
      int seg = 0;
      while (seg < 63 && run + lane_sum[a][seg] <= r) { run += lane_sum[a][seg]; ++seg; }
      int b = seg * per;
      while (b < seg * per + per - 1 && run + hb[b] <= r) { run += hb[b]; ++b; }
      if (r < below) { b = 0; run = below; }  // (cannot happen for r_lo >= below: kept for safety)
      bins[q] = b;
      if (q == 0) below_lo = run;
    }
    const float lo = P->hlo[a], hi = P->hhi[a], w = (hi - lo) / (float)kBins;
    float nlo = lo + (float)bins[0] * w, nhi = (bins[1] + 1 >= kBins) ? hi : lo + (float)(bins[1] + 1) * w;
    if (nhi < nlo) nhi = nlo;
    if (final) {  // the grid box: the quantile box widened by kWiden of its extent per side, within the bounding box
      const float wd = (nhi - nlo) * kWiden;
      nlo = fmaxf(nlo - wd, P->blo[a]);
      nhi = fminf(nhi + wd, P->bhi[a]);
    }
    box_lo[a] = nlo;
    box_hi[a] = nhi;
    if (!final) {
      P->hlo[a] = nlo;
      P->hhi[a] = nhi;
      P->below[a] = below_lo;
    }
  }
  __syncthreads();
  if (!final || threadIdx.x != 0) return;
  // the coarsest cubic cell with dim[0] * dim[1] * dim[2] <= cap (geometric bisection on the side)
  double ext[3], emax = 0.0;
  for (int k = 0; k < 3; ++k) {
    ext[k] = (double)box_hi[k] - (double)box_lo[k];
    emax = ext[k] > emax ? ext[k] : emax;
  }
  float h = 1.0f;
  uint32_t dim[3] = {1, 1, 1};
  if (emax > 0.0) {
    auto cells = [&](double side, uint32_t *d) {
      double t = 1.0;
      for (int k = 0; k < 3; ++k) {
        double c = ceil(ext[k] / side);
        c = c < 1.0 ? 1.0 : (c > (double)kMaxDim ? (double)kMaxDim : c);
        if (d) d[k] = (uint32_t)c;
        t *= c;
      }
      return t;
    };
    double s_hi = emax, s_lo = emax / (double)kMaxDim;
    if (cells(s_lo, nullptr) <= (double)cap) s_hi = s_lo;
    else
      for (int it = 0; it < 40; ++it) {
        const double mid = sqrt(s_lo * s_hi);
        if (cells(mid, nullptr) <= (double)cap) s_hi = mid; else s_lo = mid;
      }
    cells(s_hi, dim);
    h = (float)s_hi;
    if (!(h > 0.0f)) h = 1.0f;
  }
  for (int k = 0; k < 3; ++k) {
    P->lo[k] = box_lo[k];
    P->hi[k] = box_hi[k];
    P->ext[k] = box_hi[k] - box_lo[k];
    P->dim[k] = dim[k];
  }
  P->h = h;
  P->inv_h = 1.0f / h;
}

// --- 3. counting sort by cell ----------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t cell_coord(float v, float lo, float inv_h, uint32_t dim) {
  float f = (v - lo) * inv_h;  // (may be +-inf for a far outlier: clamped before the conversion)
  f = fminf(fmaxf(f, 0.0f), (float)(dim - 1));
  return (uint32_t)f;
}

__global__ void __launch_bounds__(kBlock) k_knn_count(uint32_t N, uint32_t cap, const float *__restrict__ pts,
                                                       const Params *__restrict__ P, uint32_t *__restrict__ cell_of,
                                                       uint32_t *__restrict__ counts) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
  uint32_t c = cap + 1;  // non-finite: the last bucket
  if (finite3(x, y, z) && !(x >= P->lo[0] && x <= P->hi[0] && y >= P->lo[1] && y <= P->hi[1] && z >= P->lo[2] && z <= P->hi[2])) {
    c = cap;  // outside the grid box: the outlier bucket after the last cell
  } else if (finite3(x, y, z)) {
    const float ih = P->inv_h;
    const uint32_t cx = cell_coord(x, P->lo[0], ih, P->dim[0]), cy = cell_coord(y, P->lo[1], ih, P->dim[1]),
                   cz = cell_coord(z, P->lo[2], ih, P->dim[2]);
    c = (cz * P->dim[1] + cy) * P->dim[0] + cx;
  }
  cell_of[i] = c;
  atomicAdd(&counts[c], 1u);
}

// inclusive scan of v over the 256 threads of the block (wave64 shuffles, then the four wave totals)
__device__ __forceinline__ uint32_t block_inclusive_scan(uint32_t v, uint32_t *wave_tot) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl(v, lane >= d ? lane - d : lane);
    if (lane >= d) v += o;
  }
  if (lane == 63) wave_tot[w] = v;
  __syncthreads();
  uint32_t off = 0;
  for (int k = 0; k < w; ++k) off += wave_tot[k];
  __syncthreads();
  return v + off;
}

__global__ void __launch_bounds__(kBlock) k_knn_scan_tiles(uint32_t M, const uint32_t *__restrict__ counts,
                                                            uint32_t *__restrict__ tile_sum) {
  __shared__ uint32_t wt[4];
  const uint32_t base = blockIdx.x * kScanTile + threadIdx.x * 4;
  uint32_t s = 0;
  for (int k = 0; k < 4; ++k) s += base + k < M ? counts[base + k] : 0u;
  const uint32_t inc = block_inclusive_scan(s, wt);
  if (threadIdx.x == kBlock - 1) tile_sum[blockIdx.x] = inc;
}

__global__ void __launch_bounds__(kBlock) k_knn_scan_sums(uint32_t T, uint32_t *__restrict__ tile_sum) {
  __shared__ uint32_t wt[4];
  __shared__ uint32_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint32_t t0 = 0; t0 < T; t0 += kBlock) {
    const uint32_t t = t0 + threadIdx.x;
    const uint32_t v = t < T ? tile_sum[t] : 0u;
    const uint32_t inc = block_inclusive_scan(v, wt);
    const uint32_t c = carry;
    if (t < T) tile_sum[t] = c + inc - v;  // exclusive
    __syncthreads();
    if (threadIdx.x == kBlock - 1) carry = c + inc;
    __syncthreads();
  }
}

// start[m] = exclusive scan of counts (m < M); cursor = start (the scatter's atomics advance it)
__global__ void __launch_bounds__(kBlock) k_knn_scan_apply(uint32_t M, const uint32_t *__restrict__ counts,
                                                            const uint32_t *__restrict__ tile_sum, uint32_t *__restrict__ start,
                                                            uint32_t *__restrict__ cursor) {
  __shared__ uint32_t wt[4];
  const uint32_t base = blockIdx.x * kScanTile + threadIdx.x * 4;
  uint32_t c[4], s = 0;
  for (int k = 0; k < 4; ++k) { c[k] = base + k < M ? counts[base + k] : 0u; s += c[k]; }
  uint32_t run = block_inclusive_scan(s, wt) - s + tile_sum[blockIdx.x];
  for (int k = 0; k < 4; ++k) {
    if (base + k < M) { start[base + k] = run; cursor[base + k] = run; }
    run += c[k];
  }
}

__global__ void __launch_bounds__(kBlock) k_knn_scatter(uint32_t N, const float *__restrict__ pts, const uint32_t *__restrict__ cell_of,
                                                         uint32_t *__restrict__ cursor, float4 *__restrict__ sorted) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const uint32_t pos = atomicAdd(&cursor[cell_of[i]], 1u);
  sorted[pos] = make_float4(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], __uint_as_float(i));
}

// --- workspace --------------------------------------------------------------------------------------------------------
struct Ws {
  Params *P;
  float *part;
  uint32_t *hist, *cell_of, *counts, *start, *cursor, *tile_sum;
  float4 *sorted;
  size_t bytes;
};

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// (cap: the cell budget; the searches derive it from N and K, cell_cap)
inline Ws carve_cap(void *base, uint32_t N, uint32_t cap) {
  const uint32_t M = cap + 3, T = (M + kScanTile - 1) / kScanTile;
  char *p0 = (char *)base, *p = p0 + ((256 - ((uintptr_t)p0 & 255)) & 255);
  Ws w;
  size_t off = 0;
  auto take = [&](size_t b) { char *r = p + off; off += align256(b); return r; };
  w.P = (Params *)take(sizeof(Params));
  w.part = (float *)take(sizeof(float) * 8 * kMaxBlocks);
  w.hist = (uint32_t *)take(sizeof(uint32_t) * 3 * kBins);
  w.cell_of = (uint32_t *)take(sizeof(uint32_t) * (size_t)N);
  w.counts = (uint32_t *)take(sizeof(uint32_t) * (size_t)M);
  w.start = (uint32_t *)take(sizeof(uint32_t) * (size_t)M);
  w.cursor = (uint32_t *)take(sizeof(uint32_t) * (size_t)M);
  w.tile_sum = (uint32_t *)take(sizeof(uint32_t) * (size_t)T);
  w.sorted = (float4 *)take(sizeof(float4) * (size_t)N);
  w.bytes = off + 256;  // (room for the leading alignment of any base address)
  return w;
}
inline Ws carve(void *base, uint32_t N, uint32_t K) { return carve_cap(base, N, cell_cap(N, K)); }

// steps 1-3: the index over `points` (launch shapes from N and K alone)
inline int build_index_cap(const float *points, uint32_t N, uint32_t cap, const Ws &w, hipStream_t s) {
  const uint32_t M = cap + 3, T = (M + kScanTile - 1) / kScanTile;
  const uint32_t nb = reduce_blocks(N), ng = (N + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(k_knn_bbox, dim3(nb), dim3(kBlock), 0, s, N, points, w.part);
  hipLaunchKernelGGL(k_knn_bbox_final, dim3(1), dim3(64), 0, s, nb, (const float *)w.part, w.P);
  for (int pass = 0; pass < 2; ++pass) {
    if (int e = (int)hipMemsetAsync(w.hist, 0, sizeof(uint32_t) * 3 * kBins, s)) return e;
    hipLaunchKernelGGL(k_knn_hist, dim3(nb), dim3(kBlock), 0, s, N, points, (const Params *)w.P, w.hist);
    hipLaunchKernelGGL(k_knn_select, dim3(1), dim3(192), 0, s, (const uint32_t *)w.hist, w.P, cap, pass);
  }
  if (int e = (int)hipMemsetAsync(w.counts, 0, sizeof(uint32_t) * (size_t)M, s)) return e;
  hipLaunchKernelGGL(k_knn_count, dim3(ng), dim3(kBlock), 0, s, N, cap, points, (const Params *)w.P, w.cell_of, w.counts);
  hipLaunchKernelGGL(k_knn_scan_tiles, dim3(T), dim3(kBlock), 0, s, M, (const uint32_t *)w.counts, w.tile_sum);
  hipLaunchKernelGGL(k_knn_scan_sums, dim3(1), dim3(kBlock), 0, s, T, w.tile_sum);
  hipLaunchKernelGGL(k_knn_scan_apply, dim3(T), dim3(kBlock), 0, s, M, (const uint32_t *)w.counts, (const uint32_t *)w.tile_sum,
                     w.start, w.cursor);
  hipLaunchKernelGGL(k_knn_scatter, dim3(ng), dim3(kBlock), 0, s, N, points, (const uint32_t *)w.cell_of, w.cursor, w.sorted);
  return 0;
}
inline int build_index(const float *points, uint32_t N, uint32_t K, const Ws &w, hipStream_t s) {
  return build_index_cap(points, N, cell_cap(N, K), w, s);
}

}  // namespace GSGEN_INDEX_NS
