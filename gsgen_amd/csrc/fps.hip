// fps.hip -- exact farthest point sampling for gfx950 (compiled with -ffp-contract=off).
//
// Replaces pytorch3d's sample_farthest_points as utils/ops.py:76-100 calls it (guidance/point_e.py:120-127, :169-179 in every step;
// utils/initialize.py:379, utils/viewer/pcd.py:183), which does not exist for ROCm.
//
// The rule (one cloud points[L, D], a start s0, K picks):
//   idx[0] = s0 (the lowest-index finite point when s0 is out of range or not finite); m[p] = +inf for every finite point;
//   after pick s: m[p] = min(m[p], d2(p, s)), d2 = sum over the D coordinates of (p_c - s_c)^2, left to right in fp32 without
//   contraction, so an fp32 NumPy loop reproduces every bit; the next pick is the point of the largest m, ties to the lowest index:
//   the maximum of the 64-bit key  float_bits(m) << 32 | (0xFFFFFFFF - index)  (m >= 0: the integer order is the (m, -index) order,
//   and no two points share a key, so no internal order can show in the result).  Key 0 stands for "no point".
//   A point with a NaN / Inf coordinate, or past lengths[b], is never picked; entries past the number of pickable points are -1.
//   Once every remaining m is 0 (exact duplicates) the rule picks the lowest index again; that is not special-cased.
//
// Two kernels, both ONE workgroup of 1024 threads per start (16 wavefronts on one compute unit; farthest point sampling is
// sequential in K, and no workgroup ever waits for another: whatever crosses workgroups crosses a kernel boundary):
//   k_fps_brute<D, REG>  D = 3 or 6.  Thread t owns points t, t + 1024, ...; m stays in registers while L <= 1024 * kRegPoints
//                        (REG), else in the workspace.  Per pick: every owned point's d2 from global memory (coalesced, the cloud is
//                        L2-resident), the thread's best key, a wave reduction in registers, one 16-slot LDS exchange in which each
//                        wave's winner also deposits its coordinates, so the new pick's coordinates are broadcast from LDS.  Two
//                        alternating slots: one barrier per pick.
//   k_fps_bucket         D = 3, pruned and still exact.  The cloud is counting-sorted into at most 4096 spatial buckets by knn.hip's
//                        index (knn_index.hpp: robust box, cubic cells, outlier bucket, non-finite bucket, sorted float4 copy);
//                        k_fps_bucket_box takes each bucket's bounding box from its actual members.  Each thread owns at most 4
//                        bucket records in registers (box, the bucket's best key).  Per pick: (1) owners test
//                        lower_bound_d2(pick, box) < m_max(bucket) and put the buckets that pass into an LDS list (ballot + prefix);
//                        (2) wavefronts take the list's entries in turn, lanes stride over the bucket's points in the sorted copy,
//                        update m (workspace, indexed by sorted position, written only where it decreased) and reduce the bucket's
//                        new best key into an LDS table; (3) owners reload their keys and a workgroup maximum gives the next pick.
//                        Exactness: the box holds every member, and fp32 subtraction, multiplication and addition round
//                        monotonically, so the bound -- the same expression on the per-axis gaps -- is <= the d2 the update would
//                        compute for any member; it is shrunk by a relative margin on top.  A bucket with bound >= m_max >= m[p]
//                        for all its members cannot change.  The outlier bucket simply has a large box; the non-finite bucket is
//                        never touched.  A shared cloud (cloud_stride == 0) is indexed once for all starts.
// Launch shapes depend on the sizes only; starts, lengths and point values are read on the device: a captured call replays on new
// values in the same buffers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gsgen_hip.h"
#define GSGEN_INDEX_NS gs_fps_index
#include "knn_index.hpp"

namespace gs_fps {

using namespace gs_fps_index;
typedef unsigned long long u64;

constexpr int kThreads = 1024;          // one workgroup per start
constexpr int kWaves = kThreads / 64;
constexpr int kRegPoints = 16;          // brute: m in registers while L <= kThreads * kRegPoints
constexpr uint32_t kBucketsMax = 4096;  // bucket: cells + the outlier bucket + the non-finite bucket
constexpr int kOwned = kBucketsMax / kThreads;
constexpr uint32_t kMinPerCell = 16;    // points per cell the cell budget aims at, at least
// auto: the bucket kernel for D = 3 from this many points.  Measured on the MI355X ("Farthest point sampling"): the
// smallest power of two from which the bucket kernel wins on both the cfg2-like and the clustered cloud.
constexpr uint32_t kAutoBucketMin = 65536;
constexpr float kInf = __builtin_huge_valf();
constexpr float kBoundShrink = 0.99999f;  // relative margin on the pruning bound (on top of the monotone-rounding argument)

__host__ __device__ inline uint32_t fps_cell_cap(uint32_t L) {
  uint32_t per = (L + (kBucketsMax - 3)) / (kBucketsMax - 2);
  per = per < kMinPerCell ? kMinPerCell : per;
  const uint32_t c = L / per;
  return c < 1u ? 1u : c;  // <= kBucketsMax - 2
}

__device__ __forceinline__ u64 make_key(float m, uint32_t i) { return ((u64)__float_as_uint(m) << 32) | (u64)(0xffffffffu - i); }
__device__ __forceinline__ uint32_t key_index(u64 k) { return 0xffffffffu - (uint32_t)(k & 0xffffffffull); }
__device__ __forceinline__ float key_m(u64 k) { return __uint_as_float((uint32_t)(k >> 32)); }

__device__ __forceinline__ u64 wave_max(u64 k) {
  for (int d = 32; d > 0; d >>= 1) {
    const u64 o = __shfl_xor(k, d);
    k = o > k ? o : k;
  }
  return k;
}

template <int D>
__device__ __forceinline__ bool finite_row(const float *p) {
  bool f = true;
#pragma unroll
  for (int c = 0; c < D; ++c) f = f && fabsf(p[c]) <= 3.402823466e38f;  // (NaN fails the comparison)
  return f;
}

template <int D>
struct Slot {
  u64 key[kWaves];
  float c[kWaves][D];
};

// The workgroup's maximum of `key` and the coordinates q of the point it names, through slot (the caller alternates two slots, so
// one barrier per call suffices).  Keys of distinct points are distinct: exactly one lane of a wave holds the wave's non-zero maximum.
template <int D>
__device__ __forceinline__ u64 block_pick(u64 key, const float *__restrict__ pts, Slot<D> &slot, float (&q)[D]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const u64 wk = wave_max(key);
  if (wk == key && key != 0) {
    const float *p = pts + (size_t)D * key_index(key);
#pragma unroll
    for (int c = 0; c < D; ++c) slot.c[w][c] = p[c];
  }
  if (lane == 0) slot.key[w] = wk;
  __syncthreads();
  u64 best = 0;
  int bw = 0;
#pragma unroll
  for (int k = 0; k < kWaves; ++k) {
    const u64 o = slot.key[k];
    if (o > best) { best = o; bw = k; }
  }
#pragma unroll
  for (int c = 0; c < D; ++c) q[c] = slot.c[bw][c];
  return best;
}

__device__ __forceinline__ uint32_t valid_length(const int32_t *__restrict__ lengths, uint32_t b, uint32_t L) {
  if (!lengths) return L;
  const int32_t v = lengths[b];
  return v <= 0 ? 0u : ((uint32_t)v < L ? (uint32_t)v : L);
}

template <int D>
__device__ __forceinline__ float dist2(const float *__restrict__ p, const float (&q)[D]) {
  float d2 = 0.0f;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    const float d = p[c] - q[c];
    d2 = c == 0 ? d * d : d2 + d * d;
  }
  return d2;
}

// --- the brute kernel ------------------------------------------------------------------------------------------------
// m < 0 marks a point that is never picked (non-finite, or past the cloud's length): fminf keeps it there (also against a NaN d2)
// and no such m ever exceeds the running best.
template <int D, bool REG>
__global__ void __launch_bounds__(kThreads) k_fps_brute(const float *__restrict__ points, uint32_t L, size_t cloud_stride,
                                                         const int32_t *__restrict__ lengths, const int32_t *__restrict__ start_idx,
                                                         uint32_t K, int32_t *__restrict__ idx_out, float *__restrict__ m_ws) {
  __shared__ Slot<D> slot[2];
  __shared__ uint32_t s_nfin;
  const uint32_t t = threadIdx.x, b = blockIdx.x;
  const float *pts = points + (size_t)b * cloud_stride;
  const uint32_t n = valid_length(lengths, b, L);
  int32_t *out = idx_out + (size_t)b * K;
  float *mg = REG ? nullptr : m_ws + (size_t)b * L;
  float m[REG ? kRegPoints : 1];
  if (t == 0) s_nfin = 0;
  __syncthreads();
  uint32_t cnt = 0, first = 0xffffffffu;
  if (REG) {
#pragma unroll
    for (int r = 0; r < kRegPoints; ++r) {
      const uint32_t i = t + (uint32_t)r * kThreads;
      const bool ok = i < n && finite_row<D>(pts + (size_t)D * (i < n ? i : 0));
      m[r] = ok ? kInf : -1.0f;
      if (ok) { ++cnt; first = first == 0xffffffffu ? i : first; }
    }
  } else {
    for (uint32_t i = t; i < L; i += kThreads) {
      const bool ok = i < n && finite_row<D>(pts + (size_t)D * i);
      mg[i] = ok ? kInf : -1.0f;
      if (ok) { ++cnt; first = first == 0xffffffffu ? i : first; }
    }
  }
  if (cnt) atomicAdd(&s_nfin, cnt);
  __syncthreads();
  const uint32_t npick = s_nfin < K ? s_nfin : K;
  for (uint32_t k = npick + t; k < K; k += kThreads) out[k] = -1;
  if (npick == 0) return;

  float q[D];
  uint32_t cur;
  int par = 0;
  const int32_t s0 = start_idx[b];
  if (s0 >= 0 && (uint32_t)s0 < n && finite_row<D>(pts + (size_t)D * (uint32_t)s0)) {
    cur = (uint32_t)s0;
#pragma unroll
    for (int c = 0; c < D; ++c) q[c] = pts[(size_t)D * cur + c];
  } else {  // the lowest-index finite point: the maximum key at m = +inf everywhere
    cur = key_index(block_pick<D>(first == 0xffffffffu ? 0ull : make_key(kInf, first), pts, slot[par], q));
    par ^= 1;
  }
  for (uint32_t k = 0; k < npick; ++k) {
    if (t == 0) out[k] = (int32_t)cur;
    if (k + 1 == npick) break;
    float bm = -1.0f;
    uint32_t bi = 0;
    if (REG) {
#pragma unroll
      for (int r = 0; r < kRegPoints; ++r) {
        const uint32_t i = t + (uint32_t)r * kThreads;
        const float d2 = dist2<D>(pts + (size_t)D * (i < L ? i : L - 1), q);
        m[r] = fminf(m[r], d2);
        if (m[r] > bm) { bm = m[r]; bi = i; }  // (ascending i: the lowest index of equal m stays)
      }
    } else {
      for (uint32_t i = t; i < L; i += kThreads) {
        float mv = mg[i];
        const float d2 = dist2<D>(pts + (size_t)D * i, q);
        if (d2 < mv) { mv = d2; mg[i] = d2; }
        if (mv > bm) { bm = mv; bi = i; }
      }
    }
    cur = key_index(block_pick<D>(bm >= 0.0f ? make_key(bm, bi) : 0ull, pts, slot[par], q));
    par ^= 1;
  }
}

// --- the bucket kernel -----------------------------------------------------------------------------------------------
// box[2 c] = (min x, min y, min z, -), box[2 c + 1] = (max x, max y, max z, -) over the members of bucket c (cells, then the outlier
// bucket); an empty bucket keeps an inverted box and is never flagged (its key is 0).  One wavefront per bucket.
__global__ void __launch_bounds__(256) k_fps_bucket_box(uint32_t nb, const uint32_t *__restrict__ start, const float4 *__restrict__ sorted,
                                                         float4 *__restrict__ box) {
  const uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= nb) return;  // (a whole wavefront)
  float lo[3] = {3.402823466e38f, 3.402823466e38f, 3.402823466e38f}, hi[3] = {-3.402823466e38f, -3.402823466e38f, -3.402823466e38f};
  const uint32_t e = start[c + 1];
  for (uint32_t j = start[c] + lane; j < e; j += 64) {
    const float4 p = sorted[j];
    lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
    hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
  }
  for (int d = 32; d > 0; d >>= 1)
    for (int a = 0; a < 3; ++a) {
      lo[a] = fminf(lo[a], __shfl_xor(lo[a], d));
      hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], d));
    }
  if (lane == 0) {
    box[2 * (size_t)c] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    box[2 * (size_t)c + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
  }
}

#if defined(GSGEN_EMU_KNOBS)  // the CPU emulator build of tests/test_fps_host.py only: buckets visited per pick (start 0)
static uint32_t g_emu_visits[4096];
static uint32_t g_emu_nonempty;
#endif

// a lower bound of d2(p, q) over the points p of the box: the update's own expression on the per-axis gaps (see the header)
__device__ __forceinline__ float box_bound(const float (&q)[3], const float (&lo)[3], const float (&hi)[3]) {
  float g[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) g[a] = fmaxf(fmaxf(lo[a] - q[a], q[a] - hi[a]), 0.0f);
  return (g[0] * g[0] + g[1] * g[1] + g[2] * g[2]) * kBoundShrink;
}

// nb buckets can be flagged (cells + outliers <= kBucketsMax - 1).  index_stride / box_stride: bytes / float4s between the indexes
// of consecutive starts (0: one index for all).
__global__ void __launch_bounds__(kThreads) k_fps_bucket(const float *__restrict__ points, uint32_t L, size_t cloud_stride,
                                                          const int32_t *__restrict__ lengths, const int32_t *__restrict__ start_idx,
                                                          uint32_t K, int32_t *__restrict__ idx_out, uint32_t nb,
                                                          const uint32_t *__restrict__ start0, const float4 *__restrict__ sorted0,
                                                          size_t index_stride, const float4 *__restrict__ box0, size_t box_stride,
                                                          float *__restrict__ m_ws) {
  __shared__ u64 table[kBucketsMax];
  __shared__ uint16_t list[kBucketsMax];
  __shared__ Slot<3> slot[2];
  __shared__ uint32_t cursor[2];
  __shared__ uint32_t s_nfin;
  const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.x;
  const float *pts = points + (size_t)b * cloud_stride;
  const uint32_t n = valid_length(lengths, b, L);
  int32_t *out = idx_out + (size_t)b * K;
  const uint32_t *start = (const uint32_t *)((const char *)start0 + (size_t)b * index_stride);
  const float4 *sorted = (const float4 *)((const char *)sorted0 + (size_t)b * index_stride);
  const float4 *box = box0 + (size_t)b * box_stride;
  float *m = m_ws + (size_t)b * L;  // by sorted position

  if (t == 0) { cursor[0] = 0; cursor[1] = 0; s_nfin = 0; }
  __syncthreads();
  // m = +inf and every bucket's first key: (+inf, its lowest pickable index)
  uint32_t cnt = 0;
  for (uint32_t c = wave; c < nb; c += kWaves) {
    const uint32_t e = start[c + 1];
    uint32_t lo_i = 0xffffffffu;
    for (uint32_t j = start[c] + lane; j < e; j += 64) {
      const uint32_t orig = __float_as_uint(sorted[j].w);
      if (orig < n) {
        m[j] = kInf;
        lo_i = orig < lo_i ? orig : lo_i;
        ++cnt;
      }
    }
    for (int d = 32; d > 0; d >>= 1) {
      const uint32_t o = __shfl_xor(lo_i, d);
      lo_i = o < lo_i ? o : lo_i;
    }
    if (lane == 0) table[c] = lo_i == 0xffffffffu ? 0ull : make_key(kInf, lo_i);
  }
  if (cnt) atomicAdd(&s_nfin, cnt);
  __syncthreads();
  const uint32_t npick = s_nfin < K ? s_nfin : K;
  for (uint32_t k = npick + t; k < K; k += kThreads) out[k] = -1;
  if (npick == 0) return;

  float blo[kOwned][3], bhi[kOwned][3];
  u64 okey[kOwned];
  u64 key = 0;
#pragma unroll
  for (int j = 0; j < kOwned; ++j) {
    const uint32_t c = t + (uint32_t)j * kThreads;
    okey[j] = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) { blo[j][a] = 0.0f; bhi[j][a] = 0.0f; }
    if (c < nb) {
      const float4 l4 = box[2 * (size_t)c], h4 = box[2 * (size_t)c + 1];
      blo[j][0] = l4.x; blo[j][1] = l4.y; blo[j][2] = l4.z;
      bhi[j][0] = h4.x; bhi[j][1] = h4.y; bhi[j][2] = h4.z;
      okey[j] = table[c];
    }
    key = okey[j] > key ? okey[j] : key;
  }
#if defined(GSGEN_EMU_KNOBS)
  if (t == 0 && b == 0) {
    g_emu_nonempty = 0;
    for (uint32_t c = 0; c < nb; ++c) g_emu_nonempty += table[c] != 0;
    for (int k = 0; k < 4096; ++k) g_emu_visits[k] = 0;
  }
#endif

  float q[3];
  uint32_t cur;
  int par = 0;
  const int32_t s0 = start_idx[b];
  if (s0 >= 0 && (uint32_t)s0 < n && finite_row<3>(pts + 3 * (size_t)(uint32_t)s0)) {
    cur = (uint32_t)s0;
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = pts[3 * (size_t)cur + c];
  } else {
    cur = key_index(block_pick<3>(key, pts, slot[par], q));
    par ^= 1;
  }
  for (uint32_t k = 0; k < npick; ++k) {
    if (t == 0) out[k] = (int32_t)cur;
    if (k + 1 == npick) break;
    const int cp = (int)(k & 1);
    // 1. the buckets this pick can change
#pragma unroll
    for (int j = 0; j < kOwned; ++j) {
      const uint32_t c = t + (uint32_t)j * kThreads;
      const bool f = c < nb && okey[j] != 0 && box_bound(q, blo[j], bhi[j]) < key_m(okey[j]);
      const u64 mask = __ballot(f);
      uint32_t base = 0;
      if (lane == 0 && mask) base = atomicAdd(&cursor[cp], (uint32_t)__popcll(mask));
      base = __shfl(base, 0);
      if (f) list[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (uint16_t)c;
    }
    if (t == 0) cursor[cp ^ 1] = 0;  // (last read before the previous pick's second barrier, next written after this pick's)
    __syncthreads();
    // 2. wavefronts take the flagged buckets in turn
    const uint32_t nflag = cursor[cp];
#if defined(GSGEN_EMU_KNOBS)
    if (t == 0 && b == 0 && k < 4096) g_emu_visits[k] = nflag;
#endif
    for (uint32_t f = wave; f < nflag; f += kWaves) {
      const uint32_t c = list[f], e = start[c + 1];
      u64 bk = 0;
      for (uint32_t j = start[c] + lane; j < e; j += 64) {
        const float4 p = sorted[j];
        const uint32_t orig = __float_as_uint(p.w);
        if (orig < n) {
          const float pv[3] = {p.x, p.y, p.z};
          const float d2 = dist2<3>(pv, q);
          float mv = m[j];
          if (d2 < mv) { mv = d2; m[j] = d2; }
          const u64 pk = make_key(mv, orig);
          bk = pk > bk ? pk : bk;
        }
      }
      bk = wave_max(bk);
      if (lane == 0) table[c] = bk;
    }
    __syncthreads();
    // 3. owners reload, the workgroup's maximum is the next pick
    key = 0;
#pragma unroll
    for (int j = 0; j < kOwned; ++j) {
      const uint32_t c = t + (uint32_t)j * kThreads;
      if (c < nb) okey[j] = table[c];
      key = okey[j] > key ? okey[j] : key;
    }
    cur = key_index(block_pick<3>(key, pts, slot[par], q));
    par ^= 1;
  }
}

// --- host side ---------------------------------------------------------------------------------------------------------
enum { kAuto = 0, kBrute = 1, kBucket = 2 };

// 0: unsupported pair
inline int route(uint32_t L, uint32_t dim, int method) {
  if (dim != 3 && dim != 6) return 0;
  if (method == kBrute) return kBrute;
  if (method == kBucket) return dim == 3 ? kBucket : 0;
  if (method == kAuto) return (dim == 3 && L >= kAutoBucketMin) ? kBucket : kBrute;
  return 0;
}

struct FpsWs {
  float *m;        // brute beyond the register size: [n_starts, L]; bucket: [n_starts, L]
  char *index;     // bucket: n_starts indexes, index_bytes apart (a shared cloud uses the first)
  float4 *box;     // bucket: [n_starts, 2 * (cap + 1)]
  size_t index_bytes, bytes;
};

inline FpsWs carve_fps(void *base, uint32_t L, uint32_t n_starts, int routed) {
  char *p0 = (char *)base, *p = p0 + ((256 - ((uintptr_t)p0 & 255)) & 255);
  FpsWs w;
  size_t off = 0;
  auto take = [&](size_t b) { char *r = p + off; off += align256(b); return r; };
  w.m = nullptr; w.index = nullptr; w.box = nullptr; w.index_bytes = 0;
  if (routed == kBucket) {
    const uint32_t cap = fps_cell_cap(L);
    w.index_bytes = align256(carve_cap(nullptr, L, cap).bytes);
    w.m = (float *)take(sizeof(float) * (size_t)n_starts * L);
    w.index = take(w.index_bytes * n_starts);
    w.box = (float4 *)take(sizeof(float4) * 2 * (size_t)(cap + 1) * n_starts);
  } else if (L > (uint32_t)kThreads * kRegPoints) {
    w.m = (float *)take(sizeof(float) * (size_t)n_starts * L);
  }
  w.bytes = off + 256;
  return w;
}

template <int D>
inline void launch_brute(bool reg, uint32_t n_starts, const float *points, uint32_t L, size_t stride, const int32_t *lengths,
                         const int32_t *start_idx, uint32_t K, int32_t *idx_out, float *m, hipStream_t s) {
  if (reg)
    hipLaunchKernelGGL((k_fps_brute<D, true>), dim3(n_starts), dim3(kThreads), 0, s, points, L, stride, lengths, start_idx, K, idx_out, m);
  else
    hipLaunchKernelGGL((k_fps_brute<D, false>), dim3(n_starts), dim3(kThreads), 0, s, points, L, stride, lengths, start_idx, K, idx_out, m);
}

}  // namespace gs_fps

using namespace gs_fps;

extern "C" {

size_t gsgen_fps_workspace_bytes(uint32_t n_points, uint32_t dim, uint32_t n_starts, uint32_t K, int method) {
  const int routed = route(n_points, dim, method);
  if (!routed || n_points == 0 || n_points > 0x7fffffffu || n_starts == 0 || K == 0) return 0;
  return carve_fps(nullptr, n_points, n_starts, routed).bytes;
}

int gsgen_fps(const float *points, uint32_t n_points, uint32_t dim, size_t cloud_stride, const int32_t *lengths, const int32_t *start_idx,
              uint32_t n_starts, uint32_t K, int32_t *idx_out, void *workspace, size_t workspace_bytes, int method,
              gsgen_stream_t stream) {
  const int routed = route(n_points, dim, method);
  if (!routed) return GSGEN_EUNSUPPORTED;
  if (K == 0 || n_points == 0 || n_points > 0x7fffffffu || n_starts == 0) return GSGEN_EINVAL;
  if (!points || !start_idx || !idx_out || !workspace) return GSGEN_EINVAL;
  const uint32_t L = n_points;
  const FpsWs w = carve_fps(workspace, L, n_starts, routed);
  if (w.bytes > workspace_bytes) return GSGEN_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (routed == kBrute) {
    const bool reg = L <= (uint32_t)kThreads * kRegPoints;
    if (dim == 3) launch_brute<3>(reg, n_starts, points, L, cloud_stride, lengths, start_idx, K, idx_out, w.m, s);
    else launch_brute<6>(reg, n_starts, points, L, cloud_stride, lengths, start_idx, K, idx_out, w.m, s);
    return (int)hipGetLastError();
  }
  const uint32_t cap = fps_cell_cap(L), nb = cap + 1, n_index = cloud_stride == 0 ? 1u : n_starts;
  Ws first = carve_cap(w.index, L, cap);
  for (uint32_t i = 0; i < n_index; ++i) {
    const Ws wi = carve_cap(w.index + (size_t)i * w.index_bytes, L, cap);
    if (int e = build_index_cap(points + (size_t)i * cloud_stride, L, cap, wi, s)) return e;
    hipLaunchKernelGGL(k_fps_bucket_box, dim3((nb + 3) / 4), dim3(256), 0, s, nb, (const uint32_t *)wi.start, (const float4 *)wi.sorted,
                       w.box + 2 * (size_t)nb * i);
  }
  hipLaunchKernelGGL(k_fps_bucket, dim3(n_starts), dim3(kThreads), 0, s, points, L, cloud_stride, lengths, start_idx, K, idx_out, nb,
                     (const uint32_t *)first.start, (const float4 *)first.sorted, n_index == 1 ? (size_t)0 : w.index_bytes,
                     (const float4 *)w.box, n_index == 1 ? (size_t)0 : 2 * (size_t)nb, w.m);
  return (int)hipGetLastError();
}

#if defined(GSGEN_EMU_KNOBS)
// -> the number of non-empty pickable buckets of the last bucket call's start 0 (a full scan's visits per pick); out[k] = buckets
// visited by the update after pick k
uint32_t gsgen_fps_emu_visits(uint32_t *out, uint32_t n) {
  for (uint32_t k = 0; k < n && k < 4096; ++k) out[k] = g_emu_visits[k];
  return g_emu_nonempty;
}
void gsgen_fps_emu_constants(uint32_t *out) {
  out[0] = kThreads; out[1] = kRegPoints; out[2] = kBucketsMax; out[3] = kAutoBucketMin;
}
#endif

}  // extern "C"
