// mesh_sample.hip -- a triangle mesh to an evenly spaced point cloud, for gfx950 (compiled with -ffp-contract=off): what the
// reference takes from trimesh (utils/mesh.py:52-69: sample_surface_even = area-weighted surface samples thinned by remove_close).
// DESIGN.md ("Mesh sampling") has the definitions and their reasons; in short:
//
// (a) Face weights.  w[f] = 0.5 * |(v1 - v0) x (v2 - v0)| in fp64 from the fp32 vertices (the differences, the cross product
//     (a_y b_z - a_z b_y, ...) and sqrt((c_x^2 + c_y^2) + c_z^2) all in fp64, nothing fused); 0 where the area is 0, a vertex is not
//     finite or a vertex index lies outside [0, V) (counted in bad_faces).  cum[] = the inclusive fp64 scan of w over three levels
//     (tiles of 1024 faces, 1024 tiles, one workgroup over the rest), total = cum[F - 1].
// (b) Sampling, one lane per sample, from uniforms (u_face, r1, r2) in [0, 1): pick = (double)u_face * total; the face is the first
//     i with cum[i] >= pick (binary search) and w[i] > 0 (a forward walk over zero-weight faces, which only pick = 0 on leading
//     zero-weight faces can need when cum is monotone); r1 + r2 > 1 (fp32 sum) -> both become 1 - r;
//     p = v0 + ((v1 - v0) * r1 + (v2 - v0) * r2) in fp32 in this order; attributes the same; the face normal is the fp64 cross
//     product over its fp64 length, rounded once.  total == 0: NaN everywhere, face -1, zero_area_flag = 1.
// (c) remove_close.  Keep point i iff no kept j < i has d2(i, j) <= r * r, d2 = (dx dx + dy dy) + dz dz in fp32, r * r one fp32
//     product: the greedy loop in index order.  A uniform grid over the bounding box of the finite points with cell side
//     h >= 1.0001 r (and >= 2^-60: below that fp32 squares underflow), enlarged until the cells fit the budget; cell coordinates
//     are floor(((double)v - (double)lo) / h), a monotone map under which two points the fp32 predicate accepts (at most
//     r (1 + 2^-22) apart per axis) differ by at most one cell, so the 27 surrounding cells hold every candidate.  r * r = +inf:
//     one cell.  Points are counting-sorted by cell with their index (knn_index.hpp's scan and scatter); non-finite points go to
//     a bucket of their own and are REMOVED from the start.  Then rounds, one launch each: an UNDECIDED point scans its lower-index
//     neighbours within r: one KEPT -> REMOVED; else none UNDECIDED -> KEPT; else it waits.  A decision is final and is the
//     greedy one whatever the round saw of its neighbours, so updating the state in place is sound; no workgroup waits for
//     another inside a launch.  Every round adds the points it leaves undecided to a counter, and a round that finds the previous
//     round's counter at 0 returns at once.
// No allocation, no host synchronisation, launch shapes from the sizes alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gsgen_hip.h"

#define GSGEN_INDEX_NS gs_ms_index  // (the scans and the scatter of the counting sort; one kernel namespace per translation unit)
#include "knn_index.hpp"

namespace gs_ms {

using gs_ms_index::align256;
using gs_ms_index::finite3;

constexpr int kBlock = 256;
constexpr int kPer = 4;
constexpr uint32_t kTile = kBlock * kPer;  // faces of one workgroup of the scan
constexpr uint32_t kMaxAttr = 8;

// in the workspace of gsgen_mesh_sample; the status block the caller gets is a copy
struct Status {
  uint32_t bad_faces, zero_area;
  double total;
};

// inclusive scan of v over the 256 threads of the block (wave64 shuffles, then the four wave totals)
__device__ __forceinline__ double block_inclusive_scan_f64(double v, double *wave_tot) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl(v, lane >= d ? lane - d : lane);
    if (lane >= d) v += o;
  }
  if (lane == 63) wave_tot[w] = v;
  __syncthreads();
  double off = 0.0;
  for (int k = 0; k < w; ++k) off += wave_tot[k];
  __syncthreads();
  return v + off;
}

// the weight of face f; p = its vertices, c = the fp64 cross product, len = its length (all valid only where the weight is > 0)
__device__ __forceinline__ double face_weight(const float *__restrict__ verts, uint32_t V, const int32_t *__restrict__ tris, uint32_t f,
                                              float p[3][3], double c[3], double *len, bool *bad) {
  const int32_t id[3] = {tris[3 * (size_t)f], tris[3 * (size_t)f + 1], tris[3 * (size_t)f + 2]};
  *bad = false;
  for (int k = 0; k < 3; ++k)
    if (id[k] < 0 || (uint32_t)id[k] >= V) *bad = true;
  if (*bad) return 0.0;
  for (int k = 0; k < 3; ++k)
    for (int m = 0; m < 3; ++m) p[k][m] = verts[3 * (size_t)id[k] + m];
  for (int k = 0; k < 3; ++k)
    if (!finite3(p[k][0], p[k][1], p[k][2])) return 0.0;
  double a[3], b[3];
  for (int m = 0; m < 3; ++m) {
    a[m] = (double)p[1][m] - (double)p[0][m];
    b[m] = (double)p[2][m] - (double)p[0][m];
  }
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
  *len = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
  const double w = 0.5 * *len;
  return w > 0.0 ? w : 0.0;
}

// cum[f] = w[f] (scanned by k_ms_apply), tile_sum[t] = the sum of tile t in the order k_ms_apply adds it
__global__ void __launch_bounds__(kBlock) k_ms_weights(const float *__restrict__ verts, uint32_t V, const int32_t *__restrict__ tris,
                                                        uint32_t F, double *__restrict__ cum, double *__restrict__ tile_sum,
                                                        Status *__restrict__ st) {
  __shared__ double wt[4];
  const uint32_t f0 = blockIdx.x * kTile + threadIdx.x * kPer;
  double s = 0.0;
  uint32_t nbad = 0;
  for (int k = 0; k < kPer; ++k) {
    if (f0 + k >= F) break;
    float p[3][3];
    double c[3], len;
    bool bad;
    const double w = face_weight(verts, V, tris, f0 + k, p, c, &len, &bad);
    nbad += bad ? 1u : 0u;
    cum[f0 + k] = w;
    s += w;
  }
  if (nbad) atomicAdd(&st->bad_faces, nbad);
  const double inc = block_inclusive_scan_f64(s, wt);
  if (threadIdx.x == kBlock - 1) tile_sum[blockIdx.x] = inc;
}

// APPLY false: super[b] = the sum of v[1024 b .. 1024 b + 1024);  true: v -> its exclusive scan in place, starting from super[b]
template <bool APPLY>
__global__ void __launch_bounds__(kBlock) k_ms_scan(uint32_t n, double *__restrict__ v, double *__restrict__ super) {
  __shared__ double wt[4];
  const uint32_t t0 = blockIdx.x * kTile + threadIdx.x * kPer;
  double x[kPer], s = 0.0;
  for (int k = 0; k < kPer; ++k) {
    x[k] = t0 + k < n ? v[t0 + k] : 0.0;
    s += x[k];
  }
  const double inc = block_inclusive_scan_f64(s, wt);
  if (APPLY) {
    double run = super[blockIdx.x] + (inc - s);
    for (int k = 0; k < kPer; ++k) {
      if (t0 + k < n) v[t0 + k] = run;
      run += x[k];
    }
  } else if (threadIdx.x == kBlock - 1) {
    super[blockIdx.x] = inc;
  }
}

// super[0 .. S) -> its exclusive scan (one workgroup)
__global__ void __launch_bounds__(kBlock) k_ms_scan_super(uint32_t S, double *__restrict__ super) {
  __shared__ double wt[4];
  __shared__ double carry;
  if (threadIdx.x == 0) carry = 0.0;
  __syncthreads();
  for (uint32_t b0 = 0; b0 < S; b0 += kBlock) {
    const uint32_t b = b0 + threadIdx.x;
    const double v = b < S ? super[b] : 0.0;
    const double inc = block_inclusive_scan_f64(v, wt);
    const double cr = carry;
    if (b < S) super[b] = cr + (inc - v);
    __syncthreads();
    if (threadIdx.x == kBlock - 1) carry = cr + inc;
    __syncthreads();
  }
}

// cum: weights -> inclusive scan (tile_base[t] + the scan within tile t); the owner of face F - 1 publishes the status
__global__ void __launch_bounds__(kBlock) k_ms_apply(uint32_t F, double *__restrict__ cum, const double *__restrict__ tile_base,
                                                      Status *__restrict__ st, Status *__restrict__ status_out) {
  __shared__ double wt[4];
  const uint32_t f0 = blockIdx.x * kTile + threadIdx.x * kPer;
  double x[kPer], s = 0.0;
  for (int k = 0; k < kPer; ++k) {
    x[k] = f0 + k < F ? cum[f0 + k] : 0.0;
    s += x[k];
  }
  const double inc = block_inclusive_scan_f64(s, wt);
  double run = tile_base[blockIdx.x] + (inc - s);
  for (int k = 0; k < kPer; ++k) {
    if (f0 + k >= F) break;
    run += x[k];
    cum[f0 + k] = run;
    if (f0 + k == F - 1) {
      st->total = run;
      st->zero_area = run > 0.0 ? 0u : 1u;
      if (status_out) {
        status_out->bad_faces = st->bad_faces;  // (final: k_ms_weights ended before this launch began)
        status_out->zero_area = st->zero_area;
        status_out->total = run;
      }
    }
  }
}

__global__ void __launch_bounds__(kBlock) k_ms_sample(const float *__restrict__ verts, uint32_t V, const int32_t *__restrict__ tris,
                                                       uint32_t F, const double *__restrict__ cum, const Status *__restrict__ st,
                                                       const float *__restrict__ uniforms, uint32_t M, const float *__restrict__ attrs,
                                                       uint32_t A, float *__restrict__ points, int32_t *__restrict__ face,
                                                       float *__restrict__ bary, float *__restrict__ attr_out,
                                                       float *__restrict__ normals) {
  const uint32_t m = blockIdx.x * kBlock + threadIdx.x;
  if (m >= M) return;
  const float nanf_ = __uint_as_float(0x7fc00000u);
  if (st->zero_area) {
    if (points) for (int k = 0; k < 3; ++k) points[3 * (size_t)m + k] = nanf_;
    if (face) face[m] = -1;
    if (bary) { bary[2 * (size_t)m] = nanf_; bary[2 * (size_t)m + 1] = nanf_; }
    if (attr_out) for (uint32_t a = 0; a < A; ++a) attr_out[A * (size_t)m + a] = nanf_;
    if (normals) for (int k = 0; k < 3; ++k) normals[3 * (size_t)m + k] = nanf_;
    return;
  }
  const double pick = (double)uniforms[3 * (size_t)m] * st->total;
  uint32_t lo = 0, hi = F - 1;  // (cum[F - 1] = total >= pick)
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (cum[mid] >= pick) hi = mid; else lo = mid + 1;
  }
  float p[3][3];
  double c[3], len = 0.0;
  bool bad;
  uint32_t f = lo;
  double w = face_weight(verts, V, tris, f, p, c, &len, &bad);
  while (!(w > 0.0) && f + 1 < F) w = face_weight(verts, V, tris, ++f, p, c, &len, &bad);
  // (total > 0 and a monotone cum leave a face with weight at or after lo; rounding between the scan's levels can break the
  // monotony by an ulp of fp64, so walk back rather than trust it)
  for (f = w > 0.0 ? f : lo; !(w > 0.0) && f > 0;) w = face_weight(verts, V, tris, --f, p, c, &len, &bad);
  float r1 = uniforms[3 * (size_t)m + 1], r2 = uniforms[3 * (size_t)m + 2];
  if (r1 + r2 > 1.0f) {
    r1 = 1.0f - r1;
    r2 = 1.0f - r2;
  }
  if (points)
    for (int k = 0; k < 3; ++k) points[3 * (size_t)m + k] = p[0][k] + ((p[1][k] - p[0][k]) * r1 + (p[2][k] - p[0][k]) * r2);
  if (face) face[m] = (int32_t)f;
  if (bary) { bary[2 * (size_t)m] = r1; bary[2 * (size_t)m + 1] = r2; }
  if (attr_out) {
    const size_t i0 = (size_t)tris[3 * (size_t)f], i1 = (size_t)tris[3 * (size_t)f + 1], i2 = (size_t)tris[3 * (size_t)f + 2];
    for (uint32_t a = 0; a < A; ++a) {
      const float a0 = attrs[A * i0 + a], a1 = attrs[A * i1 + a], a2 = attrs[A * i2 + a];
      attr_out[A * (size_t)m + a] = a0 + ((a1 - a0) * r1 + (a2 - a0) * r2);
    }
  }
  if (normals)
    for (int k = 0; k < 3; ++k) normals[3 * (size_t)m + k] = (float)(c[k] / len);
}

// --- remove_close ------------------------------------------------------------------------------------------------------
constexpr uint8_t kUndecided = 0, kKept = 1, kRemoved = 2;
constexpr uint32_t kMaxCells = 1u << 26;

struct Grid {
  float lo[3];
  uint32_t dim[3];
  double h;
};

__host__ __device__ inline uint32_t cell_budget(uint32_t N) { return N < 64u ? 64u : (N > kMaxCells ? kMaxCells : N); }

// the bounding box of the finite points (k_knn_bbox's partials) -> the grid: cell side and cells per axis
__global__ void __launch_bounds__(64) k_rc_grid(uint32_t nb, const float *__restrict__ part, float r, float r2, uint32_t cap,
                                                 Grid *__restrict__ G) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float mn[3] = {3.402823466e38f, 3.402823466e38f, 3.402823466e38f}, mx[3] = {-3.402823466e38f, -3.402823466e38f, -3.402823466e38f};
  uint32_t cnt = 0;
  for (uint32_t b = 0; b < nb; ++b) {
    for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], part[8 * b + a]); mx[a] = fmaxf(mx[a], part[8 * b + 3 + a]); }
    cnt += __float_as_uint(part[8 * b + 6]);
  }
  double ext[3], emax = 0.0;
  for (int a = 0; a < 3; ++a) {
    if (cnt == 0) { mn[a] = 0.0f; mx[a] = 0.0f; }
    ext[a] = (double)mx[a] - (double)mn[a];
    emax = ext[a] > emax ? ext[a] : emax;
    G->lo[a] = mn[a];
  }
  double h = 1.0;
  uint32_t dim[3] = {1, 1, 1};
  if (emax > 0.0 && r2 <= 3.402823466e38f) {  // (r * r = +inf accepts every pair: one cell)
    auto cells = [&](double side, uint32_t *d) {
      double t = 1.0;
      for (int a = 0; a < 3; ++a) {
        const double c = floor(ext[a] / side) + 1.0;
        if (d) d[a] = (uint32_t)c;  // (called with d only where the product is within the budget)
        t *= c;
      }
      return t;
    };
    double h_min = (double)r * 1.0001;
    if (h_min < 0x1p-60) h_min = 0x1p-60;
    h = h_min;
    if (cells(h_min, nullptr) > (double)cap) {  // the budget binds: the smallest side that fits it (geometric bisection)
      double s_lo = h_min, s_hi = 2.0 * emax;   // (a side above every extent: one cell)
      if (s_hi < 2.0 * h_min) s_hi = 2.0 * h_min;
      for (int it = 0; it < 64; ++it) {
        const double mid = sqrt(s_lo * s_hi);
        if (cells(mid, nullptr) <= (double)cap) s_hi = mid; else s_lo = mid;
      }
      h = s_hi;
    }
    cells(h, dim);
  }
  for (int a = 0; a < 3; ++a) G->dim[a] = dim[a];
  G->h = h;
}

// monotone in v, and at most dim - 1: dim = floor(ext / h) + 1 with ext the same expression at v = the box's maximum
__device__ __forceinline__ uint32_t cell_coord(float v, float lo, double h, uint32_t dim) {
  const double t = ((double)v - (double)lo) / h;
  return t >= (double)(dim - 1) ? dim - 1 : (uint32_t)t;
}

// cell_of[i] = the cell of point i, `cap` for a non-finite point (the bucket after the last possible cell); counts[cell]++
__global__ void __launch_bounds__(kBlock) k_rc_count(uint32_t N, uint32_t cap, const float *__restrict__ pts, const Grid *__restrict__ G,
                                                      uint32_t *__restrict__ cell_of, uint32_t *__restrict__ counts) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
  uint32_t c = cap;
  if (finite3(x, y, z)) {
    const double h = G->h;
    const uint32_t cx = cell_coord(x, G->lo[0], h, G->dim[0]), cy = cell_coord(y, G->lo[1], h, G->dim[1]),
                   cz = cell_coord(z, G->lo[2], h, G->dim[2]);
    c = (cz * G->dim[1] + cy) * G->dim[0] + cx;
  }
  cell_of[i] = c;
  atomicAdd(&counts[c], 1u);
}

// state by sorted position: the finite points (before start[cap]) UNDECIDED, the others REMOVED; keep[] = 0; cnt[2] = the
// undecided count "of the round before the first"
__global__ void __launch_bounds__(kBlock) k_rc_reset(uint32_t N, const uint32_t *__restrict__ first_nonfinite, uint8_t *__restrict__ state,
                                                      uint8_t *__restrict__ keep, uint32_t *__restrict__ cnt) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t nf = *first_nonfinite;
  if (p == 0) cnt[2] = nf;
  if (p >= N) return;
  state[p] = p < nf ? kUndecided : kRemoved;
  keep[p] = 0;
}

__global__ void __launch_bounds__(kBlock) k_rc_round(uint32_t N, const float4 *__restrict__ sorted, const uint32_t *__restrict__ start,
                                                      const Grid *__restrict__ G, float r2, uint8_t *state, uint8_t *__restrict__ keep,
                                                      const uint32_t *__restrict__ prev, uint32_t *__restrict__ cur) {
  if (*prev == 0u) return;  // (the whole grid: nothing was undecided after the round before)
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  bool undecided = false;
  if (p < N && state[p] == kUndecided) {
    const float4 q = sorted[p];
    const uint32_t i = __float_as_uint(q.w);
    const double h = G->h;
    const uint32_t dx = G->dim[0], dy = G->dim[1], dz = G->dim[2];
    const uint32_t cx = cell_coord(q.x, G->lo[0], h, dx), cy = cell_coord(q.y, G->lo[1], h, dy), cz = cell_coord(q.z, G->lo[2], h, dz);
    const uint32_t x0 = cx > 0 ? cx - 1 : 0, x1 = cx + 1 < dx ? cx + 1 : cx;
    const uint32_t y0 = cy > 0 ? cy - 1 : 0, y1 = cy + 1 < dy ? cy + 1 : cy;
    const uint32_t z0 = cz > 0 ? cz - 1 : 0, z1 = cz + 1 < dz ? cz + 1 : cz;
    uint8_t res = kKept;
    for (uint32_t z = z0; z <= z1 && res != kRemoved; ++z)
      for (uint32_t y = y0; y <= y1 && res != kRemoved; ++y) {
        const uint32_t row = (z * dy + y) * dx;  // (cells x0 .. x1 of a row are consecutive in the sorted order)
        const uint32_t e = start[row + x1 + 1];
        for (uint32_t j = start[row + x0]; j < e; ++j) {
          const float4 o = sorted[j];
          if (__float_as_uint(o.w) >= i) continue;
          const float ax = q.x - o.x, ay = q.y - o.y, az = q.z - o.z;
          const float d2 = (ax * ax + ay * ay) + az * az;
          if (!(d2 <= r2)) continue;
          const uint8_t s = state[j];
          if (s == kKept) { res = kRemoved; break; }
          if (s == kUndecided) res = kUndecided;
        }
      }
    if (res == kUndecided) {
      undecided = true;
    } else {
      state[p] = res;
      if (res == kKept) keep[i] = 1;
    }
  }
  const uint32_t n = (uint32_t)__popcll(__ballot(undecided));
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(cur, n);
}

// the last round's count -> where the next call and the caller read it
__global__ void __launch_bounds__(64) k_rc_publish(const uint32_t *__restrict__ from, uint32_t *__restrict__ last,
                                                    uint32_t *__restrict__ remaining) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const uint32_t v = *from;
  *last = v;
  if (remaining) *remaining = v;
}

// --- host side ---------------------------------------------------------------------------------------------------------
struct MsWs {
  Status *st;
  double *cum;       // [F]
  double *tile_sum;  // [T]
  double *super;     // [S]
  uint32_t T, S;
  size_t bytes;
};

inline MsWs carve_ms(void *base, uint32_t F) {
  char *p0 = (char *)base, *p = p0 + ((256 - ((uintptr_t)p0 & 255)) & 255);
  MsWs w;
  w.T = (F + kTile - 1) / kTile;
  w.S = (w.T + kTile - 1) / kTile;
  size_t off = 0;
  auto take = [&](size_t b) { char *r = p + off; off += align256(b); return r; };
  w.st = (Status *)take(sizeof(Status));
  w.cum = (double *)take(sizeof(double) * (size_t)F);
  w.tile_sum = (double *)take(sizeof(double) * (size_t)w.T);
  w.super = (double *)take(sizeof(double) * (size_t)w.S);
  w.bytes = off + 256;  // (room for the leading alignment of any base address)
  return w;
}

struct RcWs {
  Grid *G;
  float *part;
  uint32_t *cell_of, *counts, *start, *cursor, *tile_sum, *cnt;
  float4 *sorted;
  uint8_t *state;
  uint32_t cap, M, T;
  size_t bytes;
};

inline RcWs carve_rc(void *base, uint32_t N) {
  char *p0 = (char *)base, *p = p0 + ((256 - ((uintptr_t)p0 & 255)) & 255);
  RcWs w;
  w.cap = cell_budget(N);
  w.M = w.cap + 2;  // the cells, the non-finite bucket, and the end of it (start[cap + 1] = N)
  w.T = (w.M + gs_ms_index::kScanTile - 1) / gs_ms_index::kScanTile;
  size_t off = 0;
  auto take = [&](size_t b) { char *r = p + off; off += align256(b); return r; };
  w.G = (Grid *)take(sizeof(Grid));
  w.part = (float *)take(sizeof(float) * 8 * gs_ms_index::kMaxBlocks);
  w.cnt = (uint32_t *)take(sizeof(uint32_t) * 4);
  w.cell_of = (uint32_t *)take(sizeof(uint32_t) * (size_t)N);
  w.counts = (uint32_t *)take(sizeof(uint32_t) * (size_t)w.M);
  w.start = (uint32_t *)take(sizeof(uint32_t) * (size_t)w.M);
  w.cursor = (uint32_t *)take(sizeof(uint32_t) * (size_t)w.M);
  w.tile_sum = (uint32_t *)take(sizeof(uint32_t) * (size_t)w.T);
  w.sorted = (float4 *)take(sizeof(float4) * (size_t)N);
  w.state = (uint8_t *)take((size_t)N);
  w.bytes = off + 256;
  return w;
}

inline bool bad_radius(float r) { return !(r >= 0.0f); }  // (negative or NaN)

}  // namespace gs_ms

using namespace gs_ms;

extern "C" {

size_t gsgen_mesh_sample_workspace_bytes(uint32_t n_faces) {
  if (n_faces == 0 || n_faces > 0x7fffffffu) return 0;
  return carve_ms(nullptr, n_faces).bytes;
}

int gsgen_mesh_sample(const float *verts, uint32_t n_verts, const int32_t *tris, uint32_t n_faces, const float *uniforms,
                      uint32_t n_samples, const float *attributes, uint32_t n_attr, float *points, int32_t *face_index,
                      float *barycentric, float *attr_out, float *normals, void *status, void *workspace, size_t workspace_bytes,
                      gsgen_stream_t stream) {
  if (n_attr > kMaxAttr || n_faces > 0x7fffffffu || n_verts > 0x7fffffffu) return GSGEN_EINVAL;
  if ((n_attr != 0) != (attributes != nullptr) || (attr_out && !n_attr)) return GSGEN_EINVAL;
  if (status && ((uintptr_t)status & 7)) return GSGEN_EINVAL;
  if (n_faces == 0 || (n_samples == 0 && !status)) return 0;
  if (!tris || !workspace || (n_verts && !verts) || (n_samples && !uniforms)) return GSGEN_EINVAL;
  const MsWs w = carve_ms(workspace, n_faces);
  if (w.bytes > workspace_bytes) return GSGEN_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  if (int e = (int)hipMemsetAsync(w.st, 0, sizeof(Status), s)) return e;
  hipLaunchKernelGGL(k_ms_weights, dim3(w.T), dim3(kBlock), 0, s, verts, n_verts, tris, n_faces, w.cum, w.tile_sum, w.st);
  hipLaunchKernelGGL(k_ms_scan<false>, dim3(w.S), dim3(kBlock), 0, s, w.T, w.tile_sum, w.super);
  hipLaunchKernelGGL(k_ms_scan_super, dim3(1), dim3(kBlock), 0, s, w.S, w.super);
  hipLaunchKernelGGL(k_ms_scan<true>, dim3(w.S), dim3(kBlock), 0, s, w.T, w.tile_sum, w.super);
  hipLaunchKernelGGL(k_ms_apply, dim3(w.T), dim3(kBlock), 0, s, n_faces, w.cum, (const double *)w.tile_sum, w.st, (Status *)status);
  if (n_samples)
    hipLaunchKernelGGL(k_ms_sample, dim3((n_samples + kBlock - 1) / kBlock), dim3(kBlock), 0, s, verts, n_verts, tris, n_faces,
                       (const double *)w.cum, (const Status *)w.st, uniforms, n_samples, attributes, n_attr, points, face_index,
                       barycentric, attr_out, normals);
  return (int)hipGetLastError();
}

size_t gsgen_remove_close_workspace_bytes(uint32_t n_points) {
  if (n_points == 0 || n_points > 0x7fffffffu) return 0;
  return carve_rc(nullptr, n_points).bytes;
}

int gsgen_remove_close_init(const float *points, uint32_t n_points, float radius, uint8_t *keep, void *workspace,
                            size_t workspace_bytes, gsgen_stream_t stream) {
  if (bad_radius(radius) || n_points > 0x7fffffffu) return GSGEN_EINVAL;
  if (n_points == 0) return 0;
  if (!points || !keep || !workspace) return GSGEN_EINVAL;
  const RcWs w = carve_rc(workspace, n_points);
  if (w.bytes > workspace_bytes) return GSGEN_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const uint32_t N = n_points, nb = gs_ms_index::reduce_blocks(N), ng = (N + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(gs_ms_index::k_knn_bbox, dim3(nb), dim3(kBlock), 0, s, N, points, w.part);
  hipLaunchKernelGGL(k_rc_grid, dim3(1), dim3(64), 0, s, nb, (const float *)w.part, radius, radius * radius, w.cap, w.G);
  if (int e = (int)hipMemsetAsync(w.counts, 0, sizeof(uint32_t) * (size_t)w.M, s)) return e;
  hipLaunchKernelGGL(k_rc_count, dim3(ng), dim3(kBlock), 0, s, N, w.cap, points, (const Grid *)w.G, w.cell_of, w.counts);
  hipLaunchKernelGGL(gs_ms_index::k_knn_scan_tiles, dim3(w.T), dim3(kBlock), 0, s, w.M, (const uint32_t *)w.counts, w.tile_sum);
  hipLaunchKernelGGL(gs_ms_index::k_knn_scan_sums, dim3(1), dim3(kBlock), 0, s, w.T, w.tile_sum);
  hipLaunchKernelGGL(gs_ms_index::k_knn_scan_apply, dim3(w.T), dim3(kBlock), 0, s, w.M, (const uint32_t *)w.counts,
                     (const uint32_t *)w.tile_sum, w.start, w.cursor);
  hipLaunchKernelGGL(gs_ms_index::k_knn_scatter, dim3(ng), dim3(kBlock), 0, s, N, points, (const uint32_t *)w.cell_of, w.cursor,
                     w.sorted);
  hipLaunchKernelGGL(k_rc_reset, dim3(ng), dim3(kBlock), 0, s, N, (const uint32_t *)(w.start + w.cap), w.state, keep, w.cnt);
  return (int)hipGetLastError();
}

int gsgen_remove_close_rounds(uint32_t n_rounds, uint32_t n_points, float radius, uint8_t *keep, uint32_t *remaining, void *workspace,
                              size_t workspace_bytes, gsgen_stream_t stream) {
  if (bad_radius(radius) || n_points > 0x7fffffffu) return GSGEN_EINVAL;
  if (n_points == 0) return 0;
  if (!keep || !workspace) return GSGEN_EINVAL;
  const RcWs w = carve_rc(workspace, n_points);
  if (w.bytes > workspace_bytes) return GSGEN_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const uint32_t ng = (n_points + kBlock - 1) / kBlock;
  const float r2 = radius * radius;
  const uint32_t *prev = w.cnt + 2;  // (what the last call, or the init, left)
  for (uint32_t k = 0; k < n_rounds; ++k) {
    uint32_t *cur = w.cnt + (k & 1u);
    if (int e = (int)hipMemsetAsync(cur, 0, sizeof(uint32_t), s)) return e;
    hipLaunchKernelGGL(k_rc_round, dim3(ng), dim3(kBlock), 0, s, n_points, (const float4 *)w.sorted, (const uint32_t *)w.start,
                       (const Grid *)w.G, r2, w.state, keep, prev, cur);
    prev = cur;
  }
  hipLaunchKernelGGL(k_rc_publish, dim3(1), dim3(64), 0, s, prev, w.cnt + 2, remaining);
  return (int)hipGetLastError();
}

}  // extern "C"
