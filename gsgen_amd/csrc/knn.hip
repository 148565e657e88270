// knn.hip -- exact self k-nearest-neighbour search over the Gaussian centres, for gfx950 (compiled with -ffp-contract=off).
//
// Replaces pytorch3d's knn_points (utils/ops.py:104-134) and faiss IndexFlatL2 (utils/initialize.py:16-35), neither of which
// exists for ROCm.  Every point is also a query; each row lists the K nearest points in ascending (dist2, index) order, with
// dist2 = dx*dx + dy*dy + dz*dz, d = p_j - p_i, evaluated left to right without contraction, so that an fp32 brute force
// reproduces every bit.  A non-finite point is nobody's neighbour; its own row and every row short of K finite candidates are
// padded with (idx -1, dist2 +inf).
//
// Pipeline (every launch shape depends on N and K only; bounds, cell size and counts live in the workspace, so the call can be
// captured in a hipGraph and replayed on new values of the same buffer):
//   1. k_knn_bbox / k_knn_bbox_final: min / max of the finite points per axis (per-block partials, then one block).
//   2. k_knn_hist x 2 + k_knn_select x 2: the grid box per axis -- the 1 % / 99 % quantiles, located with a 1024-bin histogram
//      over the bounding box and refined with a second one over the selected bins, then widened by a quarter of their distance
//      per side (within the bounding box).  Points outside that box are OUTLIERS: they go to a list of their own instead of
//      stretching the grid (a 1 %-outlier cloud at 100x the radius would otherwise put its whole core in a handful of cells).
//      The second select also sizes the grid: the coarsest cubic cell with at most `cap` cells in total, cap = N / points per
//      cell (from N and K).
//   3. counting sort of the points by bucket: k_knn_count (histogram), a three-kernel exclusive scan, k_knn_scatter.  Buckets:
//      the cells, then the outliers, then the non-finite points.  The order inside a bucket is whatever the atomics give: the
//      result does not depend on it (every key (dist2, index) is distinct).
//   4. k_knn_query: one thread per point, in bucket order (the lanes of a wave share cells), with a sorted top-K of 64-bit keys
//      (float bits of dist2 << 32 | index: dist2 >= 0, so the integer order is the (dist2, index) order, ties included) held in
//      registers -- a compare-and-shift network unrolled over the compile-time list length, no dynamic indexing, no LDS.  The
//      grid search visits the query's cell, then Chebyshev rings of cells outward; a ring stops the search once its lower bound
//      exceeds the current K-th distance, a cell is skipped when its box is farther than that.  A query in the box reads the
//      outlier list only when the box's nearest face is within its K-th distance; an outlier query reads the outlier list first
//      and the grid only while the box is within its K-th distance.  Every bound is shrunk by a margin that covers the rounding
//      of the cell assignment, so pruning never drops a candidate that could enter the list.
//
// Steps 1-3 are the INDEX over `points` (build_index, in knn_index.hpp beside this file: fps.hip builds the same index); step 4 is one of five consumers of it:
//   k_knn_query       every point is a query (gsgen_knn, above).
//   k_knn_query_ext   queries from an array of their own, in the caller's order (gsgen_knn_query): d = p_j - q.  The query's cell
//                     comes from the index's Params; a query outside the grid box takes the outlier-query path, a non-finite
//                     query keeps its padded row.
//   k_density_grid    the lattice of utils/export.py:66-120 (get_density_val_grid_from_ckpt): a wavefront takes a 4 x 4 x 4 brick of
//                     lattice points, runs the same search and sums opacity_j exp(-1/2 d^T Sigma_j^-1 d) over the neighbours it
//                     keeps, straight from the top-K in registers: one store per lattice point, no idx / dist2 in memory.
//                     Sigma^-1 = R diag(1 / s^2) R^T in closed form, once per Gaussian (k_density_prep).
//   k_density_points  the same search and sum at points of the caller's own, one lane per point as k_knn_query_ext, with the sum's
//                     gradient and a density-weighted colour beside its value (gsgen_density_points: mesh vertex normals and colours).
//   k_point_normals   the self search of k_knn_query, then the covariance of the neighbourhood and its eigen-frame from the list in
//                     registers (gsgen_point_normals: pytorch3d's estimate_pointcloud_normals); K up to 64, a list width of its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gsgen_hip.h"
#include "knn_index.hpp"

namespace gs_knn {

// --- 4. the query ----------------------------------------------------------------------------------------------------
template <int L>
__device__ __forceinline__ void topk_insert(unsigned long long (&list)[L], unsigned long long key) {
  // list ascending; key < list[L-1] (checked by the caller).  new[j] = min(list[j], max(key, list[j-1])), unrolled
#pragma unroll
  for (int j = L - 1; j > 0; --j) {
    const unsigned long long prev = list[j - 1];
    const unsigned long long m = key > prev ? key : prev;
    list[j] = m < list[j] ? m : list[j];
  }
  list[0] = key < list[0] ? key : list[0];
}

// distance from q to the slab [blo, bhi] of one axis, shrunk by the rounding margin
__device__ __forceinline__ float axis_gap(float q, float blo, float bhi, float margin) {
  float g = 0.0f;
  if (q < blo) g = blo - q;
  if (q > bhi) g = q - bhi;
  g -= margin;
  return g > 0.0f ? g : 0.0f;
}

template <int L>
__device__ __forceinline__ void scan_range(unsigned long long (&list)[L], const float4 *__restrict__ sorted, uint32_t b, uint32_t e,
                                           const float4 q) {
  for (uint32_t j = b; j < e; ++j) {
    const float4 p = sorted[j];
    const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    const float d2 = dx * dx + dy * dy + dz * dz;
    const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | __float_as_uint(p.w);
    if (key < list[L - 1]) topk_insert<L>(list, key);
  }
}

__device__ __forceinline__ float kth_of(unsigned long long key) { return __uint_as_float((uint32_t)(key >> 32)); }

// The grid points (all inside the grid box) in rings of cells around the query's (clamped) cell.  floor: a lower bound of the
// distance from the query to any point of the grid box (0 inside it).
template <int L>
__device__ __forceinline__ void scan_grid(unsigned long long (&list)[L], const Params *__restrict__ P, const uint32_t *__restrict__ start,
                                          const float4 *__restrict__ sorted, const float4 q, float floor) {
  const float qv[3] = {q.x, q.y, q.z};
  const float h = P->h, ih = P->inv_h;
  int dim[3], c[3];
  float lo[3], margin[3];
  for (int a = 0; a < 3; ++a) {
    dim[a] = (int)P->dim[a];
    lo[a] = P->lo[a];
    c[a] = (int)cell_coord(qv[a], lo[a], ih, (uint32_t)dim[a]);
    // covers the rounding of (v - lo) * inv_h and of lo + c * h (relative 2^-22 of the magnitudes involved)
    margin[a] = 1e-3f * h + 1e-6f * (fabsf(lo[a]) + fabsf(qv[a]) + P->ext[a]);
  }
  int rmax = 0;
  for (int a = 0; a < 3; ++a) {
    rmax = c[a] > rmax ? c[a] : rmax;
    rmax = dim[a] - 1 - c[a] > rmax ? dim[a] - 1 - c[a] : rmax;
  }
  for (int r = 0; r <= rmax; ++r) {
    // lower bound of every point in ring r and beyond: the nearest face of the (2r-1)-cube around the query's cell on a side
    // where cells of ring r exist, and never below the distance to the grid box
    float lb = r == 0 ? floor : 3.402823466e38f;
    if (r > 0) {
      for (int a = 0; a < 3; ++a) {
        if (c[a] + r <= dim[a] - 1) lb = fminf(lb, fmaxf(lo[a] + (float)(c[a] + r) * h - qv[a] - margin[a], 0.0f));
        if (c[a] - r >= 0) lb = fminf(lb, fmaxf(qv[a] - (lo[a] + (float)(c[a] - r + 1) * h) - margin[a], 0.0f));
      }
      lb = fmaxf(lb, floor);
    }
    if (lb * lb > kth_of(list[L - 1])) break;
    const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, dim[2] - 1);
    const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, dim[1] - 1);
    for (int cz = z0; cz <= z1; ++cz) {
      const float gz = axis_gap(qv[2], lo[2] + (float)cz * h, lo[2] + (float)(cz + 1) * h, margin[2]);
      for (int cy = y0; cy <= y1; ++cy) {
        const float gy = axis_gap(qv[1], lo[1] + (float)cy * h, lo[1] + (float)(cy + 1) * h, margin[1]);
        const bool shell = (cz - c[2] == r || c[2] - cz == r || cy - c[1] == r || c[1] - cy == r);
        const int step = (shell || r == 0) ? 1 : 2 * r;
        for (int cx = c[0] - r; cx <= c[0] + r; cx += step) {
          if (cx < 0 || cx >= dim[0]) continue;
          const float gx = axis_gap(qv[0], lo[0] + (float)cx * h, lo[0] + (float)(cx + 1) * h, margin[0]);
          if (gx * gx + gy * gy + gz * gz > kth_of(list[L - 1])) continue;
          const uint32_t cell = ((uint32_t)cz * (uint32_t)dim[1] + (uint32_t)cy) * (uint32_t)dim[0] + (uint32_t)cx;
          scan_range<L>(list, sorted, start[cell], start[cell + 1], q);
        }
      }
    }
  }
}

// Sorted layout: [cells 0 .. cap-1 | outliers (finite, outside the grid box) | non-finite].  A query in the grid box searches the
// grid, then the outliers if the box's exterior is nearer than its K-th distance; an outlier query searches the outliers first,
// then the grid with the distance to the box as a floor (a far outlier is done after the first bound).
// The self search of the point at position t of the sorted copy (its list: `list`, padded by the caller).  A non-finite point
// (t >= start[cap + 1]) searches nothing.
template <int L>
__device__ __forceinline__ void search_self(unsigned long long (&list)[L], uint32_t t, uint32_t cap, const Params *__restrict__ P,
                                            const uint32_t *__restrict__ start, const float4 *__restrict__ sorted, const float4 q) {
  const uint32_t o_begin = start[cap], o_end = start[cap + 1];
  if (t < o_begin) {
    scan_grid<L>(list, P, start, sorted, q, 0.0f);
    if (o_end > o_begin) {
      // every outlier lies beyond a face of the box: at least the distance to the nearest face
      const float qv[3] = {q.x, q.y, q.z};
      float ext = 3.402823466e38f;
      for (int a = 0; a < 3; ++a) {
        const float m = 1e-6f * (fabsf(P->lo[a]) + fabsf(P->hi[a]) + fabsf(qv[a]));
        ext = fminf(ext, fmaxf(fminf(qv[a] - P->lo[a], P->hi[a] - qv[a]) - m, 0.0f));
      }
      if (ext * ext <= kth_of(list[L - 1])) scan_range<L>(list, sorted, o_begin, o_end, q);
    }
  } else if (t < o_end) {
    scan_range<L>(list, sorted, o_begin, o_end, q);
    const float qv[3] = {q.x, q.y, q.z};
    float g2 = 0.0f;
    for (int a = 0; a < 3; ++a) {
      const float m = 1e-6f * (fabsf(P->lo[a]) + fabsf(P->hi[a]) + fabsf(qv[a]));
      const float g = axis_gap(qv[a], P->lo[a], P->hi[a], m);
      g2 += g * g;
    }
    scan_grid<L>(list, P, start, sorted, q, sqrtf(g2));
  }
}

template <int L>
__global__ void __launch_bounds__(kBlock) k_knn_query(uint32_t N, uint32_t K, uint32_t cap, const Params *__restrict__ P,
                                                       const uint32_t *__restrict__ start, const float4 *__restrict__ sorted,
                                                       float *__restrict__ dist2, int32_t *__restrict__ idx) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= N) return;
  const float4 q = sorted[t];
  const uint32_t qi = __float_as_uint(q.w);
  unsigned long long list[L];
#pragma unroll
  for (int k = 0; k < L; ++k) list[k] = kPad;
  search_self<L>(list, t, cap, P, start, sorted, q);
  float *drow = dist2 + (size_t)qi * K;
  int32_t *irow = idx + (size_t)qi * K;
#pragma unroll
  for (int k = 0; k < L; ++k) {
    if ((uint32_t)k < K) {
      const uint32_t j = (uint32_t)(list[k] & 0xffffffffull);
      drow[k] = __uint_as_float((uint32_t)(list[k] >> 32));
      irow[k] = j == 0xffffffffu ? -1 : (int32_t)j;
    }
  }
}

// --- 4b. queries that are not points of the index ------------------------------------------------------------------------
// The search of k_knn_query for any position q: in the grid box (the test k_knn_count applies to a point) the grid, then the
// outliers if the box's exterior is nearer than the K-th distance; outside it the outliers first, then the grid with the distance
// to the box as a floor.  A non-finite q searches nothing: its list stays padded.
template <int L>
__device__ __forceinline__ void search_ext(unsigned long long (&list)[L], uint32_t cap, const Params *__restrict__ P,
                                           const uint32_t *__restrict__ start, const float4 *__restrict__ sorted, const float4 q) {
  if (!finite3(q.x, q.y, q.z)) return;
  const uint32_t o_begin = start[cap], o_end = start[cap + 1];
  const float qv[3] = {q.x, q.y, q.z};
  const bool inbox = q.x >= P->lo[0] && q.x <= P->hi[0] && q.y >= P->lo[1] && q.y <= P->hi[1] && q.z >= P->lo[2] && q.z <= P->hi[2];
  if (inbox) {
    scan_grid<L>(list, P, start, sorted, q, 0.0f);
    if (o_end > o_begin) {
      float ext = 3.402823466e38f;
      for (int a = 0; a < 3; ++a) {
        const float m = 1e-6f * (fabsf(P->lo[a]) + fabsf(P->hi[a]) + fabsf(qv[a]));
        ext = fminf(ext, fmaxf(fminf(qv[a] - P->lo[a], P->hi[a] - qv[a]) - m, 0.0f));
      }
      if (ext * ext <= kth_of(list[L - 1])) scan_range<L>(list, sorted, o_begin, o_end, q);
    }
  } else {
    scan_range<L>(list, sorted, o_begin, o_end, q);
    float g2 = 0.0f;
    for (int a = 0; a < 3; ++a) {
      const float m = 1e-6f * (fabsf(P->lo[a]) + fabsf(P->hi[a]) + fabsf(qv[a]));
      const float g = axis_gap(qv[a], P->lo[a], P->hi[a], m);
      g2 += g * g;
    }
    scan_grid<L>(list, P, start, sorted, q, sqrtf(g2));
  }
}

template <int L>
__global__ void __launch_bounds__(kBlock) k_knn_query_ext(uint32_t Q, uint32_t K, uint32_t cap, const Params *__restrict__ P,
                                                           const uint32_t *__restrict__ start, const float4 *__restrict__ sorted,
                                                           const float *__restrict__ queries, float *__restrict__ dist2,
                                                           int32_t *__restrict__ idx) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= Q) return;
  const float4 q = make_float4(queries[3 * (size_t)t], queries[3 * (size_t)t + 1], queries[3 * (size_t)t + 2], 0.0f);
  unsigned long long list[L];
#pragma unroll
  for (int k = 0; k < L; ++k) list[k] = kPad;
  search_ext<L>(list, cap, P, start, sorted, q);
  float *drow = dist2 + (size_t)t * K;
  int32_t *irow = idx + (size_t)t * K;
#pragma unroll
  for (int k = 0; k < L; ++k) {
    if ((uint32_t)k < K) {
      const uint32_t j = (uint32_t)(list[k] & 0xffffffffull);
      drow[k] = __uint_as_float((uint32_t)(list[k] >> 32));
      irow[k] = j == 0xffffffffu ? -1 : (int32_t)j;
    }
  }
}

// --- 4c. the density lattice ---------------------------------------------------------------------------------------------
// rec[2 i] = (a00, a01, a02, a11), rec[2 i + 1] = (a12, a22, opacity, 0): A = Sigma^-1 = R diag(1 / s^2) R^T, R the rotation of
// geometry.hip's quat_to_rot (kornia 0.6.0, w first, normalised with eps 1e-12), Sigma = R diag(s^2) R^T as qsvec2covmat_batched
// builds it.  A_ij = (R_i0 R_j0) w_0 + (R_i1 R_j1) w_1 + (R_i2 R_j2) w_2, w_k = 1 / (s_k s_k), left to right.
// rec_g (null for the lattice, which reads rec alone): the same six entries for the GRADIENT of the point kernel, the formula
// evaluated in fp64 from the fp32 inputs and rounded to fp32 once: rec_g[2 i] = (a00, a01, a02, a11), rec_g[2 i + 1] = (a12, a22, 0, 0).
// An fp32 off-diagonal entry that is the remainder of three cancelling terms carries hundreds of eps of its own size (the errors of
// R are absolute); m = d^T A d does not feel that, its diagonal dominates, but a row of A d does.  rec itself does not change by a bit.
__global__ void __launch_bounds__(kBlock) k_density_prep(uint32_t N, const float *__restrict__ qvec, const float *__restrict__ scale,
                                                          const float *__restrict__ opacity, float4 *__restrict__ rec,
                                                          float4 *__restrict__ rec_g) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= N) return;
  const float *q = qvec + 4 * (size_t)i, *sc = scale + 3 * (size_t)i;
  float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  n = fmaxf(n, 1e-12f);
  const float w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
  const float twx = tx * w, twy = ty * w, twz = tz * w;
  const float txx = tx * x, txy = ty * x, txz = tz * x;
  const float tyy = ty * y, tyz = tz * y, tzz = tz * z;
  const float R[3][3] = {{1.0f - (tyy + tzz), txy - twz, txz + twy},
                         {txy + twz, 1.0f - (txx + tzz), tyz - twx},
                         {txz - twy, tyz + twx, 1.0f - (txx + tyy)}};
  const float w0 = 1.0f / (sc[0] * sc[0]), w1 = 1.0f / (sc[1] * sc[1]), w2 = 1.0f / (sc[2] * sc[2]);
  float A[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = a; b < 3; ++b) A[a][b] = R[a][0] * R[b][0] * w0 + R[a][1] * R[b][1] * w1 + R[a][2] * R[b][2] * w2;
  rec[2 * (size_t)i] = make_float4(A[0][0], A[0][1], A[0][2], A[1][1]);
  rec[2 * (size_t)i + 1] = make_float4(A[1][2], A[2][2], opacity[i], 0.0f);
  if (rec_g != nullptr) {
    const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    double nd = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    nd = nd > 1e-12 ? nd : 1e-12;
    const double dw = q0 / nd, dx = q1 / nd, dy = q2 / nd, dz = q3 / nd;
    const double Rd[3][3] = {{1.0 - 2.0 * (dy * dy + dz * dz), 2.0 * (dx * dy - dw * dz), 2.0 * (dx * dz + dw * dy)},
                             {2.0 * (dx * dy + dw * dz), 1.0 - 2.0 * (dx * dx + dz * dz), 2.0 * (dy * dz - dw * dx)},
                             {2.0 * (dx * dz - dw * dy), 2.0 * (dy * dz + dw * dx), 1.0 - 2.0 * (dx * dx + dy * dy)}};
    const double s0 = sc[0], s1 = sc[1], s2 = sc[2];
    const double v0 = 1.0 / (s0 * s0), v1 = 1.0 / (s1 * s1), v2 = 1.0 / (s2 * s2);
    float G[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = a; b < 3; ++b) G[a][b] = (float)(Rd[a][0] * Rd[b][0] * v0 + Rd[a][1] * Rd[b][1] * v1 + Rd[a][2] * Rd[b][2] * v2);
    rec_g[2 * (size_t)i] = make_float4(G[0][0], G[0][1], G[0][2], G[1][1]);
    rec_g[2 * (size_t)i + 1] = make_float4(G[1][2], G[2][2], 0.0f, 0.0f);
  }
}

// One term of the field, shared by the lattice and the point kernels: t = opacity_j exp(-1/2 m),
// m = a00 dx dx + a11 dy dy + a22 dz dz + 2 (a01 dx dy + a02 dx dz + a12 dy dz), d = q - mean_j, every product left to right.
__device__ __forceinline__ float density_term(const float4 q, const float *__restrict__ mean, const float4 r0, const float4 r1,
                                              uint32_t j, float &dx, float &dy, float &dz) {
  dx = q.x - mean[3 * (size_t)j], dy = q.y - mean[3 * (size_t)j + 1], dz = q.z - mean[3 * (size_t)j + 2];
  const float diag = r0.x * dx * dx + r0.w * dy * dy + r1.y * dz * dz;
  const float off = r0.y * dx * dy + r0.z * dx * dz + r1.x * dy * dz;
  const float m = diag + 2.0f * off;
  return r1.z * expf(-0.5f * m);
}

// A 256-thread workgroup = four wavefronts = four 4 x 4 x 4 bricks (z fastest, as the output is laid out); lanes past nx, ny or nz
// idle.  Kept neighbours: entries skip .. skip + K - 1 of the sorted list; a padded entry (index -1) contributes nothing.
template <int L>
__global__ void __launch_bounds__(kBlock) k_density_grid(uint32_t nx, uint32_t ny, uint32_t nz, uint32_t K, uint32_t skip, uint32_t cap,
                                                          const Params *__restrict__ P, const uint32_t *__restrict__ start,
                                                          const float4 *__restrict__ sorted, const float *__restrict__ mean,
                                                          const float4 *__restrict__ rec, const float *__restrict__ axis_x,
                                                          const float *__restrict__ axis_y, const float *__restrict__ axis_z,
                                                          float *__restrict__ out) {
  const uint32_t by = (ny + 3) / 4, bz = (nz + 3) / 4;
  const uint32_t brick = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t ix = (brick / (by * bz)) * 4 + (lane >> 4), iy = ((brick / bz) % by) * 4 + ((lane >> 2) & 3),
                 iz = (brick % bz) * 4 + (lane & 3);
  if (ix >= nx || iy >= ny || iz >= nz) return;
  const float4 q = make_float4(axis_x[ix], axis_y[iy], axis_z[iz], 0.0f);
  unsigned long long list[L];
#pragma unroll
  for (int k = 0; k < L; ++k) list[k] = kPad;
  search_ext<L>(list, cap, P, start, sorted, q);
  float sum = 0.0f;
#pragma unroll
  for (int k = 0; k < L; ++k) {
    const uint32_t j = (uint32_t)(list[k] & 0xffffffffull);
    if ((uint32_t)k >= skip && (uint32_t)k < K + skip && j != 0xffffffffu) {
      const float4 r0 = rec[2 * (size_t)j], r1 = rec[2 * (size_t)j + 1];
      float dx, dy, dz;
      sum += density_term(q, mean, r0, r1, j, dx, dy, dz);
    }
  }
  out[((size_t)ix * ny + iy) * nz + iz] = sum;
}

// --- 4d. the field at points of the caller's own ---------------------------------------------------------------------------
// The lattice kernel's search and sum at any position, in the launch shape of k_knn_query_ext: one lane per query, in the caller's
// order, the list in registers.  Per query, over the Ks = K + skip entries of the list (a padded entry contributes nothing):
//   t_k = density_term (above), g = A d row by row, left to right: gx = (a00 dx + a01 dy) + a02 dz, gy = (a01 dx + a11 dy) + a12 dz,
//   gz = (a02 dx + a12 dy) + a22 dz, with A from rec_g (k_density_prep: the entries rounded once from fp64; t_k takes rec's).
//   density = sum of t_k, grad_a = sum of -(t_k g_ka), both over the entries skip .. skip + K - 1 in list order from 0.0f (the
//   gradient of the sum with the neighbour set held fixed; x - y and x + (-y) are the same bits);
//   rgb_c = num_c / den with num_c = sum of t_k color_j[c], den = sum of t_k over ALL entries 0 .. Ks - 1 in list order (the nearest
//   centre counts even where the field drops it); den < 2^-126: the colour of list entry 0, copied.
// A non-finite query, and for rgb a list without a single centre, write 0.  density / grad / rgb / color may be null: a test that is
// uniform over the launch; an output that is not wanted costs nothing and does not change the bits of the others.
template <int L>
__global__ void __launch_bounds__(kBlock) k_density_points(uint32_t Q, uint32_t K, uint32_t skip, uint32_t cap, const Params *__restrict__ P,
                                                            const uint32_t *__restrict__ start, const float4 *__restrict__ sorted,
                                                            const float *__restrict__ mean, const float4 *__restrict__ rec,
                                                            const float4 *__restrict__ rec_g, const float *__restrict__ color,
                                                            const float *__restrict__ points,
                                                            float *__restrict__ density, float *__restrict__ grad,
                                                            float *__restrict__ rgb) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= Q) return;
  const float4 q = make_float4(points[3 * (size_t)t], points[3 * (size_t)t + 1], points[3 * (size_t)t + 2], 0.0f);
  unsigned long long list[L];
#pragma unroll
  for (int k = 0; k < L; ++k) list[k] = kPad;
  search_ext<L>(list, cap, P, start, sorted, q);
  float sum = 0.0f, gx = 0.0f, gy = 0.0f, gz = 0.0f;
  float nr = 0.0f, ng = 0.0f, nb = 0.0f, den = 0.0f;
  const bool field = density != nullptr || grad != nullptr;
#pragma unroll
  for (int k = 0; k < L; ++k) {
    const uint32_t j = (uint32_t)(list[k] & 0xffffffffull);
    const bool kept = (uint32_t)k >= skip && field;
    if ((uint32_t)k < K + skip && j != 0xffffffffu && (kept || rgb != nullptr)) {
      const float4 r0 = rec[2 * (size_t)j], r1 = rec[2 * (size_t)j + 1];
      float dx, dy, dz;
      const float tk = density_term(q, mean, r0, r1, j, dx, dy, dz);
      if (kept) {
        sum += tk;
        if (grad != nullptr) {
          const float4 g0 = rec_g[2 * (size_t)j], g1 = rec_g[2 * (size_t)j + 1];
          const float ax = g0.x * dx + g0.y * dy + g0.z * dz;
          const float ay = g0.y * dx + g0.w * dy + g1.x * dz;
          const float az = g0.z * dx + g1.x * dy + g1.y * dz;
          gx -= tk * ax;
          gy -= tk * ay;
          gz -= tk * az;
        }
      }
      if (rgb != nullptr) {
        nr += tk * color[3 * (size_t)j];
        ng += tk * color[3 * (size_t)j + 1];
        nb += tk * color[3 * (size_t)j + 2];
        den += tk;
      }
    }
  }
  if (density != nullptr) density[t] = sum;
  if (grad != nullptr) {
    grad[3 * (size_t)t] = gx;
    grad[3 * (size_t)t + 1] = gy;
    grad[3 * (size_t)t + 2] = gz;
  }
  if (rgb != nullptr) {
    const uint32_t j0 = (uint32_t)(list[0] & 0xffffffffull);
    float r = 0.0f, g = 0.0f, b = 0.0f;
    if (den >= 1.17549435e-38f) {
      r = nr / den, g = ng / den, b = nb / den;
    } else if (j0 != 0xffffffffu) {
      r = color[3 * (size_t)j0], g = color[3 * (size_t)j0 + 1], b = color[3 * (size_t)j0 + 2];
    }
    rgb[3 * (size_t)t] = r;
    rgb[3 * (size_t)t + 1] = g;
    rgb[3 * (size_t)t + 2] = b;
  }
}

// --- 4e. point-cloud normals ------------------------------------------------------------------------------------------------
// pytorch3d's estimate_pointcloud_local_coord_frames (the reference's estimate_normal, utils/ops.py:62-72) fused with the self
// search: the list of k_knn_query<L> for the same K, bit for bit, then from the list in registers (K counts the point itself):
//   d_k = p_jk - p_i per component, list order;  m = (sum_k d_k) / K from 0.0f;  c_k = d_k - m;
//   C_ab = (sum_k c_ka c_kb) / K for the six unique entries, list order (get_point_covariances: divided by K, not K - 1).
// Eigen-decomposition of C: cyclic Jacobi (kJacobiSweeps sweeps over (0,1), (0,2), (1,2)) on C scaled by the power of two that
// brings its largest diagonal entry into [1/2, 1), eigenvalues ascending (`curvature`), frame columns n (smallest), y, z (largest).
// Every element is a named scalar: nothing is indexed at run time.
// disambiguate != 0 (_disambiguate_vector_directions), for v = n and v = z: proj_k = (vx dx + vy dy) + vz dz, n_pos = #{proj_k > 0},
// n_neg = #{proj_k < 0}.  2 n_pos >= K: v; else 2 n_neg >= K: -v (the point itself has proj 0, so at most one holds and the result
// does not depend on the solver's sign).  Neither: the direction with sum_k proj_k > 0 (list order from 0.0f; the sum of -v is the
// negation, exactly); a sum that is not positive either way: first non-zero component positive.  pytorch3d's answer there depends
// on its solver's sign: this is the one place where the result is defined more tightly.  Then y = n x z.
// disambiguate == 0: the solver's three columns, each with its first non-zero component positive.
// A non-finite point and a row short of K finite neighbours write zeros.  normals / curvature / frames may be null (uniform test).
constexpr int kJacobiSweeps = 6;

// One Jacobi rotation in the (p, q) plane of the symmetric matrix (r: the third index) and of the eigenvector columns p, q.
// t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), theta = (a_qq - a_pp) / (2 a_pq): the smaller root, |t| <= 1.  a_pq == 0, or a
// theta whose square overflows: t = 0, nothing moves.
__device__ __forceinline__ void jacobi_rotate(float &app, float &aqq, float &apq, float &arp, float &arq, float &v0p, float &v0q,
                                              float &v1p, float &v1q, float &v2p, float &v2q) {
  float t = 0.0f;
  if (apq != 0.0f) {
    const float theta = (aqq - app) / (2.0f * apq);
    const float r = 1.0f / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
    t = theta < 0.0f ? -r : r;
  }
  const float c = 1.0f / sqrtf(t * t + 1.0f), s = t * c;
  const float h = t * apq;
  app = app - h;
  aqq = aqq + h;
  apq = 0.0f;
  const float rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  const float a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
  v0p = c * a0 - s * b0; v0q = s * a0 + c * b0;
  v1p = c * a1 - s * b1; v1q = s * a1 + c * b1;
  v2p = c * a2 - s * b2; v2q = s * a2 + c * b2;
}

// (lambda_a, column a) <-> (lambda_b, column b) when lambda_a > lambda_b
__device__ __forceinline__ void order_pair(float &la, float &lb, float &a0, float &a1, float &a2, float &b0, float &b1, float &b2) {
  if (la > lb) {
    float w;
    w = la; la = lb; lb = w;
    w = a0; a0 = b0; b0 = w;
    w = a1; a1 = b1; b1 = w;
    w = a2; a2 = b2; b2 = w;
  }
}

__device__ __forceinline__ void unit3(float &x, float &y, float &z) {
  const float n = sqrtf(x * x + y * y + z * z);
  x = x / n; y = y / n; z = z / n;
}

// true: the first non-zero component of (x, y, z) is negative
__device__ __forceinline__ bool first_negative(float x, float y, float z) {
  return x != 0.0f ? x < 0.0f : (y != 0.0f ? y < 0.0f : z < 0.0f);
}

template <int L>
__global__ void __launch_bounds__(kBlock) k_point_normals(uint32_t N, uint32_t K, uint32_t disambiguate, uint32_t cap,
                                                           const Params *__restrict__ P, const uint32_t *__restrict__ start,
                                                           const float4 *__restrict__ sorted, const float *__restrict__ points,
                                                           float *__restrict__ normals, float *__restrict__ curvature,
                                                           float *__restrict__ frames) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= N) return;
  const float4 q = sorted[t];
  const uint32_t qi = __float_as_uint(q.w);
  unsigned long long list[L];
#pragma unroll
  for (int k = 0; k < L; ++k) list[k] = kPad;
  search_self<L>(list, t, cap, P, start, sorted, q);
  const float fK = (float)K;
  // the neighbourhood's mean difference; a padded entry among the first K: a degenerate row
  bool padded = false;
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
#pragma unroll
  for (int k = 0; k < L; ++k) {
    if ((uint32_t)k < K) {
      const uint32_t j = (uint32_t)(list[k] & 0xffffffffull);
      if (j == 0xffffffffu) {
        padded = true;
      } else {
        sx += points[3 * (size_t)j] - q.x;
        sy += points[3 * (size_t)j + 1] - q.y;
        sz += points[3 * (size_t)j + 2] - q.z;
      }
    }
  }
  float nx = 0.0f, ny = 0.0f, nz = 0.0f, yx = 0.0f, yy = 0.0f, yz = 0.0f, zx = 0.0f, zy = 0.0f, zz = 0.0f;
  float l0 = 0.0f, l1 = 0.0f, l2 = 0.0f;
  if (!padded) {
    const float mx = sx / fK, my = sy / fK, mz = sz / fK;
    float c00 = 0.0f, c01 = 0.0f, c02 = 0.0f, c11 = 0.0f, c12 = 0.0f, c22 = 0.0f;
#pragma unroll
    for (int k = 0; k < L; ++k) {
      if ((uint32_t)k < K) {
        const uint32_t j = (uint32_t)(list[k] & 0xffffffffull);
        const float cx = (points[3 * (size_t)j] - q.x) - mx;
        const float cy = (points[3 * (size_t)j + 1] - q.y) - my;
        const float cz = (points[3 * (size_t)j + 2] - q.z) - mz;
        c00 += cx * cx; c01 += cx * cy; c02 += cx * cz;
        c11 += cy * cy; c12 += cy * cz; c22 += cz * cz;
      }
    }
    c00 = c00 / fK; c01 = c01 / fK; c02 = c02 / fK;
    c11 = c11 / fK; c12 = c12 / fK; c22 = c22 / fK;
    // scale by a power of two (exact): the largest diagonal entry, which bounds every entry of a covariance, into [1/2, 1)
    const float big = fmaxf(c00, fmaxf(c11, c22));
    int e = 0;
    if (big > 0.0f && big <= 3.402823466e38f) (void)frexpf(big, &e);
    float a00 = ldexpf(c00, -e), a01 = ldexpf(c01, -e), a02 = ldexpf(c02, -e);
    float a11 = ldexpf(c11, -e), a12 = ldexpf(c12, -e), a22 = ldexpf(c22, -e);
    float v00 = 1.0f, v01 = 0.0f, v02 = 0.0f, v10 = 0.0f, v11 = 1.0f, v12 = 0.0f, v20 = 0.0f, v21 = 0.0f, v22 = 1.0f;
    for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
      jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1), r = 2
      jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2), r = 1
      jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2), r = 0
    }
    // ascending: columns (v00, v10, v20), (v01, v11, v21), (v02, v12, v22) follow their eigenvalues
    order_pair(a00, a11, v00, v10, v20, v01, v11, v21);
    order_pair(a11, a22, v01, v11, v21, v02, v12, v22);
    order_pair(a00, a11, v00, v10, v20, v01, v11, v21);
    l0 = ldexpf(a00, e); l1 = ldexpf(a11, e); l2 = ldexpf(a22, e);
    nx = v00; ny = v10; nz = v20;
    yx = v01; yy = v11; yz = v21;
    zx = v02; zy = v12; zz = v22;
    unit3(nx, ny, nz);
    unit3(zx, zy, zz);
    if (disambiguate != 0) {
      uint32_t n_pos = 0, n_neg = 0, z_pos = 0, z_neg = 0;
      float n_sum = 0.0f, z_sum = 0.0f;
#pragma unroll
      for (int k = 0; k < L; ++k) {
        if ((uint32_t)k < K) {
          const uint32_t j = (uint32_t)(list[k] & 0xffffffffull);
          const float dx = points[3 * (size_t)j] - q.x, dy = points[3 * (size_t)j + 1] - q.y, dz = points[3 * (size_t)j + 2] - q.z;
          const float pn = nx * dx + ny * dy + nz * dz;
          const float pz = zx * dx + zy * dy + zz * dz;
          n_pos += pn > 0.0f ? 1u : 0u; n_neg += pn < 0.0f ? 1u : 0u; n_sum += pn;
          z_pos += pz > 0.0f ? 1u : 0u; z_neg += pz < 0.0f ? 1u : 0u; z_sum += pz;
        }
      }
      bool flip_n, flip_z;
      if (2u * n_pos >= K) flip_n = false;
      else if (2u * n_neg >= K) flip_n = true;
      else if (n_sum > 0.0f) flip_n = false;
      else if (n_sum < 0.0f) flip_n = true;
      else flip_n = first_negative(nx, ny, nz);
      if (2u * z_pos >= K) flip_z = false;
      else if (2u * z_neg >= K) flip_z = true;
      else if (z_sum > 0.0f) flip_z = false;
      else if (z_sum < 0.0f) flip_z = true;
      else flip_z = first_negative(zx, zy, zz);
      if (flip_n) { nx = -nx; ny = -ny; nz = -nz; }
      if (flip_z) { zx = -zx; zy = -zy; zz = -zz; }
      yx = ny * zz - nz * zy;
      yy = nz * zx - nx * zz;
      yz = nx * zy - ny * zx;
    } else {
      unit3(yx, yy, yz);
      if (first_negative(nx, ny, nz)) { nx = -nx; ny = -ny; nz = -nz; }
      if (first_negative(yx, yy, yz)) { yx = -yx; yy = -yy; yz = -yz; }
      if (first_negative(zx, zy, zz)) { zx = -zx; zy = -zy; zz = -zz; }
    }
  }
  if (normals != nullptr) {
    normals[3 * (size_t)qi] = nx; normals[3 * (size_t)qi + 1] = ny; normals[3 * (size_t)qi + 2] = nz;
  }
  if (curvature != nullptr) {
    curvature[3 * (size_t)qi] = l0; curvature[3 * (size_t)qi + 1] = l1; curvature[3 * (size_t)qi + 2] = l2;
  }
  if (frames != nullptr) {
    float *f = frames + 9 * (size_t)qi;
    f[0] = nx; f[1] = yx; f[2] = zx;
    f[3] = ny; f[4] = yy; f[5] = zy;
    f[6] = nz; f[7] = yz; f[8] = zz;
  }
}

template <int L>
inline void launch_point_normals(uint32_t N, uint32_t K, uint32_t disambiguate, uint32_t cap, const Ws &w, const float *points,
                                 float *normals, float *curvature, float *frames, hipStream_t s) {
  hipLaunchKernelGGL((k_point_normals<L>), dim3((N + kBlock - 1) / kBlock), dim3(kBlock), 0, s, N, K, disambiguate, cap,
                     (const Params *)w.P, (const uint32_t *)w.start, (const float4 *)w.sorted, points, normals, curvature, frames);
}

template <int L>
inline void launch_query(uint32_t N, uint32_t K, uint32_t cap, const Ws &w, float *dist2, int32_t *idx, hipStream_t s) {
  hipLaunchKernelGGL((k_knn_query<L>), dim3((N + kBlock - 1) / kBlock), dim3(kBlock), 0, s, N, K, cap, (const Params *)w.P,
                     (const uint32_t *)w.start, (const float4 *)w.sorted, dist2, idx);
}

template <int L>
inline void launch_query_ext(uint32_t Q, uint32_t K, uint32_t cap, const Ws &w, const float *queries, float *dist2, int32_t *idx,
                             hipStream_t s) {
  hipLaunchKernelGGL((k_knn_query_ext<L>), dim3((Q + kBlock - 1) / kBlock), dim3(kBlock), 0, s, Q, K, cap, (const Params *)w.P,
                     (const uint32_t *)w.start, (const float4 *)w.sorted, queries, dist2, idx);
}

template <int L>
inline void launch_density(uint32_t blocks, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t K, uint32_t skip, uint32_t cap, const Ws &w,
                           const float *mean, const float4 *rec, const float *ax, const float *ay, const float *az, float *out,
                           hipStream_t s) {
  hipLaunchKernelGGL((k_density_grid<L>), dim3(blocks), dim3(kBlock), 0, s, nx, ny, nz, K, skip, cap, (const Params *)w.P,
                     (const uint32_t *)w.start, (const float4 *)w.sorted, mean, rec, ax, ay, az, out);
}

template <int L>
inline void launch_density_points(uint32_t Q, uint32_t K, uint32_t skip, uint32_t cap, const Ws &w, const float *mean, const float4 *rec,
                                  const float4 *rec_g, const float *color, const float *points, float *density, float *grad, float *rgb, hipStream_t s) {
  hipLaunchKernelGGL((k_density_points<L>), dim3((uint32_t)(((uint64_t)Q + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, Q, K, skip, cap,
                     (const Params *)w.P, (const uint32_t *)w.start, (const float4 *)w.sorted, mean, rec, rec_g, color, points, density,
                     grad, rgb);
}

// the records of k_density_prep behind the index's workspace
inline size_t density_rec_offset(uint32_t N, uint32_t K) { return align256(carve(nullptr, N, K).bytes); }

}  // namespace gs_knn

using namespace gs_knn;

extern "C" {

size_t gsgen_knn_workspace_bytes(uint32_t n_points, uint32_t K) {
  if (n_points == 0 || K == 0 || K > 32) return 0;
  return carve(nullptr, n_points, K).bytes;
}

int gsgen_knn(const float *points, uint32_t n_points, uint32_t K, float *dist2, int32_t *idx, void *workspace,
              size_t workspace_bytes, gsgen_stream_t stream) {
  if (K == 0 || K > 32) return GSGEN_EUNSUPPORTED;
  if (n_points == 0 || K > n_points || n_points > 0x7fffffffu) return GSGEN_EINVAL;
  if (!points || !dist2 || !idx || !workspace) return GSGEN_EINVAL;
  const uint32_t N = n_points;
  const Ws w = carve(workspace, N, K);
  if (w.bytes > workspace_bytes) return GSGEN_EWORKSPACE;
  const uint32_t cap = cell_cap(N, K);
  hipStream_t s = (hipStream_t)stream;
  if (int e = build_index(points, N, K, w, s)) return e;
  if (K <= 1) launch_query<1>(N, K, cap, w, dist2, idx, s);
  else if (K <= 2) launch_query<2>(N, K, cap, w, dist2, idx, s);
  else if (K <= 4) launch_query<4>(N, K, cap, w, dist2, idx, s);
  else if (K <= 8) launch_query<8>(N, K, cap, w, dist2, idx, s);
  else if (K <= 16) launch_query<16>(N, K, cap, w, dist2, idx, s);
  else launch_query<32>(N, K, cap, w, dist2, idx, s);
  return (int)hipGetLastError();
}

size_t gsgen_knn_query_workspace_bytes(uint32_t n_points, uint32_t n_queries, uint32_t K) {
  (void)n_queries;  // (the queries are read in place: the workspace is the index)
  if (n_points == 0 || K == 0 || K > 32) return 0;
  return carve(nullptr, n_points, K).bytes;
}

int gsgen_knn_query(const float *points, uint32_t n_points, const float *queries, uint32_t n_queries, uint32_t K, float *dist2,
                    int32_t *idx, void *workspace, size_t workspace_bytes, gsgen_stream_t stream) {
  if (K == 0 || K > 32) return GSGEN_EUNSUPPORTED;
  if (n_points == 0 || K > n_points || n_points > 0x7fffffffu) return GSGEN_EINVAL;
  if (n_queries == 0) return 0;
  if (!points || !queries || !dist2 || !idx || !workspace) return GSGEN_EINVAL;
  const uint32_t N = n_points, Q = n_queries;
  const Ws w = carve(workspace, N, K);
  if (w.bytes > workspace_bytes) return GSGEN_EWORKSPACE;
  const uint32_t cap = cell_cap(N, K);
  hipStream_t s = (hipStream_t)stream;
  if (int e = build_index(points, N, K, w, s)) return e;
  if (K <= 1) launch_query_ext<1>(Q, K, cap, w, queries, dist2, idx, s);
  else if (K <= 2) launch_query_ext<2>(Q, K, cap, w, queries, dist2, idx, s);
  else if (K <= 4) launch_query_ext<4>(Q, K, cap, w, queries, dist2, idx, s);
  else if (K <= 8) launch_query_ext<8>(Q, K, cap, w, queries, dist2, idx, s);
  else if (K <= 16) launch_query_ext<16>(Q, K, cap, w, queries, dist2, idx, s);
  else launch_query_ext<32>(Q, K, cap, w, queries, dist2, idx, s);
  return (int)hipGetLastError();
}

size_t gsgen_point_normals_workspace_bytes(uint32_t n_points, uint32_t K) {
  if (n_points == 0 || K < 3 || K > 64) return 0;
  return carve(nullptr, n_points, K).bytes;
}

int gsgen_point_normals(const float *points, uint32_t n_points, uint32_t K, uint32_t disambiguate, float *normals, float *curvature,
                        float *frames, void *workspace, size_t workspace_bytes, gsgen_stream_t stream) {
  if (K < 3 || K > 64) return GSGEN_EUNSUPPORTED;
  if (n_points == 0 || K >= n_points || n_points > 0x7fffffffu) return GSGEN_EINVAL;
  if (!points || !workspace || (!normals && !curvature && !frames)) return GSGEN_EINVAL;
  const uint32_t N = n_points;
  const Ws w = carve(workspace, N, K);
  if (w.bytes > workspace_bytes) return GSGEN_EWORKSPACE;
  const uint32_t cap = cell_cap(N, K);
  hipStream_t s = (hipStream_t)stream;
  if (int e = build_index(points, N, K, w, s)) return e;
  if (K <= 4) launch_point_normals<4>(N, K, disambiguate, cap, w, points, normals, curvature, frames, s);
  else if (K <= 8) launch_point_normals<8>(N, K, disambiguate, cap, w, points, normals, curvature, frames, s);
  else if (K <= 16) launch_point_normals<16>(N, K, disambiguate, cap, w, points, normals, curvature, frames, s);
  else if (K <= 32) launch_point_normals<32>(N, K, disambiguate, cap, w, points, normals, curvature, frames, s);
  else launch_point_normals<64>(N, K, disambiguate, cap, w, points, normals, curvature, frames, s);  // (the one 64-entry list)
  return (int)hipGetLastError();
}

size_t gsgen_density_grid_workspace_bytes(uint32_t n_points, uint32_t K) {
  // (the index of a K + 1 search has no more cells than that of a K search: this size serves skip_nearest 0 and 1)
  if (n_points == 0 || K == 0 || K > 32) return 0;
  return density_rec_offset(n_points, K) + align256(2 * sizeof(float4) * (size_t)n_points) + 256;
}

int gsgen_density_grid(const float *mean, const float *qvec, const float *scale, const float *opacity, uint32_t N, const float *axis_x,
                       const float *axis_y, const float *axis_z, uint32_t nx, uint32_t ny, uint32_t nz, uint32_t K,
                       uint32_t skip_nearest, float *out, void *workspace, size_t workspace_bytes, gsgen_stream_t stream) {
  if (skip_nearest > 1) return GSGEN_EINVAL;
  const uint32_t Ks = K + skip_nearest;  // the list that is searched
  if (K == 0 || K > 32 || Ks > 32) return GSGEN_EUNSUPPORTED;
  if (N == 0 || Ks > N || N > 0x7fffffffu) return GSGEN_EINVAL;
  if (nx == 0 || ny == 0 || nz == 0) return 0;
  if (!mean || !qvec || !scale || !opacity || !axis_x || !axis_y || !axis_z || !out || !workspace) return GSGEN_EINVAL;
  const unsigned long long bricks = (unsigned long long)((nx + 3) / 4) * ((ny + 3) / 4) * ((nz + 3) / 4);
  if (bricks > 0x7fffffffull) return GSGEN_EINVAL;
  if (gsgen_density_grid_workspace_bytes(N, K) > workspace_bytes) return GSGEN_EWORKSPACE;
  const Ws w = carve(workspace, N, Ks);
  // (behind the index of the K search's size, which is the larger: one layout for both values of skip_nearest)
  float4 *rec = (float4 *)((char *)w.P + density_rec_offset(N, K));
  const uint32_t cap = cell_cap(N, Ks);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_density_prep, dim3((N + kBlock - 1) / kBlock), dim3(kBlock), 0, s, N, qvec, scale, opacity, rec, (float4 *)nullptr);
  if (int e = build_index(mean, N, Ks, w, s)) return e;
  const uint32_t blocks = (uint32_t)((bricks + kBlock / 64 - 1) / (kBlock / 64));
  if (Ks <= 1) launch_density<1>(blocks, nx, ny, nz, K, skip_nearest, cap, w, mean, rec, axis_x, axis_y, axis_z, out, s);
  else if (Ks <= 2) launch_density<2>(blocks, nx, ny, nz, K, skip_nearest, cap, w, mean, rec, axis_x, axis_y, axis_z, out, s);
  else if (Ks <= 4) launch_density<4>(blocks, nx, ny, nz, K, skip_nearest, cap, w, mean, rec, axis_x, axis_y, axis_z, out, s);
  else if (Ks <= 8) launch_density<8>(blocks, nx, ny, nz, K, skip_nearest, cap, w, mean, rec, axis_x, axis_y, axis_z, out, s);
  else if (Ks <= 16) launch_density<16>(blocks, nx, ny, nz, K, skip_nearest, cap, w, mean, rec, axis_x, axis_y, axis_z, out, s);
  else launch_density<32>(blocks, nx, ny, nz, K, skip_nearest, cap, w, mean, rec, axis_x, axis_y, axis_z, out, s);
  return (int)hipGetLastError();
}

size_t gsgen_density_points_workspace_bytes(uint32_t n_points, uint32_t K) {
  // (the lattice's layout, then the gradient's records)
  const size_t grid = gsgen_density_grid_workspace_bytes(n_points, K);
  return grid == 0 ? 0 : grid + align256(2 * sizeof(float4) * (size_t)n_points);
}

int gsgen_density_points(const float *mean, const float *qvec, const float *scale, const float *opacity, const float *color, uint32_t N,
                         const float *points, uint32_t Q, uint32_t K, uint32_t skip_nearest, float *density, float *grad, float *rgb,
                         void *workspace, size_t workspace_bytes, gsgen_stream_t stream) {
  if (skip_nearest > 1) return GSGEN_EINVAL;
  const uint32_t Ks = K + skip_nearest;  // the list that is searched
  if (K == 0 || K > 32 || Ks > 32) return GSGEN_EUNSUPPORTED;
  if (N == 0 || Ks > N || N > 0x7fffffffu) return GSGEN_EINVAL;
  if (rgb && !color) return GSGEN_EINVAL;
  if (Q == 0) return 0;
  if (!mean || !qvec || !scale || !opacity || !points || !workspace) return GSGEN_EINVAL;
  if (gsgen_density_points_workspace_bytes(N, K) > workspace_bytes) return GSGEN_EWORKSPACE;
  if (!density && !grad && !rgb) return 0;  // (nothing asked for)
  const Ws w = carve(workspace, N, Ks);
  float4 *rec = (float4 *)((char *)w.P + density_rec_offset(N, K));  // (the lattice's layout)
  float4 *rec_g = (float4 *)((char *)rec + align256(2 * sizeof(float4) * (size_t)N));
  const uint32_t cap = cell_cap(N, Ks);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_density_prep, dim3((N + kBlock - 1) / kBlock), dim3(kBlock), 0, s, N, qvec, scale, opacity, rec, rec_g);
  if (int e = build_index(mean, N, Ks, w, s)) return e;
  if (Ks <= 1) launch_density_points<1>(Q, K, skip_nearest, cap, w, mean, rec, rec_g, color, points, density, grad, rgb, s);
  else if (Ks <= 2) launch_density_points<2>(Q, K, skip_nearest, cap, w, mean, rec, rec_g, color, points, density, grad, rgb, s);
  else if (Ks <= 4) launch_density_points<4>(Q, K, skip_nearest, cap, w, mean, rec, rec_g, color, points, density, grad, rgb, s);
  else if (Ks <= 8) launch_density_points<8>(Q, K, skip_nearest, cap, w, mean, rec, rec_g, color, points, density, grad, rgb, s);
  else if (Ks <= 16) launch_density_points<16>(Q, K, skip_nearest, cap, w, mean, rec, rec_g, color, points, density, grad, rgb, s);
  else launch_density_points<32>(Q, K, skip_nearest, cap, w, mean, rec, rec_g, color, points, density, grad, rgb, s);
  return (int)hipGetLastError();
}

}  // extern "C"
