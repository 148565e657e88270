// marching_cubes.hip -- marching cubes over a dense fp32 lattice, for gfx950 (compiled with -ffp-contract=off): the last step of
// the reference's mesh export (utils/export.py:123-155, which calls PyMCubes on the host).
//
// Input: grid[X][Y][Z], x slowest (the layout gsgen_density_grid writes), and a threshold.  With s = grid - thresh in fp32 a
// lattice point is INSIDE iff s > 0 (a NaN is outside) -- the convention of the reference's in-tree marching cubes
// (shap_e/rendering/mc.py: field > 0), which is this file's oracle.  PyMCubes itself is not pinned: its tie-breaking at
// value == thresh and its triangle order may differ.
//
// Vertices: one per lattice edge whose end points differ in insideness, ordered as the reference orders them: all x-edges, then
// all y-edges, then all z-edges, each axis in the raster order (x slowest) of the edge's lower point.  In lattice index
// coordinates, with p1 the lower point, p2 = p1 + e_axis, s1 = s(p1), s2 = s(p2):
//   t = s1 / (s1 - s2),  v = t * p2 + (1 - t) * p1            (all three components: t * c + (1 - t) * c need not round to c)
// -ffp-contract=off: these are the reference's fp32 operations in the reference's order, and a fused multiply-add would round
// once where it rounds twice.  The vertices are bit-equal to the reference's where its own v / (n - 1) * (n - 1) round trip is
// exact (n - 1 a power of two per axis), and the g++ build of this file on the CPU emulator (tests/test_mesh_host.py) computes
// what the GPU computes.
//
// Triangles: every cube (lower point p, x < X-1, y < Y-1, z < Z-1) has an 8-bit case, bit dx + 2 dy + 4 dz set when that corner
// is inside, and emits the 0..5 triangles of mc_table.inc (generated and checked by tools/gen_mc_table.py) in cube raster order;
// a triangle holds the vertex ids of three of the cube's edges.  Normals point from inside to outside.
//
// Launches (a workgroup of kBlock = 256 threads owns a TILE of kTile = 1024 consecutive points of the raster, a thread 4
// consecutive points; the tile reads 4 KiB runs along z from each of the four lattice rows a point's cube touches):
//   k_mc_count       classifies the tile's points (x-, y-, z-edge flags, triangles of the cube; the insideness of the four rows is
//                    staged in LDS, 16 KiB, so each global load of a wave is 256 contiguous bytes), block-scans the four counters
//                    (packed two by two into 32-bit words: at most 1024 edges of an axis and 5120 triangles per tile), writes
//                    per tile the four sums and, in a tile that has a vertex, per point ONE word with its three exclusive in-tile
//                    vertex offsets (10 bits each).
//   k_mc_scan<false> sums of 1024 tiles -> super-tile sums;
//   k_mc_scan_super  one workgroup scans the <= 1024 super-tile sums and writes the totals and counts = {V, F, overflow};
//   k_mc_scan<true>  the exclusive base of every tile (the three-level pattern of knn_index.hpp's k_knn_scan_*, four counters
//                    wide, with its block_inclusive_scan).
//   k_mc_emit        (skipped by the counting call) a tile without vertices and triangles returns at once; otherwise it
//                    classifies again, writes its vertices at base + in-tile offset, block-scans its triangle counts and writes
//                    the triangles.  A triangle's vertices belong to edges owned by up to 7 points that may lie in other tiles:
//                    their ids come from those points' offset words and those tiles' bases in the workspace.
// Workspace: 4 bytes per lattice point + 32 bytes per tile.  No atomics, no host synchronisation, nothing read from the
// environment, launch shapes from X, Y, Z alone: capturable, bit-identical from run to run.  Rows past a capacity are not written.
// Limits: X * Y * Z <= 2^30 (point indices and their neighbours stay below 2^31); counters are 32-bit, so F < 2^32 is assumed
// (V <= 3 * 2^30 always holds).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gsgen_hip.h"

#define GSGEN_INDEX_NS gs_mc_index  // (block_inclusive_scan; one kernel namespace per translation unit, see knn_index.hpp)
#include "knn_index.hpp"

namespace gs_mc {

using gs_mc_index::block_inclusive_scan;

constexpr int kBlock = 256;
constexpr int kPer = 4;                  // consecutive points of one thread
constexpr uint32_t kTile = kBlock * kPer;  // points of one workgroup
constexpr uint32_t kMaxPoints = 1u << 30;
static_assert(kTile == 1024, "the offset word holds three 10-bit in-tile offsets, the scans 1024 entries per workgroup");

#include "mc_table.inc"

struct Dims {
  uint32_t X, Y, Z, YZ, N;
};

// what one thread knows about its kPer points: bits 0..2 of flag = the x-, y-, z-edge starting at the point changes sign;
// cs = the case of the cube whose lower corner the point is (0 where there is no such cube: no triangles, like case 0)
struct Cls {
  uint32_t flag[kPer], cs[kPer];
};

__device__ __forceinline__ uint32_t ntri_of(uint32_t cs) { return kMcTable[cs * 16 + 15]; }

// The workgroup stages the insideness of the points base .. base + kTile (one more than its own: the +z neighbour of the last) of
// the four rows (0, +Z, +YZ, +YZ+Z) in LDS, lane after lane along z -- every global load instruction of a wave reads 256
// contiguous bytes, each lattice value once per row --, then a thread reads the 4 x 5 flags of its kPer consecutive points.  A
// point out of range reads as outside and is masked below.  Called once per kernel by all threads of the workgroup.
__device__ __forceinline__ Cls classify(const float *__restrict__ grid, const Dims d, float thresh) {
  __shared__ uint32_t s_in[4][kTile + 4];
  const uint32_t base = blockIdx.x * kTile;
  const uint32_t row[4] = {0u, d.Z, d.YZ, d.YZ + d.Z};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const uint32_t l = threadIdx.x + k * kBlock, j = base + row[r] + l;
      s_in[r][l] = j < d.N ? (uint32_t)(grid[j] - thresh > 0.0f) : 0u;
    }
    if (threadIdx.x == 0) {
      const uint32_t j = base + row[r] + kTile;
      s_in[r][kTile] = j < d.N ? (uint32_t)(grid[j] - thresh > 0.0f) : 0u;
    }
  }
  __syncthreads();
  const uint32_t l0 = threadIdx.x * kPer, i0 = base + l0;
  uint32_t in[4][kPer + 1];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int k = 0; k <= kPer; ++k) in[r][k] = s_in[r][l0 + k];
  uint32_t z = i0 % d.Z, y = (i0 / d.Z) % d.Y, x = i0 / d.YZ;
  Cls c;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const bool live = i0 + k < d.N, hx = live && x + 1 < d.X, hy = live && y + 1 < d.Y, hz = live && z + 1 < d.Z;
    const uint32_t a = in[0][k];
    c.flag[k] = (hx && a != in[2][k] ? 1u : 0u) | (hy && a != in[1][k] ? 2u : 0u) | (hz && a != in[0][k + 1] ? 4u : 0u);
    c.cs[k] = hx && hy && hz ? (a | in[2][k] << 1 | in[1][k] << 2 | in[3][k] << 3 | in[0][k + 1] << 4 | in[2][k + 1] << 5 |
                                in[1][k + 1] << 6 | in[3][k + 1] << 7)
                             : 0u;
    if (++z == d.Z) { z = 0; if (++y == d.Y) { y = 0; ++x; } }
  }
  return c;
}

// offs[i] = in-tile exclusive offsets of point i's x- | y- << 10 | z-vertex << 20 (written only in tiles that have a vertex: nothing
// reads the others); sums[tile] = {x, y, z vertices, triangles}
__global__ void __launch_bounds__(kBlock) k_mc_count(const float *__restrict__ grid, Dims d, float thresh, uint32_t *__restrict__ offs,
                                                      uint32_t *__restrict__ sums) {
  __shared__ uint32_t wt[4];
  __shared__ uint32_t any_vertex;
  const uint32_t i0 = blockIdx.x * kTile + threadIdx.x * kPer;
  const Cls c = classify(grid, d, thresh);
  uint32_t xy = 0, zt = 0;  // x | y << 16,  z | triangles << 16
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    xy += (c.flag[k] & 1u) + ((c.flag[k] >> 1 & 1u) << 16);
    zt += (c.flag[k] >> 2 & 1u) + (ntri_of(c.cs[k]) << 16);
  }
  const uint32_t ixy = block_inclusive_scan(xy, wt), izt = block_inclusive_scan(zt, wt);
  if (threadIdx.x == kBlock - 1) {
    uint32_t *o = sums + 4 * (size_t)blockIdx.x;
    o[0] = ixy & 0xffffu; o[1] = ixy >> 16; o[2] = izt & 0xffffu; o[3] = izt >> 16;
    any_vertex = ixy | (izt & 0xffffu);
  }
  __syncthreads();
  if (any_vertex == 0u) return;  // (the whole workgroup)
  uint32_t rx = (ixy - xy) & 0xffffu, ry = (ixy - xy) >> 16, rz = (izt - zt) & 0xffffu, w[kPer];
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    w[k] = rx | ry << 10 | rz << 20;
    rx += c.flag[k] & 1u; ry += c.flag[k] >> 1 & 1u; rz += c.flag[k] >> 2 & 1u;
  }
  if (i0 + kPer <= d.N) {  // (offs is 256-byte aligned and i0 a multiple of 4: one 16-byte store)
    uint4 v;
    v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    *reinterpret_cast<uint4 *>(offs + i0) = v;
  } else {
#pragma unroll
    for (int k = 0; k < kPer; ++k)
      if (i0 + k < d.N) offs[i0 + k] = w[k];
  }
}

// APPLY false: super[b][c] = sum of the entries [1024 b, 1024 b + 1024) of in[.][c];  true: out[t][c] = exclusive scan of in[.][c]
// (in and out may not alias), starting from super[b][c] (then the exclusive scan of the super sums)
template <bool APPLY>
__global__ void __launch_bounds__(kBlock) k_mc_scan(uint32_t T, const uint32_t *__restrict__ in, uint32_t *__restrict__ super,
                                                     uint32_t *__restrict__ out) {
  __shared__ uint32_t wt[4];
  const uint32_t t0 = blockIdx.x * kTile + threadIdx.x * kPer;
  uint32_t v[kPer][4], s[4] = {0, 0, 0, 0};
#pragma unroll
  for (int k = 0; k < kPer; ++k)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[k][c] = t0 + k < T ? in[4 * (size_t)(t0 + k) + c] : 0u;
      s[c] += v[k][c];
    }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const uint32_t inc = block_inclusive_scan(s[c], wt);
    if (APPLY) {
      uint32_t run = inc - s[c] + super[4 * (size_t)blockIdx.x + c];
#pragma unroll
      for (int k = 0; k < kPer; ++k) {
        if (t0 + k < T) out[4 * (size_t)(t0 + k) + c] = run;
        run += v[k][c];
      }
    } else if (threadIdx.x == kBlock - 1) {
      super[4 * (size_t)blockIdx.x + c] = inc;
    }
  }
}

// super[b][c] -> its exclusive scan (S <= 1024 entries, one workgroup); totals[c]; counts = {V, F, a capacity is exceeded}
__global__ void __launch_bounds__(kBlock) k_mc_scan_super(uint32_t S, uint32_t *__restrict__ super, uint32_t *__restrict__ totals,
                                                           uint32_t vcap, uint32_t tcap, uint32_t *__restrict__ counts) {
  __shared__ uint32_t wt[4];
  __shared__ uint32_t carry[4];
  if (threadIdx.x < 4) carry[threadIdx.x] = 0;
  __syncthreads();
  for (uint32_t b0 = 0; b0 < S; b0 += kBlock) {
    const uint32_t b = b0 + threadIdx.x;
    for (int c = 0; c < 4; ++c) {
      const uint32_t v = b < S ? super[4 * (size_t)b + c] : 0u;
      const uint32_t inc = block_inclusive_scan(v, wt);
      const uint32_t cr = carry[c];
      if (b < S) super[4 * (size_t)b + c] = cr + inc - v;
      __syncthreads();
      if (threadIdx.x == kBlock - 1) carry[c] = cr + inc;
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    const uint32_t V = carry[0] + carry[1] + carry[2], F = carry[3];
    for (int c = 0; c < 4; ++c) totals[c] = carry[c];
    counts[0] = V; counts[1] = F; counts[2] = (V > vcap || F > tcap) ? 1u : 0u;
  }
}

// the id of the vertex on edge e (4 axis + a + 2 b, mc_table.inc) of the cube with lower point i
__device__ __forceinline__ uint32_t vertex_id(uint32_t i, uint32_t e, const Dims d, const uint32_t *__restrict__ offs,
                                              const uint32_t *__restrict__ bases, const uint32_t *axis_first) {
  const uint32_t axis = e >> 2, a = e & 1u, b = e >> 1 & 1u;
  const uint32_t sa = axis == 0 ? d.Z : d.YZ, sb = axis == 2 ? d.Z : 1u;  // (a, b): the two other axes in ascending order
  const uint32_t q = i + a * sa + b * sb;
  return axis_first[axis] + bases[4 * (size_t)(q / kTile) + axis] + (offs[q] >> (10 * axis) & 1023u);
}

__global__ void __launch_bounds__(kBlock) k_mc_emit(const float *__restrict__ grid, Dims d, float thresh, const uint32_t *__restrict__ offs,
                                                     const uint32_t *__restrict__ sums, const uint32_t *__restrict__ bases,
                                                     const uint32_t *__restrict__ totals, float *__restrict__ verts, uint32_t vcap,
                                                     int32_t *__restrict__ tris, uint32_t tcap) {
  __shared__ uint32_t wt[4];
  const uint32_t *sm = sums + 4 * (size_t)blockIdx.x;
  if ((sm[0] | sm[1] | sm[2] | sm[3]) == 0u) return;  // (the whole workgroup: nothing to write, no barrier below is reached)
  const uint32_t i0 = blockIdx.x * kTile + threadIdx.x * kPer;
  const Cls c = classify(grid, d, thresh);
  const uint32_t axis_first[3] = {0u, totals[0], totals[0] + totals[1]};
  const uint32_t *bs = bases + 4 * (size_t)blockIdx.x;
  const uint32_t stride[3] = {d.YZ, d.Z, 1u};

  uint32_t z = i0 % d.Z, y = (i0 / d.Z) % d.Y, x = i0 / d.YZ;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const uint32_t i = i0 + k;
    if (c.flag[k]) {  // (only a live point has a flag)
      const uint32_t w = offs[i];
      const float s1 = grid[i] - thresh;
      const float p1[3] = {(float)x, (float)y, (float)z};
#pragma unroll
      for (int axis = 0; axis < 3; ++axis) {
        if (!(c.flag[k] >> axis & 1u)) continue;
        const uint32_t row = axis_first[axis] + bs[axis] + (w >> (10 * axis) & 1023u);
        if (row >= vcap) continue;
        const float s2 = grid[i + stride[axis]] - thresh;
        const float t = s1 / (s1 - s2), u = 1.0f - t;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
          const float p2 = m == axis ? p1[m] + 1.0f : p1[m];
          verts[3 * (size_t)row + m] = t * p2 + u * p1[m];
        }
      }
    }
    if (++z == d.Z) { z = 0; if (++y == d.Y) { y = 0; ++x; } }
  }

  uint32_t n = 0;
#pragma unroll
  for (int k = 0; k < kPer; ++k) n += ntri_of(c.cs[k]);
  uint32_t run = block_inclusive_scan(n, wt) - n + bs[3];
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const uint32_t nt = ntri_of(c.cs[k]);
    const uint8_t *tab = kMcTable + c.cs[k] * 16;
    for (uint32_t j = 0; j < nt; ++j, ++run) {
      if (run >= tcap) continue;
#pragma unroll
      for (int m = 0; m < 3; ++m) tris[3 * (size_t)run + m] = (int32_t)vertex_id(i0 + k, tab[3 * j + m], d, offs, bases, axis_first);
    }
  }
}

// --- host side ---------------------------------------------------------------------------------------------------------
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

inline int check_dims(uint32_t X, uint32_t Y, uint32_t Z) {
  if (X < 2 || Y < 2 || Z < 2) return GSGEN_EUNSUPPORTED;
  if ((uint64_t)X * Y > kMaxPoints || (uint64_t)X * Y * Z > kMaxPoints) return GSGEN_EUNSUPPORTED;
  return 0;
}

struct McWs {
  uint32_t *offs;    // [N]
  uint32_t *sums;    // [T][4]
  uint32_t *bases;   // [T][4]
  uint32_t *super;   // [S][4]
  uint32_t *totals;  // [4]
  uint32_t T, S;
  size_t bytes;
};

inline McWs carve_mc(void *base, uint32_t N) {
  char *p0 = (char *)base, *p = p0 + ((256 - ((uintptr_t)p0 & 255)) & 255);
  McWs w;
  w.T = (N + kTile - 1) / kTile;
  w.S = (w.T + kTile - 1) / kTile;
  size_t off = 0;
  auto take = [&](size_t b) { char *r = p + off; off += align256(b); return r; };
  w.offs = (uint32_t *)take(sizeof(uint32_t) * (size_t)N);
  w.sums = (uint32_t *)take(sizeof(uint32_t) * 4 * (size_t)w.T);
  w.bases = (uint32_t *)take(sizeof(uint32_t) * 4 * (size_t)w.T);
  w.super = (uint32_t *)take(sizeof(uint32_t) * 4 * (size_t)w.S);
  w.totals = (uint32_t *)take(sizeof(uint32_t) * 4);
  w.bytes = off + 256;  // (room for the leading alignment of any base address)
  return w;
}

}  // namespace gs_mc

using namespace gs_mc;

extern "C" {

size_t gsgen_marching_cubes_workspace_bytes(uint32_t X, uint32_t Y, uint32_t Z) {
  if (check_dims(X, Y, Z) != 0) return 0;
  return carve_mc(nullptr, X * Y * Z).bytes;
}

int gsgen_marching_cubes(const float *grid, uint32_t X, uint32_t Y, uint32_t Z, float thresh, float *verts, uint32_t verts_capacity,
                         int32_t *tris, uint32_t tris_capacity, uint32_t *counts, void *workspace, size_t workspace_bytes,
                         gsgen_stream_t stream) {
  if (int e = check_dims(X, Y, Z)) return e;
  if (!grid || !counts || !workspace) return GSGEN_EINVAL;
  if ((verts_capacity && !verts) || (tris_capacity && !tris)) return GSGEN_EINVAL;
  if (verts_capacity > 0x7fffffffu || tris_capacity > 0x7fffffffu) return GSGEN_EINVAL;  // (int32 vertex ids; 3 * row in size_t)
  const Dims d = {X, Y, Z, Y * Z, X * Y * Z};
  const McWs w = carve_mc(workspace, d.N);
  if (w.bytes > workspace_bytes) return GSGEN_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mc_count, dim3(w.T), dim3(kBlock), 0, s, grid, d, thresh, w.offs, w.sums);
  hipLaunchKernelGGL(k_mc_scan<false>, dim3(w.S), dim3(kBlock), 0, s, w.T, (const uint32_t *)w.sums, w.super, (uint32_t *)nullptr);
  hipLaunchKernelGGL(k_mc_scan_super, dim3(1), dim3(kBlock), 0, s, w.S, w.super, w.totals, verts_capacity, tris_capacity, counts);
  hipLaunchKernelGGL(k_mc_scan<true>, dim3(w.S), dim3(kBlock), 0, s, w.T, (const uint32_t *)w.sums, w.super, w.bases);
  if (verts_capacity || tris_capacity)
    hipLaunchKernelGGL(k_mc_emit, dim3(w.T), dim3(kBlock), 0, s, grid, d, thresh, (const uint32_t *)w.offs, (const uint32_t *)w.sums,
                       (const uint32_t *)w.bases, (const uint32_t *)w.totals, verts, verts_capacity, tris, tris_capacity);
  return (int)hipGetLastError();
}

}  // extern "C"
