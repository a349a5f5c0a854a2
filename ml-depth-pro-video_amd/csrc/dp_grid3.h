// The sorted 3-D cell grid over an fp64 point cloud that the stray stage (dp_clean.hip), the voxel grid and the
// hybrid search (dp_normals.hip) and the exact k-NN (dp_mesh.hip) are built on: one copy of its record, its
// four kernels, its key helpers and the 64-lane top-k merge of the two searches.  Only those three files
// include it: a __global__ function in an anonymous namespace is emitted into every translation unit that
// sees it, used or not.  Contraction is off, as in dp_points.h.
#pragma once
#include "dp_points.h"

#pragma clang fp contract(off)

namespace {

constexpr int CELL_BITS = 21;                   // bits per axis of the packed cell key
constexpr int CELL_MAX = (1 << CELL_BITS) - 2;  // largest cell coordinate (its +1 neighbour still fits)
constexpr u64 NO_KEY = ~0ull;                   // key of a row that takes no part (sorts last)

// A search of radius r uses cells of edge r * EDGE_SLACK, cell = floor((p - origin) / edge) per axis.  Why
// the 3 x 3 x 3 cells around a point hold every true neighbour: for |xi - xj| < r the exact quotients differ by
// less than 1 / (1 + 2^-20) < 1 - 2^-21; the computed quotient (a subtraction, a division and the edge
// itself, each rounded once) is within 2^-50 relative of the exact one and below 2^21, so within
// 2^-29 absolute; the computed quotients therefore differ by less than 1 and their floors by at most
// 1.  Cells only select candidates: the distance test runs on the original coordinates.
// r * EDGE_SLACK is one IEEE multiply wherever it is done; every caller does it on the host.
constexpr double EDGE_SLACK = 1.0 + 1.0 / 1048576.0;

// First member of each stage's header, which keeps only the stage's own counters beside it.
struct Grid3 {
  u64 mm[6];            // keys of min / max of x, y, z over the finite rows
  uint32_t finite, nonfinite;
  uint32_t err;         // an axis needs more than CELL_MAX cells: every key is NO_KEY
  int32_t ext[4];       // largest cell coordinate per axis
  double org[3], edge;  // cell = floor((p - org) / edge)
};

__device__ __forceinline__ void grid3_reset(Grid3* g) {
  for (int a = 0; a < 3; ++a) { g->mm[2 * a] = ~0ull; g->mm[2 * a + 1] = 0; g->org[a] = 0.0; }
  for (int a = 0; a < 4; ++a) g->ext[a] = 0;
  g->finite = g->nonfinite = g->err = 0;
  g->edge = 0.0;
}

__global__ void __launch_bounds__(256) minmax3_kernel(const double* __restrict__ pts, const int32_t* n_dev, int n_max,
                                                      Grid3* g) {
  const int n = live_n(n_dev, n_max);
  u64 mn[3] = {~0ull, ~0ull, ~0ull}, mx[3] = {0, 0, 0};
  uint32_t bad = 0, good = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    if (!finite3(x, y, z)) { ++bad; continue; }
    ++good;
    const u64 k[3] = {okey(x), okey(y), okey(z)};
    #pragma unroll
    for (int a = 0; a < 3; ++a) { mn[a] = k[a] < mn[a] ? k[a] : mn[a]; mx[a] = k[a] > mx[a] ? k[a] : mx[a]; }
  }
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    wave_minmax(mn, mx, o);
    bad += __shfl_xor(bad, o);
    good += __shfl_xor(good, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (good) {
      flush_minmax(g->mm, mn, mx);
      atomicAdd(&g->finite, good);
    }
    if (bad) atomicAdd(&g->nonfinite, bad);
  }
}

// origin = min - shift per axis, the largest cell per axis, and the error word if an axis needs more than
// CELL_MAX cells of `edge`.  min - 0.0 == min for every value unkey returns, so a shift of 0 puts the origin
// on the minimum bit for bit.  Only the exact k-NN reads ext; the others pay one cell_of per axis for it here.
__global__ void grid3_setup_kernel(Grid3* g, double edge, double shift) {
  bool err = false;
  for (int a = 0; a < 3; ++a) {
    const double mn = g->finite ? unkey(g->mm[2 * a]) : 0.0, mx = g->finite ? unkey(g->mm[2 * a + 1]) : 0.0;
    const double org = mn - shift;
    g->org[a] = org;
    if (!((mx - org) / edge < (double)CELL_MAX)) err = true;      // also catches an overflowing extent
    g->ext[a] = (int32_t)cell_of<CELL_MAX>(mx, org, edge);
  }
  g->edge = edge;
  g->err = err;
}

__device__ __forceinline__ u64 pack_cell(u64 cx, u64 cy, u64 cz) { return (cx << (2 * CELL_BITS)) | (cy << CELL_BITS) | cz; }
__device__ __forceinline__ void unpack_cell(u64 key, int& cx, int& cy, int& cz) {
  cx = (int)(key >> (2 * CELL_BITS));
  cy = (int)((key >> CELL_BITS) & ((1 << CELL_BITS) - 1));
  cz = (int)(key & ((1 << CELL_BITS) - 1));
}

// With the error word up every row gets NO_KEY: the searches then find no cell and no neighbour.  (The stray
// stage keeps every row under the flag and does not look at the keys: test_stray_overflow_flag_keeps_everything.)
__global__ void __launch_bounds__(256) cell_key_kernel(const double* __restrict__ pts, const int32_t* n_dev, int n_max,
                                                       const Grid3* g, u64* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int n = live_n(n_dev, n_max);
  const double ox = g->org[0], oy = g->org[1], oz = g->org[2], edge = g->edge;
  const bool err = g->err != 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    keys[i] = !err && finite3(x, y, z) ? pack_cell(cell_of<CELL_MAX>(x, ox, edge), cell_of<CELL_MAX>(y, oy, edge),
                                                   cell_of<CELL_MAX>(z, oz, edge))
                                       : NO_KEY;
    vals[i] = (uint32_t)i;
  }
}

__global__ void __launch_bounds__(256) gather_points_kernel(const double* __restrict__ pts, const uint32_t* __restrict__ idx,
                                                            const int32_t* n_dev, int n_max, double* __restrict__ out) {
  const int n = live_n(n_dev, n_max);
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) {
    const size_t i = row_of(idx[t], n);
    out[3 * t] = pts[3 * i]; out[3 * t + 1] = pts[3 * i + 1]; out[3 * t + 2] = pts[3 * i + 2];
  }
}

// Sorted positions [a, b) of cell row (rx, ry) with z in [zlo, zhi]: its cells are one key range.
__device__ __forceinline__ void cell_row_range(const u64* __restrict__ keys, int n, int rx, int ry, int zlo, int zhi,
                                               int& a, int& b) {
  a = lower_bound(keys, n, pack_cell((u64)rx, (u64)ry, (u64)zlo));
  b = lower_bound(keys, n, pack_cell((u64)rx, (u64)ry, (u64)zhi) + 1);
}

// ---- the 64 smallest (d2, row) pairs of a search, one per lane ------------------------------------------
// (d2 bits, row) pairs, compared as the pair: d2 >= +0.0, so its bit pattern orders as the value does
__device__ __forceinline__ bool pair_less(u64 ka, uint32_t ra, u64 kb, uint32_t rb) { return ka < kb || (ka == kb && ra < rb); }

// compare-exchange with lane ^ j; keep_min says which of the two this lane keeps
__device__ __forceinline__ void cmp_xchg(u64& k, uint32_t& r, int j, bool keep_min) {
  const u64 ok = __shfl_xor(k, j);
  const uint32_t orr = __shfl_xor(r, j);
  const bool other_less = pair_less(ok, orr, k, r);
  if (other_less == keep_min) { k = ok; r = orr; }
}

// Lane l offers the pair (ck, cr) if live.  (bk, br) is the running best, one per lane in ascending order, of
// which the first k count.  What is not below the current k-th smallest can never make the list; a batch with
// no such candidate changes nothing.  Otherwise the batch is sorted across the lanes (bitonic, shuffles) and
// merged: best[l] = min(best[l], batch[63 - l]) is bitonic and holds the 64 smallest of the 128; six more
// steps sort it.  Full-wave shuffles: all 64 lanes must enter together (wave-uniform control flow at the call),
// and the early return is uniform because it hangs on a ballot.
__device__ __forceinline__ void wave_top64_merge(bool live, u64 ck, uint32_t cr, int k, int lane, u64& bk, uint32_t& br) {
  const u64 tk = __shfl(bk, k - 1);
  const uint32_t tr = __shfl(br, k - 1);
  const bool pass = live && pair_less(ck, cr, tk, tr);
  if (!__ballot(pass)) return;
  if (!pass) { ck = NO_KEY; cr = ~0u; }
  #pragma unroll
  for (int kk = 2; kk <= 64; kk <<= 1) {
    #pragma unroll
    for (int j = kk >> 1; j > 0; j >>= 1) cmp_xchg(ck, cr, j, ((lane & j) == 0) == ((lane & kk) == 0));
  }
  const u64 rk = __shfl(ck, 63 - lane);
  const uint32_t rw = __shfl(cr, 63 - lane);
  if (pair_less(rk, rw, bk, br)) { bk = rk; br = rw; }
  #pragma unroll
  for (int j = 32; j > 0; j >>= 1) cmp_xchg(bk, br, j, (lane & j) == 0);
}

// ---- host ----------------------------------------------------------------------------------------------
// After the stage's own reset of the record: minimum / maximum, the grid of `edge` from origin min - shift, and
// (cell key, row) pairs.  `blocks` workgroups for the per-row kernels.  The sort is the caller's.
void grid3_keys(hipStream_t s, Grid3* g, int blocks, const double* points, const int32_t* n_dev, int n_max, double edge,
                double shift, u64* keys, uint32_t* vals) {
  hipLaunchKernelGGL(minmax3_kernel, dim3(blocks), dim3(256), 0, s, points, n_dev, n_max, g);
  hipLaunchKernelGGL(grid3_setup_kernel, dim3(1), dim3(1), 0, s, g, edge, shift);
  hipLaunchKernelGGL(cell_key_kernel, dim3(blocks), dim3(256), 0, s, points, n_dev, n_max, g, keys, vals);
}

}  // namespace
