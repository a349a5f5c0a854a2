// The 2-D cell grids of the occupancy floor plan (dp_floorplan.hip) and its height slices (dp_slices.hip): one
// copy of the grid-extent rule, the wave join of the rasters, the packed morphology with its launch sequence
// and the 8-connected linking.  Only those two files include it: a __global__ function in an anonymous
// namespace is emitted into every translation unit that sees it, used or not.  Contraction is off, as in
// dp_points.h.
// Every kernel here works on a stack of S grids and takes its slice from blockIdx.y: slice s has its cells at
// s * max_cells, its packed words at s * words_cap and its live size in dims[2 s], dims[2 s + 1].  The single
// floor plan is the stack of one.  The lanes of a wave share their slice.
#pragma once
#include "dp_points.h"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t NO_CELL = ~0u;               // parent of a cell that is not set

// ---- extent ---------------------------------------------------------------------------------------
// cells along one axis: (int)ceil(((max + padding) - min) / resolution), or -1 for more than DP_FLOOR_MAX_DIM (NaN included)
__device__ __forceinline__ int axis_cells(double mn, double mx_padded, double res) {
  const double c = __builtin_ceil((mx_padded - mn) / res);
  return c >= 0.0 && c <= (double)DP_FLOOR_MAX_DIM ? (int)c : -1;
}

// Rule 3 of "Occupancy floor plan" from mm = the keys of min x, max x, min z, max z: the origin is the
// minimum less the padding.  Returns the status: 0, or 2 with H = W = 0 for a grid that does not fit.
__device__ __forceinline__ int grid_extent(const u64* mm, double padding, double res, int max_cells, double& ox, double& oz,
                                           int& H, int& W) {
  ox = unkey(mm[0]) - padding;
  oz = unkey(mm[2]) - padding;
  W = axis_cells(ox, unkey(mm[1]) + padding, res);
  H = axis_cells(oz, unkey(mm[3]) + padding, res);
  if (W < 0 || H < 0 || (long long)W * H > max_cells) { H = 0; W = 0; return 2; }
  return 0;
}

// ---- raster ---------------------------------------------------------------------------------------
// One row per lane.  The rows of a wave mostly fall into a few cells (the cloud is in image order), so the
// wave joins its rows cell by cell: the lanes of the first pending lane's cell add their number and the
// largest of their keys with one atomic each, until no lane is pending.  The loop is wave-uniform, and all 64
// lanes must enter it together.
template <typename K>
__device__ __forceinline__ void wave_join_cells(bool valid, int cell, K key, uint32_t* __restrict__ density, K* __restrict__ keys) {
  const int lane = threadIdx.x & 63;
  u64 todo = __ballot(valid);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int lc = __shfl(cell, leader);
    const bool mine = valid && cell == lc;
    const u64 m = __ballot(mine);
    K k = mine ? key : (K)0;
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const K t = __shfl_xor(k, o);
      k = t > k ? t : k;
    }
    if (lane == leader) {
      atomicAdd(&density[lc], (uint32_t)__popcll(m));
      atomicMax(&keys[lc], k);
    }
    todo &= ~m;
  }
}

// ---- morphology -----------------------------------------------------------------------------------
// A row is packed 64 cells to a word, bit i of word j = cell 64 j + i; the bits past W in a row's last
// word are kept 0.

// a packed row's last word: the bits below W
__device__ __forceinline__ u64 tail_mask(int W) { return (W & 63) ? ((1ull << (W & 63)) - 1) : ~0ull; }

// The radius of slice s: from its size on the device, where a size that is not odd or not in
// [1, DP_FLOOR_MAX_KERNEL] is read as 1, or the host's for every slice if there are no sizes.
__device__ __forceinline__ int slice_rad(const int32_t* size_dev, int s, int rad_host) {
  if (!size_dev) return rad_host;
  const int k = size_dev[s];
  return (k >= 1 && k <= DP_FLOOR_MAX_KERNEL && (k & 1)) ? k / 2 : 0;
}

// one wave packs one word: the ballot of "my cell is set"
__global__ void __launch_bounds__(256) pack_kernel(const uint8_t* __restrict__ grid, const int32_t* dims, int max_cells,
                                                   long long words_cap, u64* __restrict__ bits) {
  const int s = blockIdx.y;
  int H, W;
  grid_dims(dims + 2 * s, max_cells, H, W);
  const int WW = (W + 63) >> 6, lane = threadIdx.x & 63;
  const long long words = (long long)H * WW;
  const uint8_t* g = grid + (size_t)s * max_cells;
  u64* out = bits + (size_t)s * words_cap;
  for (long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); t < words; t += (long long)gridDim.x * 4) {
    const int r = (int)(t / WW), gx = (int)(t % WW) * 64 + lane;
    const u64 w = __ballot(gx < W && g[(long long)r * W + gx] != 0);
    if (lane == 0) out[t] = w;
  }
}

__global__ void __launch_bounds__(256) unpack_kernel(const u64* __restrict__ bits, const int32_t* dims, int max_cells,
                                                     long long words_cap, uint8_t* __restrict__ grid) {
  const int s = blockIdx.y;
  int H, W;
  grid_dims(dims + 2 * s, max_cells, H, W);
  const int WW = (W + 63) >> 6;
  const long long cells = (long long)H * W;
  const u64* in = bits + (size_t)s * words_cap;
  uint8_t* g = grid + (size_t)s * max_cells;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < cells; c += (long long)gridDim.x * 256) {
    const int r = (int)(c / W), gx = (int)(c % W);
    g[c] = (uint8_t)((in[(long long)r * WW + (gx >> 6)] >> (gx & 63)) & 1);
  }
}

// Horizontal pass of a (2 rad + 1)-wide row of ones, one thread per word: shifts of the word and its two
// neighbours, ORed (dilation: cells outside the grid read 0) or ANDed (erosion: they read 1).
__global__ void __launch_bounds__(256) morph_h_kernel(const u64* __restrict__ src_all, u64* __restrict__ dst_all,
                                                      const int32_t* dims, int max_cells, long long words_cap,
                                                      const int32_t* size_dev, int rad_host, int erode) {
  const int s = blockIdx.y;
  int H, W;
  grid_dims(dims + 2 * s, max_cells, H, W);
  const int WW = (W + 63) >> 6, rad = slice_rad(size_dev, s, rad_host);
  const long long words = (long long)H * WW;
  const u64* src = src_all + (size_t)s * words_cap;
  u64* dst = dst_all + (size_t)s * words_cap;
  const u64 fill = erode ? ~0ull : 0ull, tail = tail_mask(W);
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < words; t += (long long)gridDim.x * 256) {
    const int j = (int)(t % WW);
    u64 C = src[t];
    if (j == WW - 1) C = (C & tail) | (fill & ~tail);
    const u64 L = j > 0 ? src[t - 1] : fill;
    u64 R = fill;
    if (j + 1 < WW) {
      R = src[t + 1];
      if (j + 1 == WW - 1) R = (R & tail) | (fill & ~tail);
    }
    u64 acc = C;
    for (int k = 1; k <= rad; ++k) {
      const u64 a = (C >> k) | (R << (64 - k)), b = (C << k) | (L >> (64 - k));
      acc = erode ? (acc & a & b) : (acc | a | b);
    }
    dst[t] = j == WW - 1 ? (acc & tail) : acc;
  }
}

// Vertical pass: OR / AND over the 2 rad + 1 row words; a row outside the grid is the neutral element.
__global__ void __launch_bounds__(256) morph_v_kernel(const u64* __restrict__ src_all, u64* __restrict__ dst_all,
                                                      const int32_t* dims, int max_cells, long long words_cap,
                                                      const int32_t* size_dev, int rad_host, int erode) {
  const int s = blockIdx.y;
  int H, W;
  grid_dims(dims + 2 * s, max_cells, H, W);
  const int WW = (W + 63) >> 6, rad = slice_rad(size_dev, s, rad_host);
  const long long words = (long long)H * WW;
  const u64* src = src_all + (size_t)s * words_cap;
  u64* dst = dst_all + (size_t)s * words_cap;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < words; t += (long long)gridDim.x * 256) {
    const int r = (int)(t / WW);
    u64 acc = src[t];
    for (int d = -rad; d <= rad; ++d) {
      const int rr = r + d;
      if (d == 0 || rr < 0 || rr >= H) continue;
      const u64 w = src[t + (long long)d * WW];
      acc = erode ? (acc & w) : (acc | w);
    }
    dst[t] = acc;
  }
}

// ---- 8-connected linking --------------------------------------------------------------------------
// The stacked cell index s * max_cells + c is the union-find's element (dp_points.h).  A set cell starts as
// its own parent, and slice s counts its set cells into fg[s * fg_stride] (a stride in 32-bit words).
__global__ void __launch_bounds__(256) cc_init_kernel(const uint8_t* __restrict__ grid, const int32_t* dims, int max_cells,
                                                      uint32_t* __restrict__ parent, uint32_t* fg, int fg_stride) {
  const int s = blockIdx.y;
  int H, W;
  grid_dims(dims + 2 * s, max_cells, H, W);
  const long long cells = (long long)H * W;
  const size_t at = (size_t)s * max_cells;
  for (long long b = (long long)blockIdx.x * 256; b < cells; b += (long long)gridDim.x * 256) {
    const long long c = b + threadIdx.x;
    const bool set = c < cells && grid[at + c] != 0;
    if (c < cells) parent[at + c] = set ? (uint32_t)(at + c) : NO_CELL;
    wave_count(fg + (size_t)s * fg_stride, set);
  }
}

// Every set cell is joined to its set neighbours to the west, north-west, north and north-east inside its
// slice's dims: each 8-connected pair is seen once, from its later cell, and no set spans two slices.
__global__ void __launch_bounds__(256) cc_link_kernel(const uint8_t* __restrict__ grid, const int32_t* dims, int max_cells,
                                                      uint32_t* __restrict__ parent) {
  const int s = blockIdx.y;
  int H, W;
  grid_dims(dims + 2 * s, max_cells, H, W);
  const long long cells = (long long)H * W;
  const size_t at = (size_t)s * max_cells;
  const uint8_t* g = grid + at;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < cells; c += (long long)gridDim.x * 256) {
    if (!g[c]) continue;
    const int r = (int)(c / W), x = (int)(c % W);
    const uint32_t me = (uint32_t)(at + c);
    if (x > 0 && g[c - 1]) uf_unite(parent, me, me - 1);
    if (r > 0) {
      const long long up = c - W;
      if (x > 0 && g[up - 1]) uf_unite(parent, me, me - (uint32_t)W - 1);
      if (g[up]) uf_unite(parent, me, me - (uint32_t)W);
      if (x + 1 < W && g[up + 1]) uf_unite(parent, me, me - (uint32_t)W + 1);
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------
// words of a packed grid: H * ceil(W / 64) <= (H W + 63 H) / 64
int64_t bit_words_for(int64_t cells) { return cells / 64 + DP_FLOOR_MAX_DIM + 1; }
bool pos_finite(double v) { return v > 0.0 && v < __builtin_inf(); }
bool kernel_size_ok(int k) { return k >= 1 && k <= DP_FLOOR_MAX_KERNEL && (k & 1); }

// grid -> grid_out through `close_iters` closings and one opening (none for open_size 1) of a stack of S
// grids.  The closing's sizes are read per slice from close_size_dev, or are close_size for every slice if
// that is NULL.  a, b: S * bit_words_for(max_cells) words each.  `cap` workgroups per slice at the most.
void morphology_launch(hipStream_t s, const uint8_t* grid, const int32_t* dims, int S, int max_cells,
                       const int32_t* close_size_dev, int close_size, int close_iters, int open_size, uint8_t* grid_out,
                       u64* a, u64* b, int cap) {
  const long long words = bit_words_for(max_cells);
  const dim3 gw(grid_for(words, cap), S), gc(grid_for(max_cells, cap), S), gk(grid_for(64 * words, cap), S);
  hipLaunchKernelGGL(pack_kernel, gk, dim3(256), 0, s, grid, dims, max_cells, words, a);
  // one dilation or erosion by a (2 rad + 1)-square: the row pass, then the column pass
  auto pass = [&](const int32_t* size_dev, int rad, int erode) {
    hipLaunchKernelGGL(morph_h_kernel, gw, dim3(256), 0, s, a, b, dims, max_cells, words, size_dev, rad, erode);
    hipLaunchKernelGGL(morph_v_kernel, gw, dim3(256), 0, s, b, a, dims, max_cells, words, size_dev, rad, erode);
  };
  for (int it = 0; it < close_iters; ++it) { pass(close_size_dev, close_size / 2, 0); pass(close_size_dev, close_size / 2, 1); }
  if (open_size > 1) { pass(nullptr, open_size / 2, 1); pass(nullptr, open_size / 2, 0); }
  hipLaunchKernelGGL(unpack_kernel, gc, dim3(256), 0, s, a, dims, max_cells, words, grid_out);
}

}  // namespace
