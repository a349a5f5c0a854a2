// Height-sliced floor plan (additive to ABI 20): the default mode of the reference's
// cleaned_pointcloud_to_floorplan.py in front of the regions -- the grids of all height slices in two passes
// over the cloud, the closing size each slice's raw grid asks for, and the morphology of all slices with those
// sizes read on the device.  The specification (rules R1-R4, C1-C2, M1-M2) is in dp_mi355x.h; this file is the
// method.  Every per-cell buffer is [S][max_cells]: slice s begins at s * max_cells, its live size is dims[s].
// A per-cell kernel is launched with the slice in blockIdx.y, so the lanes of a wave share their slice.
// fp64 with no FMA contraction where coordinates are involved.  No kernel waits on another workgroup.
// The extent rule, the raster's wave join, the packed morphology and the linking of the components are shared
// with the single floor plan and live in dp_grid2.h.
#include "dp_common.h"
#include "dp_grid2.h"

#pragma clang fp contract(off)

namespace {

constexpr int GRID_CAP = 4096;                  // workgroups of a per-point kernel at the most
constexpr int CELL_CAP = 1024;                  // workgroups per slice of a per-cell kernel at the most
#define SMAX DP_SLICE_MAX

struct SliceHdr {
  u64 mm[4];                      // keys of min / max of x, z over the slice's participants
  double lo, hi, ox, oz;          // R1 bounds; the grid's origin
  uint32_t part, dropped, occupied, err;
  uint32_t fg, roots;             // dp_slice_closing_sizes: set cells, components
  int32_t H, W;                   // (0, 0) under a status
};

// ---- raster ---------------------------------------------------------------------------------------
// R1, one thread per slice
__global__ void slice_init_kernel(SliceHdr* h, int S, double hmin, double hmax, double* __restrict__ bounds) {
  const int s = threadIdx.x;
  if (s >= S) return;
  const double step = (hmax - hmin) / (double)S;
  const double lo = hmin + (double)s * step;
  const double hi = lo + step;
  SliceHdr& q = h[s];
  q.mm[0] = q.mm[2] = ~0ull; q.mm[1] = q.mm[3] = 0;
  q.lo = lo; q.hi = hi; q.ox = q.oz = 0.0;
  q.part = q.dropped = q.occupied = q.err = q.fg = q.roots = 0;
  q.H = q.W = 0;
  bounds[3 * s] = lo; bounds[3 * s + 1] = hi; bounds[3 * s + 2] = (lo + hi) / 2.0;
}

// Pass 1.  One row per lane.  For every slice (R2: its own pair of comparisons) that has a row in the wave,
// the wave reduces the keys of those rows and one lane adds the result to the workgroup's copy in LDS; the
// workgroup then issues one set of global atomics per slice it has seen.
__global__ void __launch_bounds__(256) slice_minmax_kernel(const double* __restrict__ pts, const int32_t* n_dev, int n_max, int S,
                                                           SliceHdr* h) {
  __shared__ double slo[SMAX], shi[SMAX];
  __shared__ u64 smm[SMAX][4];
  __shared__ uint32_t scnt[SMAX];
  if ((int)threadIdx.x < S) {
    const int s = threadIdx.x;
    slo[s] = h[s].lo; shi[s] = h[s].hi;
    smm[s][0] = smm[s][2] = ~0ull; smm[s][1] = smm[s][3] = 0;
    scnt[s] = 0;
  }
  __syncthreads();
  const int n = live_n(n_dev, n_max), lane = threadIdx.x & 63;
  for (long long base = (long long)blockIdx.x * 256 + (threadIdx.x & ~63); base < n; base += (long long)gridDim.x * 256) {
    const long long i = base + lane;
    double x = 0.0, y = 0.0, z = 0.0;
    bool finite = false;
    if (i < n) {
      x = pts[3 * i]; y = pts[3 * i + 1]; z = pts[3 * i + 2];
      finite = finite3(x, y, z);
    }
    const u64 kx = okey(x), kz = okey(z);
    for (int s = 0; s < S; ++s) {
      const bool in = finite && y >= slo[s] && y < shi[s];
      const u64 m = __ballot(in);
      if (!m) continue;                                          // wave-uniform
      u64 mn[2] = {in ? kx : ~0ull, in ? kz : ~0ull}, mx[2] = {in ? kx : 0ull, in ? kz : 0ull};
      #pragma unroll
      for (int o = 32; o > 0; o >>= 1) wave_minmax(mn, mx, o);
      if (lane == 0) {
        atomicMin(&smm[s][0], mn[0]); atomicMax(&smm[s][1], mx[0]);
        atomicMin(&smm[s][2], mn[1]); atomicMax(&smm[s][3], mx[1]);
        atomicAdd(&scnt[s], (uint32_t)__popcll(m));
      }
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < S && scnt[threadIdx.x]) {
    const int s = threadIdx.x;
    atomicMin(&h[s].mm[0], smm[s][0]); atomicMax(&h[s].mm[1], smm[s][1]);
    atomicMin(&h[s].mm[2], smm[s][2]); atomicMax(&h[s].mm[3], smm[s][3]);
    atomicAdd(&h[s].part, scnt[s]);
  }
}

// R3 (rule 3 of "Occupancy floor plan") and R4, one thread per slice
__global__ void slice_setup_kernel(SliceHdr* h, int S, double res, double padding, int min_points, int max_cells,
                                   int32_t* __restrict__ dims, double* __restrict__ origin) {
  const int s = threadIdx.x;
  if (s >= S) return;
  SliceHdr& q = h[s];
  int err = 0, H = 0, W = 0;
  double ox = 0.0, oz = 0.0;
  if (q.part == 0 || (long long)q.part < (long long)min_points) {
    err = 1;
  } else {
    err = grid_extent(q.mm, padding, res, max_cells, ox, oz, H, W);
  }
  q.ox = ox; q.oz = oz; q.err = (uint32_t)err;
  q.H = dims[2 * s] = H;
  q.W = dims[2 * s + 1] = W;
  origin[2 * s] = ox; origin[2 * s + 1] = oz;
}

// the keys of pass 2 live in height_out until slice_finish_kernel turns them into heights
__global__ void __launch_bounds__(256) slice_clear_kernel(const SliceHdr* h, int max_cells, uint32_t* __restrict__ keys,
                                                          uint32_t* __restrict__ density) {
  const int s = blockIdx.y;
  const long long cells = (long long)h[s].H * h[s].W;
  const size_t at = (size_t)s * max_cells;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < cells; c += (long long)gridDim.x * 256) {
    keys[at + c] = 0;
    density[at + c] = 0;
  }
}

// Pass 2: the wave join of dp_grid2.h with the key (slice, cell).  The slices are taken one after the other,
// so two rows join only inside one slice; a row of two slices is rastered into both.
__global__ void __launch_bounds__(256) slice_raster_kernel(const double* __restrict__ pts, const int32_t* n_dev, int n_max, int S,
                                                           double res, SliceHdr* h, int max_cells, uint32_t* __restrict__ keys,
                                                           uint32_t* __restrict__ density) {
  __shared__ double slo[SMAX], shi[SMAX], sox[SMAX], soz[SMAX];
  __shared__ int sH[SMAX], sW[SMAX];
  if ((int)threadIdx.x < S) {
    const int s = threadIdx.x;
    slo[s] = h[s].lo; shi[s] = h[s].hi; sox[s] = h[s].ox; soz[s] = h[s].oz;
    sH[s] = h[s].H; sW[s] = h[s].W;
  }
  __syncthreads();
  const int n = live_n(n_dev, n_max), lane = threadIdx.x & 63;
  for (long long base = (long long)blockIdx.x * 256 + (threadIdx.x & ~63); base < n; base += (long long)gridDim.x * 256) {
    const long long i = base + lane;
    double x = 0.0, y = 0.0, z = 0.0;
    bool finite = false;
    if (i < n) {
      x = pts[3 * i]; y = pts[3 * i + 1]; z = pts[3 * i + 2];
      finite = finite3(x, y, z);
    }
    const uint32_t key = okey32((float)y);
    for (int s = 0; s < S; ++s) {
      const bool in = finite && y >= slo[s] && y < shi[s];
      const int H = sH[s], W = sW[s];
      if (!__ballot(in) || W == 0) continue;                     // wave-uniform: no row here, or a slice under a status
      bool valid = false;
      int cell = -1;
      if (in) {
        const double qx = (x - sox[s]) / res, qz = (z - soz[s]) / res;      // >= 0: the origin lies below every participant
        if (qx < (double)W && qz < (double)H) {
          cell = (int)qz * W + (int)qx;
          valid = true;
        }
      }
      const u64 out = __ballot(in && !valid);
      if (out && lane == 0) atomicAdd(&h[s].dropped, (uint32_t)__popcll(out));
      const size_t at = (size_t)s * max_cells;
      wave_join_cells(valid, cell, key, density + at, keys + at);
    }
  }
}

__global__ void __launch_bounds__(256) slice_finish_kernel(SliceHdr* h, int max_cells, const uint32_t* __restrict__ density,
                                                           float* __restrict__ height, uint8_t* __restrict__ occupied) {
  const int s = blockIdx.y;
  const long long cells = (long long)h[s].H * h[s].W;
  const size_t at = (size_t)s * max_cells;
  for (long long b = (long long)blockIdx.x * 256; b < cells; b += (long long)gridDim.x * 256) {
    const long long c = b + threadIdx.x;
    bool occ = false;
    if (c < cells) {
      occ = density[at + c] > 0;
      const uint32_t k = __float_as_uint(height[at + c]);
      height[at + c] = occ ? unkey32(k) : 0.0f;
      occupied[at + c] = occ;
    }
    wave_count(&h[s].occupied, occ);
  }
}

__global__ void slice_stats_kernel(const SliceHdr* h, int S, double* __restrict__ st) {
  const int s = threadIdx.x;
  if (s >= S) return;
  double* o = st + 8 * s;
  o[0] = (double)h[s].part; o[1] = (double)h[s].dropped; o[2] = (double)h[s].occupied;
  o[3] = (double)h[s].H; o[4] = (double)h[s].W; o[5] = (double)h[s].err;
  o[6] = o[7] = 0.0;
}

// ---- closing sizes --------------------------------------------------------------------------------
__global__ void cc_zero_kernel(SliceHdr* h, int S) {
  if ((int)threadIdx.x < S) h[threadIdx.x].fg = h[threadIdx.x].roots = 0;
}

// after the last union a set cell is a root iff it is its own parent (halving only rewrites other words)
__global__ void __launch_bounds__(256) cc_roots_kernel(const int32_t* dims, int max_cells, const uint32_t* __restrict__ parent,
                                                       SliceHdr* h) {
  const int s = blockIdx.y;
  int H, W;
  grid_dims(dims + 2 * s, max_cells, H, W);
  const long long cells = (long long)H * W;
  const size_t at = (size_t)s * max_cells;
  for (long long b = (long long)blockIdx.x * 256; b < cells; b += (long long)gridDim.x * 256) {
    const long long c = b + threadIdx.x;
    wave_count(&h[s].roots, c < cells && ld(&parent[at + c]) == (uint32_t)(at + c));
  }
}

// C2 in 64-bit integers, one thread per slice
__global__ void cc_sizes_kernel(const SliceHdr* h, int S, int32_t* __restrict__ size, long long* __restrict__ counts) {
  const int s = threadIdx.x;
  if (s >= S) return;
  const long long cells = h[s].fg, comps = h[s].roots;
  int k = 11;
  if (comps == 0 || cells < 400 * comps) k = 3;
  else if (cells < 900 * comps) k = 5;
  else if (cells < 1600 * comps) k = 7;
  else if (cells < 2500 * comps) k = 9;
  size[s] = k;
  counts[2 * s] = cells; counts[2 * s + 1] = comps;
}

// ---- workspace ------------------------------------------------------------------------------------
struct Ws {
  SliceHdr* h;
  uint32_t* parent;
  u64 *bits_a, *bits_b;
};
int64_t ws_bytes_for(int64_t S, int64_t max_cells) {
  const int64_t k = S < 0 ? 0 : (S > SMAX ? SMAX : S), n = max_cells < 0 ? 0 : max_cells;
  return al256(sizeof(SliceHdr) * SMAX) + al256(4 * k * n) + 2 * al256(8 * k * bit_words_for(n)) + 256;
}
bool ws_carve(void* ws, int64_t bytes, int64_t S, int64_t max_cells, Ws* o) {
  if (!ws || bytes < ws_bytes_for(S, max_cells) || ((uintptr_t)ws & 7)) return false;
  char* p = (char*)ws;
  o->h = (SliceHdr*)p;        p += al256(sizeof(SliceHdr) * SMAX);
  o->parent = (uint32_t*)p;   p += al256(4 * S * max_cells);
  o->bits_a = (u64*)p;        p += al256(8 * S * bit_words_for(max_cells));
  o->bits_b = (u64*)p;
  return true;
}
bool finite_h(double v) { return __builtin_fabs(v) < __builtin_inf(); }
// S in [1, DP_SLICE_MAX], and the stacked cell index below 2^31
bool layout_ok(int S, int max_cells) { return S >= 1 && S <= SMAX && max_cells >= 0 && (int64_t)S * max_cells <= 0x7fffffffll; }

}  // namespace

extern "C" int64_t dp_slices_workspace_size(int64_t num_slices, int64_t max_cells) { return ws_bytes_for(num_slices, max_cells); }

extern "C" int dp_slice_grids(const double* points, const int32_t* n_dev, int32_t n_max, double height_min, double height_max,
                              int32_t num_slices, double resolution, double padding, int32_t min_points, int32_t max_cells,
                              uint32_t* density_out, float* height_out, uint8_t* occupied_out, int32_t* dims_out,
                              double* origin_out, double* bounds_out, double* stats_out, void* workspace,
                              int64_t workspace_bytes, dp_stream_t stream) {
  if (!dims_out || !origin_out || !bounds_out || !stats_out || (n_max > 0 && !points) ||
      (max_cells > 0 && (!density_out || !height_out || !occupied_out)))
    return DP_ERR_ARG;
  if (n_max < 0 || !layout_ok(num_slices, max_cells) || min_points < 0 || !pos_finite(resolution) || !(padding >= 0.0) ||
      !(padding < __builtin_inf()) || !finite_h(height_min) || !finite_h(height_max) || !(height_max > height_min))
    return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, num_slices, max_cells, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int S = num_slices, gp = grid_for(n_max, GRID_CAP);
  const dim3 gc(grid_for(max_cells, CELL_CAP), S);
  uint32_t* keys = (uint32_t*)height_out;
  hipLaunchKernelGGL(slice_init_kernel, dim3(1), dim3(64), 0, s, w.h, S, height_min, height_max, bounds_out);
  hipLaunchKernelGGL(slice_minmax_kernel, dim3(gp), dim3(256), 0, s, points, n_dev, n_max, S, w.h);
  hipLaunchKernelGGL(slice_setup_kernel, dim3(1), dim3(64), 0, s, w.h, S, resolution, padding, min_points, max_cells, dims_out,
                     origin_out);
  hipLaunchKernelGGL(slice_clear_kernel, gc, dim3(256), 0, s, w.h, max_cells, keys, density_out);
  hipLaunchKernelGGL(slice_raster_kernel, dim3(gp), dim3(256), 0, s, points, n_dev, n_max, S, resolution, w.h, max_cells, keys,
                     density_out);
  hipLaunchKernelGGL(slice_finish_kernel, gc, dim3(256), 0, s, w.h, max_cells, density_out, height_out, occupied_out);
  hipLaunchKernelGGL(slice_stats_kernel, dim3(1), dim3(64), 0, s, w.h, S, stats_out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_slice_closing_sizes(const uint8_t* grid, const int32_t* dims, int32_t num_slices, int32_t max_cells,
                                      int32_t* close_size_out, int64_t* counts_out, void* workspace, int64_t workspace_bytes,
                                      dp_stream_t stream) {
  if (!dims || !close_size_out || !counts_out || (max_cells > 0 && !grid)) return DP_ERR_ARG;
  if (!layout_ok(num_slices, max_cells)) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, num_slices, max_cells, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int S = num_slices;
  const dim3 gc(grid_for(max_cells, CELL_CAP), S);
  hipLaunchKernelGGL(cc_zero_kernel, dim3(1), dim3(64), 0, s, w.h, S);
  hipLaunchKernelGGL(cc_init_kernel, gc, dim3(256), 0, s, grid, dims, max_cells, w.parent, &w.h->fg, (int)(sizeof(SliceHdr) / 4));
  hipLaunchKernelGGL(cc_link_kernel, gc, dim3(256), 0, s, grid, dims, max_cells, w.parent);
  hipLaunchKernelGGL(cc_roots_kernel, gc, dim3(256), 0, s, dims, max_cells, w.parent, w.h);
  hipLaunchKernelGGL(cc_sizes_kernel, dim3(1), dim3(64), 0, s, w.h, S, close_size_out, (long long*)counts_out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_slice_morphology(const uint8_t* grid, const int32_t* dims, int32_t num_slices, int32_t max_cells,
                                   const int32_t* close_size, int32_t close_iters, int32_t open_size, uint8_t* grid_out,
                                   void* workspace, int64_t workspace_bytes, dp_stream_t stream) {
  if (!dims || !close_size || (max_cells > 0 && (!grid || !grid_out))) return DP_ERR_ARG;
  if (!layout_ok(num_slices, max_cells) || close_iters < 0 || !kernel_size_ok(open_size)) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, num_slices, max_cells, &w)) return DP_ERR_ARG;
  morphology_launch((hipStream_t)stream, grid, dims, num_slices, max_cells, close_size, 1, close_iters, open_size, grid_out, w.bits_a,
                    w.bits_b, CELL_CAP);
  DP_CHECK_LAUNCH();
  return 0;
}
