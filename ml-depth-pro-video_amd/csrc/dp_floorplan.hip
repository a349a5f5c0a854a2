// Occupancy floor plan (ABI 20): the top-down raster of the levelled cloud, binary morphology with OpenCV's
// border rule, 8-connected regions with their table, and the picture -- everything of the reference's
// cleaned_pointcloud_to_floorplan.py in front of the contour tracing.  The specification is in dp_mi355x.h.
// fp64 with no FMA contraction where coordinates are involved.  The grid's size is only known on the device
// (dims), so every kernel is launched for the caller's capacity and strides over the cells that exist.
// The extent rule, the raster's wave join, the packed morphology and the linking of the regions are shared with
// the height slices and live in dp_grid2.h, where this grid is the stack of one slice.
#include "dp_common.h"
#include "dp_grid2.h"

#pragma clang fp contract(off)

namespace {

constexpr int GRID_CAP = 4096;                  // workgroups of a per-point or per-cell kernel at the most
constexpr int MAX_DIM = DP_FLOOR_MAX_DIM;
constexpr int COLS = DP_FLOOR_COLUMNS;
constexpr int ACC = 12;                         // 64-bit accumulators per region (A_* below)
enum { A_COUNT = 0, A_SX, A_SZ, A_POINTS, A_OCC, A_SUMH, A_X0, A_Z0, A_X1, A_Z1, A_MAXH };

struct Hdr {
  u64 mm[4];            // keys of min / max of x, z over the participants
  uint32_t ctr[8];
  double par[4];        // min_x, min_z, resolution
  int32_t dim[2];       // H, W of the raster call (0, 0 under an error)
  int32_t ncells;       // H * W of the regions call (the scan's live count)
  int32_t pad;
};
enum { C_PART = 0, C_NONFINITE, C_BELOW, C_DROPPED, C_OCCUPIED, C_ERR, C_FG };

// ---- raster ---------------------------------------------------------------------------------------
__global__ void hdr_init_kernel(Hdr* h) {
  for (int a = 0; a < 2; ++a) { h->mm[2 * a] = ~0ull; h->mm[2 * a + 1] = 0; }
  for (int a = 0; a < 8; ++a) h->ctr[a] = 0;
  for (int a = 0; a < 4; ++a) h->par[a] = 0.0;
  h->dim[0] = h->dim[1] = 0;
  h->ncells = 0;
}

__device__ __forceinline__ bool takes_part(double x, double y, double z, double thr, bool& finite) {
  finite = finite3(x, y, z);
  return finite && !(y < thr);                    // a NaN threshold takes every finite row
}

__global__ void __launch_bounds__(256) minmax_xz_kernel(const double* __restrict__ pts, const int32_t* n_dev, int n_max,
                                                        double thr, Hdr* h) {
  const int n = live_n(n_dev, n_max);
  u64 mn[2] = {~0ull, ~0ull}, mx[2] = {0, 0};
  uint32_t bad = 0, low = 0, good = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    bool finite;
    if (!takes_part(x, y, z, thr, finite)) { bad += !finite; low += finite; continue; }
    ++good;
    const u64 k[2] = {okey(x), okey(z)};
    #pragma unroll
    for (int a = 0; a < 2; ++a) { mn[a] = k[a] < mn[a] ? k[a] : mn[a]; mx[a] = k[a] > mx[a] ? k[a] : mx[a]; }
  }
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    wave_minmax(mn, mx, o);
    bad += __shfl_xor(bad, o); low += __shfl_xor(low, o); good += __shfl_xor(good, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (good) {
      flush_minmax(h->mm, mn, mx);
      atomicAdd(&h->ctr[C_PART], good);
    }
    if (bad) atomicAdd(&h->ctr[C_NONFINITE], bad);
    if (low) atomicAdd(&h->ctr[C_BELOW], low);
  }
}

__global__ void grid_setup_kernel(Hdr* h, double res, double padding, int max_cells, int32_t* dims, double* origin) {
  int err = 0, H = 0, W = 0;
  double ox = 0.0, oz = 0.0;
  if (!h->ctr[C_PART]) {
    err = 1;
  } else {
    err = grid_extent(h->mm, padding, res, max_cells, ox, oz, H, W);
  }
  h->par[0] = ox; h->par[1] = oz; h->par[2] = res;
  h->dim[0] = dims[0] = H;
  h->dim[1] = dims[1] = W;
  h->ctr[C_ERR] = (uint32_t)err;
  origin[0] = ox; origin[1] = oz;
}

__global__ void __launch_bounds__(256) grid_clear_kernel(const Hdr* h, u64* __restrict__ keys, uint32_t* __restrict__ density) {
  const long long cells = (long long)h->dim[0] * h->dim[1];
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < cells; c += (long long)gridDim.x * 256) {
    keys[c] = 0;
    density[c] = 0;
  }
}

// One row per lane; the wave joins the rows of one cell before it touches the cell (dp_grid2.h).
__global__ void __launch_bounds__(256) raster_kernel(const double* __restrict__ pts, const int32_t* n_dev, int n_max, double thr,
                                                     Hdr* h, u64* __restrict__ keys, uint32_t* __restrict__ density) {
  const int n = live_n(n_dev, n_max), lane = threadIdx.x & 63;
  const int H = h->dim[0], W = h->dim[1];
  if (h->ctr[C_ERR]) return;
  const double ox = h->par[0], oz = h->par[1], res = h->par[2];
  uint32_t dropped = 0;
  for (long long base = ((long long)blockIdx.x * 256 + (threadIdx.x & ~63)); base < n; base += (long long)gridDim.x * 256) {
    const long long i = base + lane;
    bool valid = false;
    int cell = -1;
    u64 key = 0;
    if (i < n) {
      const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
      bool finite;
      if (takes_part(x, y, z, thr, finite)) {
        const double qx = (x - ox) / res, qz = (z - oz) / res;        // >= 0: ox, oz lie at or below every participant
        if (qx < (double)W && qz < (double)H) {
          cell = (int)qz * W + (int)qx;
          key = ((u64)okey32((float)y) << 32) | (u64)(~(uint32_t)i);
          valid = true;
        } else {
          ++dropped;
        }
      }
    }
    wave_join_cells(valid, cell, key, density, keys);
  }
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) dropped += __shfl_xor(dropped, o);
  if (lane == 0 && dropped) atomicAdd(&h->ctr[C_DROPPED], dropped);
}

__global__ void __launch_bounds__(256) grid_finish_kernel(Hdr* h, const u64* __restrict__ keys, const uint32_t* __restrict__ density,
                                                          const uint8_t* __restrict__ colors, int n_max, float* __restrict__ height,
                                                          uint8_t* __restrict__ color, uint8_t* __restrict__ occupied) {
  const long long cells = (long long)h->dim[0] * h->dim[1];
  for (long long b = (long long)blockIdx.x * 256; b < cells; b += (long long)gridDim.x * 256) {
    const long long c = b + threadIdx.x;
    bool occ = false;
    if (c < cells) {
      const u64 k = keys[c];
      occ = density[c] > 0;
      height[c] = occ ? unkey32((uint32_t)(k >> 32)) : 0.0f;
      occupied[c] = occ;
      if (color && occ) {
        const size_t row = row_of(~(uint32_t)k, n_max);
        color[3 * c] = colors[3 * row]; color[3 * c + 1] = colors[3 * row + 1]; color[3 * c + 2] = colors[3 * row + 2];
      }
    }
    wave_count(&h->ctr[C_OCCUPIED], occ);
  }
}

__global__ void grid_stats_kernel(const Hdr* h, double* st) {
  st[0] = (double)h->ctr[C_PART];
  st[1] = (double)h->ctr[C_NONFINITE];
  st[2] = (double)h->ctr[C_BELOW];
  st[3] = (double)h->ctr[C_DROPPED];
  st[4] = (double)h->ctr[C_OCCUPIED];
  st[5] = (double)h->dim[0];
  st[6] = (double)h->dim[1];
  st[7] = (double)h->ctr[C_ERR];
}

// ---- regions --------------------------------------------------------------------------------------
// After the last union of dp_grid2.h's linking: every cell points at its root (the region's first cell), and the
// roots are flagged.  It leaves H * W in the header, where the scan behind it reads its live count.
__global__ void __launch_bounds__(256) uf_flatten_kernel(Hdr* h, const int32_t* dims, int max_cells, uint32_t* __restrict__ parent,
                                                         uint8_t* __restrict__ flag) {
  int H, W;
  grid_dims(dims, max_cells, H, W);
  const long long cells = (long long)H * W;
  if (blockIdx.x == 0 && threadIdx.x == 0) h->ncells = (int32_t)cells;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < cells; c += (long long)gridDim.x * 256) {
    uint8_t f = 0;
    if (ld(&parent[c]) != NO_CELL) {
      const uint32_t r = uf_find(parent, (uint32_t)c);
      if (r != (uint32_t)c) atomicMin(&parent[c], r);
      else f = 1;
    }
    flag[c] = f;
  }
}

// Third step of the root flags' scan (dp_points.h): a root's number is 1 + the roots before it.
__global__ void __launch_bounds__(256) root_number_kernel(const uint8_t* __restrict__ flag, const Hdr* h, int max_cells,
                                                          const uint32_t* __restrict__ bc, int32_t* __restrict__ num) {
  __shared__ uint32_t wsum[4];
  const int n = live_n(&h->ncells, max_cells);
  const long long tile = (long long)blockIdx.x * SCAN_TILE;
  uint32_t run = bc[blockIdx.x];
  for (int r = 0; r < SCAN_ITEMS && tile + r * 256 < n; ++r) {
    const long long t = tile + r * 256 + threadIdx.x;
    const uint32_t f = t < n ? flag[t] : 0u;
    uint32_t tot = 0;
    const uint32_t excl = run + block_excl_scan(f, wsum, &tot);
    if (f) num[t] = (int32_t)(excl + 1);
    run += tot;
  }
}

__global__ void acc_init_kernel(u64* __restrict__ acc, int max_regions) {
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < (long long)max_regions * ACC; t += (long long)gridDim.x * 256) {
    const int a = (int)(t % ACC);
    acc[t] = (a == A_X0 || a == A_Z0) ? ~0ull : 0ull;
  }
}

// labels (in place over the parents: a thread reads and writes its own cell's word only) and the regions'
// accumulators, one atomic per column and cell
__global__ void __launch_bounds__(256) label_kernel(const int32_t* dims, int max_cells, int32_t* __restrict__ labels,
                                                    const int32_t* __restrict__ num, const uint32_t* __restrict__ density,
                                                    const float* __restrict__ height, int max_regions, u64* __restrict__ acc) {
  int H, W;
  grid_dims(dims, max_cells, H, W);
  const long long cells = (long long)H * W;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < cells; c += (long long)gridDim.x * 256) {
    const uint32_t root = ((const uint32_t*)labels)[c];
    if (root == NO_CELL || root >= (uint32_t)cells) { labels[c] = 0; continue; }
    const int32_t l = num[root];
    labels[c] = l;
    if (l < 1 || l > max_regions) continue;
    u64* a = acc + (size_t)(l - 1) * ACC;
    const u64 x = (u64)(c % W), z = (u64)(c / W);
    atomicAdd(&a[A_COUNT], 1ull);
    atomicAdd(&a[A_SX], x);
    atomicAdd(&a[A_SZ], z);
    atomicMin(&a[A_X0], x); atomicMax(&a[A_X1], x);
    atomicMin(&a[A_Z0], z); atomicMax(&a[A_Z1], z);
    const uint32_t d = density[c];
    if (d) {
      const float hc = height[c];
      atomicAdd(&a[A_POINTS], (u64)d);
      atomicAdd(&a[A_OCC], 1ull);
      atomicAdd((double*)&a[A_SUMH], (double)hc);
      atomicMax(&a[A_MAXH], (u64)okey32(hc));
    }
  }
}

__global__ void __launch_bounds__(256) table_kernel(const int32_t* n_regions, int max_regions, const u64* __restrict__ acc,
                                                    const double* origin, double res, double* __restrict__ table) {
  const int rows = table_rows(n_regions, max_regions);
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < rows; t += (long long)gridDim.x * 256) {
    const u64* a = acc + (size_t)t * ACC;
    double* row = table + (size_t)t * COLS;
    const double cnt = (double)a[A_COUNT];
    const double cx = (double)a[A_SX] / cnt, cz = (double)a[A_SZ] / cnt;
    row[0] = cnt;
    row[1] = cnt * (res * res);
    row[2] = (double)a[A_X0]; row[3] = (double)a[A_Z0]; row[4] = (double)a[A_X1]; row[5] = (double)a[A_Z1];
    row[6] = cx; row[7] = cz;
    row[8] = origin[0] + (cx + 0.5) * res;
    row[9] = origin[1] + (cz + 0.5) * res;
    row[10] = (double)a[A_POINTS];
    row[11] = a[A_OCC] ? (double)unkey32((uint32_t)a[A_MAXH]) : 0.0;
    row[12] = a[A_OCC] ? __longlong_as_double((long long)a[A_SUMH]) / (double)a[A_OCC] : 0.0;
  }
}

__global__ void regions_stats_kernel(const Hdr* h, const int32_t* dims, int max_cells, const int32_t* n_regions, int max_regions,
                                     double* st) {
  int H, W;
  grid_dims(dims, max_cells, H, W);
  const int n = *n_regions;
  st[0] = (double)h->ctr[C_FG];
  st[1] = (double)n;
  st[2] = (double)table_rows(n_regions, max_regions);
  st[3] = n > max_regions ? 1.0 : 0.0;
  st[4] = (double)H;
  st[5] = (double)W;
  st[6] = st[7] = 0.0;
}

// ---- picture --------------------------------------------------------------------------------------
__device__ __forceinline__ uint8_t sat_u8(double v) { return (uint8_t)(v < 0.0 ? 0 : (v > 255.0 ? 255 : (int)v)); }

__global__ void __launch_bounds__(256) image_kernel(const int32_t* __restrict__ labels, const int32_t* dims, int max_cells,
                                                    const double* __restrict__ table, const int32_t* n_regions, int max_regions,
                                                    double min_area, double max_height, int by_height, int bar_len,
                                                    uint8_t* __restrict__ image) {
  int H, W;
  grid_dims(dims, max_cells, H, W);
  const long long cells = (long long)H * W;
  const int rows = table_rows(n_regions, max_regions);
  // the reference's 1 m scale bar (its non-fast sizes: 20 cells high, 50 from the lower right corner)
  const int bx = min(W - 50 - bar_len, W - 10), bz = min(H - 50, H - 10);
  const bool bar = bx > 0 && bz > 0 && bz < H && bx + bar_len < W;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < cells; c += (long long)gridDim.x * 256) {
    const int z = (int)(c / W), x = (int)(c % W);
    const int32_t l = labels[c];
    uint8_t r = 255, g = 255, b = 255;
    if (l >= 1 && l <= rows && table[(size_t)(l - 1) * COLS + 1] >= min_area) {
      const bool edge = x == 0 || x == W - 1 || z == 0 || z == H - 1 || labels[c - 1] != l || labels[c + 1] != l ||
                        labels[c - W] != l || labels[c + W] != l;
      if (edge) {
        r = g = b = 0;
      } else if (!by_height) {
        r = g = b = 180;
      } else {
        const double q = table[(size_t)(l - 1) * COLS + 12] / max_height;
        const double hh = q < 1.0 ? q : 1.0;
        r = sat_u8(255.0 * hh);
        g = sat_u8(255.0 * (1.0 - __builtin_fabs(2.0 * hh - 1.0)));
        b = sat_u8(255.0 * (1.0 - hh));
      }
    }
    if (bar && z >= bz && z < bz + 20 && x >= bx && x < bx + bar_len) r = g = b = 0;
    image[3 * c] = r; image[3 * c + 1] = g; image[3 * c + 2] = b;
  }
}

// ---- workspace ------------------------------------------------------------------------------------
struct Ws {
  Hdr* h;
  u64 *keys, *bits_a, *bits_b, *acc;
  int32_t* num;
  uint8_t* flag;
  uint32_t* bc;
};
int64_t ws_bytes_for(int64_t max_cells, int64_t max_regions) {
  const int64_t n = max_cells < 0 ? 0 : max_cells, k = max_regions < 0 ? 0 : max_regions;
  return al256(sizeof(Hdr)) + al256(8 * n) + 2 * al256(8 * bit_words_for(n)) + al256(4 * n) + al256(n) +
         al256(4 * (scan_blocks_for(n) + 1)) + al256(8 * ACC * k) + 256;
}
bool ws_carve(void* ws, int64_t bytes, int64_t max_cells, int64_t max_regions, Ws* o) {
  if (!ws || bytes < ws_bytes_for(max_cells, max_regions) || ((uintptr_t)ws & 7)) return false;
  const int64_t n = max_cells;
  char* p = (char*)ws;
  o->h = (Hdr*)p;            p += al256(sizeof(Hdr));
  o->keys = (u64*)p;         p += al256(8 * n);
  o->bits_a = (u64*)p;       p += al256(8 * bit_words_for(n));
  o->bits_b = (u64*)p;       p += al256(8 * bit_words_for(n));
  o->num = (int32_t*)p;      p += al256(4 * n);
  o->flag = (uint8_t*)p;     p += al256(n);
  o->bc = (uint32_t*)p;      p += al256(4 * (scan_blocks_for(n) + 1));
  o->acc = (u64*)p;
  return true;
}

}  // namespace

extern "C" int64_t dp_floorplan_workspace_size(int64_t max_cells, int64_t max_regions) { return ws_bytes_for(max_cells, max_regions); }

extern "C" int dp_occupancy_grid(const double* points, const uint8_t* colors, const int32_t* n_dev, int32_t n_max,
                                 double height_threshold, double resolution, double padding, int32_t max_cells,
                                 uint32_t* density_out, float* height_out, uint8_t* color_out, uint8_t* occupied_out,
                                 int32_t* dims_out, double* origin_out, double* stats_out, void* workspace,
                                 int64_t workspace_bytes, dp_stream_t stream) {
  if (!dims_out || !origin_out || !stats_out || (n_max > 0 && !points) || (colors && !color_out) ||
      (max_cells > 0 && (!density_out || !height_out || !occupied_out)))
    return DP_ERR_ARG;
  if (n_max < 0 || max_cells < 0 || !pos_finite(resolution) || !(padding >= 0.0) || !(padding < __builtin_inf()) ||
      __builtin_fabs(height_threshold) == __builtin_inf())
    return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, max_cells, 0, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int gp = grid_for(n_max, GRID_CAP), gc = grid_for(max_cells, GRID_CAP);
  hipLaunchKernelGGL(hdr_init_kernel, dim3(1), dim3(1), 0, s, w.h);
  hipLaunchKernelGGL(minmax_xz_kernel, dim3(gp), dim3(256), 0, s, points, n_dev, n_max, height_threshold, w.h);
  hipLaunchKernelGGL(grid_setup_kernel, dim3(1), dim3(1), 0, s, w.h, resolution, padding, max_cells, dims_out, origin_out);
  hipLaunchKernelGGL(grid_clear_kernel, dim3(gc), dim3(256), 0, s, w.h, w.keys, density_out);
  hipLaunchKernelGGL(raster_kernel, dim3(gp), dim3(256), 0, s, points, n_dev, n_max, height_threshold, w.h, w.keys, density_out);
  hipLaunchKernelGGL(grid_finish_kernel, dim3(gc), dim3(256), 0, s, w.h, w.keys, density_out, colors, n_max, height_out,
                     colors ? color_out : nullptr, occupied_out);
  hipLaunchKernelGGL(grid_stats_kernel, dim3(1), dim3(1), 0, s, w.h, stats_out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_grid_morphology(const uint8_t* grid, const int32_t* dims, int32_t max_cells, int32_t close_size,
                                  int32_t close_iters, int32_t open_size, uint8_t* grid_out, void* workspace,
                                  int64_t workspace_bytes, dp_stream_t stream) {
  if (!dims || (max_cells > 0 && (!grid || !grid_out))) return DP_ERR_ARG;
  if (max_cells < 0 || close_iters < 0 || !kernel_size_ok(close_size) || !kernel_size_ok(open_size)) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, max_cells, 0, &w)) return DP_ERR_ARG;
  // a closing by one cell changes nothing: no launch for it
  morphology_launch((hipStream_t)stream, grid, dims, 1, max_cells, nullptr, close_size, close_size > 1 ? close_iters : 0, open_size,
                    grid_out, w.bits_a, w.bits_b, GRID_CAP);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_grid_regions(const uint8_t* grid, const uint32_t* density, const float* height, const int32_t* dims,
                               const double* origin, int32_t max_cells, double resolution, int32_t max_regions,
                               int32_t* labels_out, int32_t* n_regions_dev, double* table_out, double* stats_out,
                               void* workspace, int64_t workspace_bytes, dp_stream_t stream) {
  if (!dims || !origin || !n_regions_dev || !stats_out || (max_regions > 0 && !table_out) ||
      (max_cells > 0 && (!grid || !density || !height || !labels_out)))
    return DP_ERR_ARG;
  if (max_cells < 0 || max_regions < 0 || !pos_finite(resolution)) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, max_cells, max_regions, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int gc = grid_for(max_cells, GRID_CAP), nb = (int)scan_blocks_for(max_cells);
  uint32_t* parent = (uint32_t*)labels_out;
  hipLaunchKernelGGL(hdr_init_kernel, dim3(1), dim3(1), 0, s, w.h);
  hipLaunchKernelGGL(cc_init_kernel, dim3(gc), dim3(256), 0, s, grid, dims, max_cells, parent, &w.h->ctr[C_FG], 0);
  hipLaunchKernelGGL(cc_link_kernel, dim3(gc), dim3(256), 0, s, grid, dims, max_cells, parent);
  hipLaunchKernelGGL(uf_flatten_kernel, dim3(gc), dim3(256), 0, s, w.h, dims, max_cells, parent, w.flag);
  if (nb) hipLaunchKernelGGL(scan_count_kernel, dim3(nb), dim3(256), 0, s, w.flag, &w.h->ncells, max_cells, w.bc);
  hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(256), 0, s, w.bc, nb, (uint32_t*)n_regions_dev);   // the same bits
  if (nb) hipLaunchKernelGGL(root_number_kernel, dim3(nb), dim3(256), 0, s, w.flag, w.h, max_cells, w.bc, w.num);
  hipLaunchKernelGGL(acc_init_kernel, dim3(grid_for((int64_t)max_regions * ACC, GRID_CAP)), dim3(256), 0, s, w.acc, max_regions);
  hipLaunchKernelGGL(label_kernel, dim3(gc), dim3(256), 0, s, dims, max_cells, labels_out, w.num, density, height,
                     max_regions, w.acc);
  hipLaunchKernelGGL(table_kernel, dim3(grid_for(max_regions, GRID_CAP)), dim3(256), 0, s, n_regions_dev, max_regions, w.acc,
                     origin, resolution, table_out);
  hipLaunchKernelGGL(regions_stats_kernel, dim3(1), dim3(1), 0, s, w.h, dims, max_cells, n_regions_dev, max_regions, stats_out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_floorplan_image(const int32_t* labels, const int32_t* dims, int32_t max_cells, const double* table,
                                  const int32_t* n_regions_dev, int32_t max_regions, double resolution, double min_area,
                                  double max_height, int32_t color_by_height, uint8_t* image_out, dp_stream_t stream) {
  if (!dims || !n_regions_dev || (max_regions > 0 && !table) || (max_cells > 0 && (!labels || !image_out))) return DP_ERR_ARG;
  if (max_cells < 0 || max_regions < 0 || !pos_finite(resolution) || !pos_finite(max_height) || !(min_area >= 0.0) ||
      !(min_area < __builtin_inf()))
    return DP_ERR_SHAPE;
  const double len = 1.0 / resolution;
  const int bar_len = len < (double)(2 * MAX_DIM) ? (int)len : 2 * MAX_DIM;        // longer than any grid: no bar
  hipLaunchKernelGGL(image_kernel, dim3(grid_for(max_cells, GRID_CAP)), dim3(256), 0, (hipStream_t)stream, labels, dims,
                     max_cells, table, n_regions_dev, max_regions, min_area, max_height, color_by_height, bar_len, image_out);
  DP_CHECK_LAUNCH();
  return 0;
}
