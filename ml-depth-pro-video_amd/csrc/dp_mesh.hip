// Triangle mesh (additive to ABI 20): the exact k nearest other rows (dp_knn_exact), the reference's "simple"
// mesher -- a fan of triangles over each point's neighbour list (dp_mesh_fan) -- and the removal of degenerate
// and duplicated triangles (dp_mesh_clean_triangles), plus the mean neighbour distance of a list
// (dp_mesh_mean_distance).  pointcloud_to_mesh.py:397-465.  The specification is in dp_mi355x.h.  fp64, no FMA
// contraction anywhere in this file.  The grid is dp_knn_search's (cell keys, dp_sort_pairs, cell rows by
// binary search, the top-k merge): it lives in dp_grid3.h.
#include "dp_common.h"
#include "dp_grid3.h"

#pragma clang fp contract(off)

namespace {

constexpr int GRID_CAP = 4096;                  // workgroups of a per-row kernel at the most
constexpr int MAX_K = 64;                       // one kept neighbour per lane
constexpr int RING_MAX = 8;                     // rings walked cell by cell; a query that needs more reads every row

struct Hdr {
  Grid3 g;              // dp_knn_exact
  uint32_t ctr[5];
};
enum { C_FEW = 0, C_RING = 1,                                                       // dp_knn_exact
       T_INVALID = 2, T_DEGENERATE = 3, T_HEADS = 4 };                              // dp_mesh_clean_triangles

__global__ void hdr_init_kernel(Hdr* h) {
  grid3_reset(&h->g);
  for (int a = 0; a < 5; ++a) h->ctr[a] = 0;
}

// ---- exact k nearest ------------------------------------------------------------------------------
// Lane l offers the sorted position c (live: c is a candidate, never the query itself) to the running best.
// Called by all 64 lanes of the wave together.
__device__ __forceinline__ void offer(bool live, int c, const double* __restrict__ sp, const uint32_t* __restrict__ idx,
                                      double x, double y, double z, int k, int lane, u64& bk, uint32_t& br) {
  u64 ck = NO_KEY;
  uint32_t cr = ~0u;
  if (live) {
    const double dx = sp[3 * (size_t)c] - x, dy = sp[3 * (size_t)c + 1] - y, dz = sp[3 * (size_t)c + 2] - z;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    ck = (u64)__double_as_longlong(d2);
    cr = idx[c];
  }
  wave_top64_merge(live, ck, cr, k, lane, bk, br);
}

// smallest r >= 0 with d2 < (r * edge) * (r * edge), capped at cap: rule 4's distance ring
__device__ __forceinline__ int ring_of(double d2, double edge, int cap) {
  double g = __builtin_floor(__builtin_sqrt(d2) / edge) - 2.0;
  int r = g > 0.0 ? (g < (double)cap ? (int)g : cap) : 0;
  while (r < cap) {
    const double lim = (double)r * edge;
    if (d2 < lim * lim) break;
    ++r;
  }
  return r;
}

// One wave per query, in sorted (cell) order.  Ring r is the shell of cells at Chebyshev distance exactly r from
// the query's cell, as key ranges: the 8 r cell rows (x, y) on the square's rim with z in [cz - r, cz + r], and
// for the (2 r - 1)^2 rows inside it the two cells at cz - r and cz + r.  Each lane takes one range (its two
// binary searches), clipped to the grid's extent; the ranges' candidates are numbered through a prefix sum over
// the lanes and go 64 at a time to `offer`.  After ring r the walk ends if the list is full with its largest d2
// below (r * cell_edge)^2 -- the grid's edge is cell_edge * EDGE_SLACK, so no unvisited cell holds a point that
// near, the argument at EDGE_SLACK (dp_grid3.h) -- or if the cube covers the grid.  A query still open after
// RING_MAX rings starts again over every participant, in sorted order: bounded work whatever the cloud looks like.
__global__ void __launch_bounds__(256) knn_exact_kernel(const u64* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                        const double* __restrict__ sp, const int32_t* n_dev, int n_max,
                                                        double edge, int k, Hdr* h, int32_t* __restrict__ nbr,
                                                        int32_t* __restrict__ nbr_count, double* __restrict__ d2_out) {
  const int n = live_n(n_dev, n_max), lane = threadIdx.x & 63;
  const bool err = h->g.err != 0;
  const int nfin = err ? 0 : (int)(h->g.finite < (uint32_t)n ? h->g.finite : (uint32_t)n);
  const int ex = h->g.ext[0], ey = h->g.ext[1], ez = h->g.ext[2];
  uint32_t few = 0;                                       // this wave's counters (lane-uniform)
  int ring_max = 0;
  for (long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); q < n; q += (long long)gridDim.x * 4) {
    const u64 key = keys[q];
    const uint32_t row = idx[q];
    if (row >= (uint32_t)n) continue;                     // never, for a consistent sort
    u64 bk = NO_KEY;
    uint32_t br = ~0u;
    uint32_t cnt = 0;
    if (key != NO_KEY && q < nfin) {
      int cx, cy, cz;
      unpack_cell(key, cx, cy, cz);
      const double x = sp[3 * q], y = sp[3 * q + 1], z = sp[3 * q + 2];
      int cover = cx > ex - cx ? cx : ex - cx;            // the ring at which the cube covers the grid
      cover = cy > cover ? cy : cover; cover = ey - cy > cover ? ey - cy : cover;
      cover = cz > cover ? cz : cover; cover = ez - cz > cover ? ez - cz : cover;
      bool done = false;
      for (int r = 0; r <= RING_MAX && !done; ++r) {
        const int side = 8 * r, w = 2 * r - 1;
        const int nranges = r == 0 ? 1 : side + 2 * w * w;
        for (int rb = 0; rb < nranges; rb += 64) {
          const int e = rb + lane;
          int a = 0;
          uint32_t len = 0;
          if (e < nranges) {
            int dx = 0, dy = 0, zlo = cz - r, zhi = cz + r;
            if (r > 0 && e < side) {
              const int s = e / (2 * r), t = e % (2 * r);
              dx = s == 0 ? t - r : (s == 1 ? r : (s == 2 ? r - t : -r));
              dy = s == 0 ? -r : (s == 1 ? t - r : (s == 2 ? r : r - t));
            } else if (r > 0) {
              const int f = e - side, g = f >> 1;
              dx = g % w - (r - 1);
              dy = g / w - (r - 1);
              if (f & 1) zlo = zhi; else zhi = zlo;
            }
            const int rx = cx + dx, ry = cy + dy;
            zlo = zlo < 0 ? 0 : zlo;
            zhi = zhi > ez ? ez : zhi;
            if (rx >= 0 && rx <= ex && ry >= 0 && ry <= ey && zlo <= zhi) {
              int b;
              cell_row_range(keys, nfin, rx, ry, zlo, zhi, a, b);
              len = (uint32_t)(b - a);
            }
          }
          uint32_t inc = len;                              // candidates of the lanes up to this one
          #pragma unroll
          for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
          }
          const uint32_t total = __shfl(inc, 63), excl = inc - len;
          for (uint32_t base = 0; base < total; base += 64) {
            const uint32_t t = base + lane < total ? base + lane : total - 1;
            int L = 0;                                     // the first lane whose inc is above t owns candidate t
            #pragma unroll
            for (int s = 32; s > 0; s >>= 1) {
              const uint32_t v = __shfl(inc, L + s - 1);
              if (v <= t) L += s;
            }
            const int c = __shfl(a, L) + (int)(t - __shfl(excl, L));
            offer(base + lane < total && c != (int)q, c, sp, idx, x, y, z, k, lane, bk, br);
          }
        }
        const u64 tk = __shfl(bk, k - 1);
        const double lim = (double)r * edge;
        done = r >= cover || (tk != NO_KEY && __longlong_as_double((long long)tk) < lim * lim);
      }
      if (!done) {                                         // every participant, 64 at a time
        bk = NO_KEY;
        br = ~0u;
        for (int base = 0; base < nfin; base += 64) {
          const int c = base + lane;
          offer(c < nfin && c != (int)q, c, sp, idx, x, y, z, k, lane, bk, br);
        }
      }
      cnt = (uint32_t)__popcll(__ballot(lane < k && bk != NO_KEY));
      few += cnt < (uint32_t)k;
      const u64 tk = __shfl(bk, k - 1);
      const int ring = tk != NO_KEY ? ring_of(__longlong_as_double((long long)tk), edge, cover) : cover;
      ring_max = ring > ring_max ? ring : ring_max;
    }
    if (lane < k) {
      const bool listed = (uint32_t)lane < cnt && br < (uint32_t)n;
      nbr[(size_t)row * k + lane] = listed ? (int32_t)br : -1;
      if (d2_out && listed) d2_out[(size_t)row * k + lane] = __longlong_as_double((long long)bk);
    }
    if (lane == 0) nbr_count[row] = (int32_t)cnt;
  }
  if (lane == 0) {
    if (few) atomicAdd(&h->ctr[C_FEW], few);
    if (ring_max) atomicMax(&h->ctr[C_RING], (uint32_t)ring_max);
  }
}

__global__ void knn_exact_final_kernel(const Hdr* h, double* st) {
  const bool err = h->g.err != 0;
  st[0] = (double)h->g.finite;
  st[1] = (double)h->g.nonfinite;
  st[2] = err ? (double)h->g.finite : (double)h->ctr[C_FEW];          // no list at all under the flag
  st[3] = (double)h->ctr[C_RING];
  st[4] = (double)h->g.err;
  st[5] = st[6] = st[7] = 0.0;
}

// ---- mean neighbour distance ----------------------------------------------------------------------
// per row: (sqrt(d2[0]) + sqrt(d2[1]) + ...) / m in list order; 0 for a row without neighbours
__global__ void __launch_bounds__(256) row_mean_kernel(const double* __restrict__ d2, const int32_t* __restrict__ nbr_count,
                                                       const int32_t* n_dev, int n_max, int k, double* __restrict__ rm) {
  const int n = live_n(n_dev, n_max);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    int m = nbr_count[i];
    m = m < 0 ? 0 : (m > k ? k : m);
    double s = 0.0;
    for (int j = 0; j < m; ++j) s += __builtin_sqrt(d2[(size_t)i * k + j]);
    rm[i] = m ? s / (double)m : 0.0;
  }
}

// One workgroup, the order of rule 2: thread t adds rows t, t + 256, ... in turn; a wave's 64 sums meet in the
// butterfly 32, 16, ..., 1; the four waves' sums are added in wave order.
__global__ void __launch_bounds__(256) mean_reduce_kernel(const double* __restrict__ rm, const int32_t* __restrict__ nbr_count,
                                                          const int32_t* n_dev, int n_max, double* out) {
  __shared__ double ws[4];
  __shared__ double wc[4];
  const int n = live_n(n_dev, n_max);
  double s = 0.0, c = 0.0;
  for (long long i = threadIdx.x; i < n; i += 256)
    if (nbr_count[i] > 0) { s += rm[i]; c += 1.0; }
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); c += __shfl_xor(c, o); }
  if ((threadIdx.x & 63) == 0) { ws[threadIdx.x >> 6] = s; wc[threadIdx.x >> 6] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double tot = ((ws[0] + ws[1]) + ws[2]) + ws[3], rows = ((wc[0] + wc[1]) + wc[2]) + wc[3];
    out[0] = rows > 0.0 ? tot / rows : 0.0;
    out[1] = rows;
  }
}

// ---- fan ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) fan_kernel(const int32_t* __restrict__ nbr, const int32_t* __restrict__ nbr_count,
                                                  const int32_t* n_dev, int n_max, int k, int32_t* __restrict__ tri) {
  const long long slots = (long long)live_n(n_dev, n_max) * (k - 1);
  for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < slots; s += (long long)gridDim.x * 256) {
    const long long i = s / (k - 1);
    const int j = (int)(s % (k - 1));
    int m = nbr_count[i];
    m = m > k ? k : m;
    const bool on = j + 1 < m;
    tri[3 * s] = on ? (int32_t)i : -1;
    tri[3 * s + 1] = on ? nbr[i * k + j] : -1;
    tri[3 * s + 2] = on ? nbr[i * k + j + 1] : -1;
  }
}

// ---- degenerate and duplicated triangles ------------------------------------------------------------
struct Tri { uint32_t p, q, r; int state; };               // canonical form; state 0 good, 1 invalid, 2 degenerate

__device__ __forceinline__ Tri canon(const int32_t* __restrict__ tri, size_t i, int nv) {
  const int32_t a = tri[3 * i], b = tri[3 * i + 1], c = tri[3 * i + 2];
  Tri t;
  t.state = ((uint32_t)a >= (uint32_t)nv || (uint32_t)b >= (uint32_t)nv || (uint32_t)c >= (uint32_t)nv) ? 1
            : ((a == b || b == c || a == c) ? 2 : 0);
  const bool a0 = a <= b && a <= c, b0 = !a0 && b <= c;    // the smallest index first, the cycle kept
  t.p = (uint32_t)(a0 ? a : (b0 ? b : c));
  t.q = (uint32_t)(a0 ? b : (b0 ? c : a));
  t.r = (uint32_t)(a0 ? c : (b0 ? a : b));
  return t;
}

// first pass: the third index (a triangle that leaves sorts last in both passes), the input position as payload
__global__ void __launch_bounds__(256) tri_key3_kernel(const int32_t* __restrict__ tri, const int32_t* t_dev, int t_max, int nv,
                                                       Hdr* h, u64* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int n = live_n(t_dev, t_max);
  const long long padded = ((long long)n + 63) / 64 * 64;   // whole waves, for wave_count
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < padded; i += (long long)gridDim.x * 256) {
    const bool in = i < n;
    Tri t = {0, 0, 0, 0};
    if (in) {
      t = canon(tri, (size_t)i, nv);
      keys[i] = t.state ? 0xffffffffull : (u64)t.r;
      vals[i] = (uint32_t)i;
    }
    wave_count(&h->ctr[T_INVALID], in && t.state == 1);
    wave_count(&h->ctr[T_DEGENERATE], in && t.state == 2);
  }
}

// second pass: (first, second) index of the triangle now at each sorted position
__global__ void __launch_bounds__(256) tri_key12_kernel(const int32_t* __restrict__ tri, const int32_t* t_dev, int t_max, int nv,
                                                        const uint32_t* __restrict__ vals, u64* __restrict__ keys) {
  const int n = live_n(t_dev, t_max);
  for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < n; s += (long long)gridDim.x * 256) {
    const Tri t = canon(tri, row_of(vals[s], n), nv);
    keys[s] = t.state ? NO_KEY : (((u64)t.p << 32) | (u64)t.q);
  }
}

// A run of equal canonical forms is in input order (both passes are stable): its first member is kept.  The flag
// goes to the member's input position, so that the scan and the compaction run in input order.
__global__ void __launch_bounds__(256) tri_head_kernel(const int32_t* __restrict__ tri, const int32_t* t_dev, int t_max, int nv,
                                                       const uint32_t* __restrict__ vals, Hdr* h, uint8_t* __restrict__ flag) {
  const int n = live_n(t_dev, t_max);
  const long long padded = ((long long)n + 63) / 64 * 64;   // whole waves, for wave_count
  for (long long s = (long long)blockIdx.x * 256 + threadIdx.x; s < padded; s += (long long)gridDim.x * 256) {
    bool head = false;
    if (s < n) {
      const uint32_t i = row_of(vals[s], n);
      const Tri t = canon(tri, i, nv);
      head = t.state == 0;
      if (head && s > 0) {
        const Tri u = canon(tri, row_of(vals[s - 1], n), nv);
        head = u.state != 0 || u.p != t.p || u.q != t.q || u.r != t.r;
      }
      flag[i] = head;
    }
    wave_count(&h->ctr[T_HEADS], head);
  }
}

// third step of the flags' scan (dp_points.h): the kept triangles move up, in input order and as they came
__global__ void __launch_bounds__(256) tri_compact_kernel(const int32_t* __restrict__ tri, const uint8_t* __restrict__ flag,
                                                          const int32_t* t_dev, int t_max, const uint32_t* __restrict__ bc,
                                                          int32_t* __restrict__ out) {
  __shared__ uint32_t wsum[4];
  const int n = live_n(t_dev, t_max);
  const long long tile = (long long)blockIdx.x * SCAN_TILE;
  uint32_t run = bc[blockIdx.x];
  for (int r = 0; r < SCAN_ITEMS && tile + r * 256 < n; ++r) {
    const long long i = tile + r * 256 + threadIdx.x;
    const uint32_t f = i < n ? flag[i] : 0u;
    uint32_t tot = 0;
    const size_t o = run + block_excl_scan(f, wsum, &tot);
    if (f && o < (size_t)n) { out[3 * o] = tri[3 * i]; out[3 * o + 1] = tri[3 * i + 1]; out[3 * o + 2] = tri[3 * i + 2]; }
    run += tot;
  }
}

__global__ void tri_final_kernel(const Hdr* h, const int32_t* t_dev, int t_max, double* st) {
  const int n = live_n(t_dev, t_max);
  const uint32_t bad = h->ctr[T_INVALID], deg = h->ctr[T_DEGENERATE], kept = h->ctr[T_HEADS];
  st[0] = (double)n;
  st[1] = (double)bad;
  st[2] = (double)deg;
  st[3] = (double)((uint32_t)n - bad - deg - kept);
  st[4] = (double)kept;
  st[5] = st[6] = st[7] = 0.0;
}

// ---- workspace ------------------------------------------------------------------------------------
struct Ws {
  Hdr* h;
  u64* keys;
  uint32_t *vals, *bc;
  uint8_t* flag;
  double* sp;
  void* sort;
  int64_t sort_bytes;
};
int64_t clamp0(int64_t n) { return n < 0 ? 0 : n; }
// keys, payloads, flags, block counts and the sort's own space for max(n, t) elements; coordinates for n rows
int64_t ws_bytes_for(int64_t n_max, int64_t t_max) {
  const int64_t n = clamp0(n_max), m = n > clamp0(t_max) ? n : clamp0(t_max);
  return al256(sizeof(Hdr)) + al256(8 * m) + al256(4 * m) + al256(4 * (scan_blocks_for(m) + 1)) + al256(m) + al256(24 * n) +
         al256(dp_clean_workspace_size(m)) + 256;
}
// carve for m elements of the sort and n rows of coordinates; the caller's sizes must be covered by `bytes`
bool ws_carve(void* ws, int64_t bytes, int64_t n, int64_t m, Ws* o) {
  if (!ws || bytes < ws_bytes_for(n, m) || ((uintptr_t)ws & 7)) return false;
  m = n > m ? n : m;
  char* p = (char*)ws;
  o->h = (Hdr*)p;          p += al256(sizeof(Hdr));
  o->keys = (u64*)p;       p += al256(8 * m);
  o->vals = (uint32_t*)p;  p += al256(4 * m);
  o->bc = (uint32_t*)p;    p += al256(4 * (scan_blocks_for(m) + 1));
  o->flag = (uint8_t*)p;   p += al256(m);
  o->sp = (double*)p;      p += al256(24 * n);
  o->sort = p;
  o->sort_bytes = dp_clean_workspace_size(m);
  return true;
}

}  // namespace

extern "C" int64_t dp_mesh_workspace_size(int64_t n_max, int64_t t_max) { return ws_bytes_for(n_max, t_max); }

extern "C" int dp_knn_exact(const double* points, const int32_t* n_dev, int32_t n_max, int32_t k, double cell_edge,
                            int32_t* nbr_out, int32_t* nbr_count_out, double* d2_out, double* stats_out, void* workspace,
                            int64_t workspace_bytes, dp_stream_t stream) {
  if (!stats_out || (n_max > 0 && (!points || !nbr_out || !nbr_count_out))) return DP_ERR_ARG;
  if (n_max < 0 || k < 1 || k > MAX_K || !(cell_edge > 0.0) || !(cell_edge < __builtin_inf())) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, n_max, 0, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int g = grid_for(n_max, GRID_CAP);
  hipLaunchKernelGGL(hdr_init_kernel, dim3(1), dim3(1), 0, s, w.h);
  grid3_keys(s, &w.h->g, g, points, n_dev, n_max, cell_edge * EDGE_SLACK, 0.0, w.keys, w.vals);
  const int rc = dp_sort_pairs((uint64_t*)w.keys, w.vals, n_dev, n_max, 0, 64, w.sort, w.sort_bytes, (dp_stream_t)s);
  if (rc) return rc;
  hipLaunchKernelGGL(gather_points_kernel, dim3(g), dim3(256), 0, s, points, w.vals, n_dev, n_max, w.sp);
  hipLaunchKernelGGL(knn_exact_kernel, dim3(grid_for(64 * (int64_t)n_max, GRID_CAP)), dim3(256), 0, s, w.keys, w.vals, w.sp,
                     n_dev, n_max, cell_edge, k, w.h, nbr_out, nbr_count_out, d2_out);
  hipLaunchKernelGGL(knn_exact_final_kernel, dim3(1), dim3(1), 0, s, w.h, stats_out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_mesh_mean_distance(const double* d2, const int32_t* nbr_count, const int32_t* n_dev, int32_t n_max,
                                     int32_t k, double* mean_out, void* workspace, int64_t workspace_bytes,
                                     dp_stream_t stream) {
  if (!mean_out || (n_max > 0 && (!d2 || !nbr_count))) return DP_ERR_ARG;
  if (n_max < 0 || k < 1 || k > MAX_K) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, n_max, 0, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(row_mean_kernel, dim3(grid_for(n_max, GRID_CAP)), dim3(256), 0, s, d2, nbr_count, n_dev, n_max, k, w.sp);
  hipLaunchKernelGGL(mean_reduce_kernel, dim3(1), dim3(256), 0, s, w.sp, nbr_count, n_dev, n_max, mean_out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_mesh_fan(const int32_t* nbr, const int32_t* nbr_count, const int32_t* n_dev, int32_t n_max, int32_t k,
                           int32_t* tri_out, dp_stream_t stream) {
  if (n_max > 0 && k > 1 && (!nbr || !nbr_count || !tri_out)) return DP_ERR_ARG;
  if (n_max < 0 || k < 1 || k > MAX_K || (int64_t)n_max * (k - 1) >= (1ll << 31) / 3) return DP_ERR_SHAPE;
  const int64_t slots = (int64_t)n_max * (k - 1);
  if (slots == 0) return 0;                                // k = 1: no slot, nothing to write
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fan_kernel, dim3(grid_for(slots, GRID_CAP)), dim3(256), 0, s, nbr, nbr_count, n_dev, n_max, k, tri_out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_mesh_clean_triangles(const int32_t* tri_in, const int32_t* t_dev, int32_t t_max, int32_t n_vertices,
                                       int32_t* tri_out, int32_t* t_out_dev, double* stats_out, void* workspace,
                                       int64_t workspace_bytes, dp_stream_t stream) {
  if (!stats_out || !t_out_dev || (t_max > 0 && (!tri_in || !tri_out || tri_in == tri_out))) return DP_ERR_ARG;
  if (t_max < 0 || n_vertices < 0) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, 0, t_max, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int g = grid_for(t_max, GRID_CAP), nb = (int)scan_blocks_for(t_max);
  hipLaunchKernelGGL(hdr_init_kernel, dim3(1), dim3(1), 0, s, w.h);
  hipLaunchKernelGGL(tri_key3_kernel, dim3(g), dim3(256), 0, s, tri_in, t_dev, t_max, n_vertices, w.h, w.keys, w.vals);
  int rc = dp_sort_pairs((uint64_t*)w.keys, w.vals, t_dev, t_max, 0, 32, w.sort, w.sort_bytes, (dp_stream_t)s);
  if (rc) return rc;
  hipLaunchKernelGGL(tri_key12_kernel, dim3(g), dim3(256), 0, s, tri_in, t_dev, t_max, n_vertices, w.vals, w.keys);
  rc = dp_sort_pairs((uint64_t*)w.keys, w.vals, t_dev, t_max, 0, 64, w.sort, w.sort_bytes, (dp_stream_t)s);
  if (rc) return rc;
  hipLaunchKernelGGL(tri_head_kernel, dim3(g), dim3(256), 0, s, tri_in, t_dev, t_max, n_vertices, w.vals, w.h, w.flag);
  if (nb) hipLaunchKernelGGL(scan_count_kernel, dim3(nb), dim3(256), 0, s, w.flag, t_dev, t_max, w.bc);
  hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(256), 0, s, w.bc, nb, (uint32_t*)t_out_dev);   // the same bits
  if (nb) hipLaunchKernelGGL(tri_compact_kernel, dim3(nb), dim3(256), 0, s, tri_in, w.flag, t_dev, t_max, w.bc, tri_out);
  hipLaunchKernelGGL(tri_final_kernel, dim3(1), dim3(1), 0, s, w.h, t_dev, t_max, stats_out);
  DP_CHECK_LAUNCH();
  return 0;
}
