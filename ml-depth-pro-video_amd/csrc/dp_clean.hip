// Cleaned point clouds (ABI 16): a stable LSD radix sort of (u64 key, u32 payload) pairs, and on top
// of it stray-point removal (pointcloud_cleaner.py:142-207), shadow-column removal (:209-309) and
// order-preserving compaction.  fp64 as numpy computes it; no FMA contraction anywhere in this file,
// so each product and sum is rounded on its own.  Three kernels per sort pass (histogram, table
// scan, scatter); no kernel waits on another workgroup's progress.
#include "dp_common.h"
#include "dp_grid3.h"

#pragma clang fp contract(off)

namespace {

constexpr int GRID_CAP = 4096;                  // workgroups of a per-point kernel at the most
constexpr int SORT_ITEMS = 16;                  // rounds of 256 consecutive elements per workgroup
constexpr int SORT_TILE = 256 * SORT_ITEMS;     // elements of one workgroup (sort)
constexpr uint32_t NO_COL = 0xffffffffu;        // shadow stage: "in no column"

struct Hdr {
  Grid3 g;              // the stray stage's grid (dp_grid3.h); the shadow stage reads its extremes and finite count
  uint32_t ctr[8];
  double par[4];        // shadow stage: first x edge, first z edge, cell size; [3] is padding for tot
  uint32_t tot[8][256]; // per sort pass: elements per digit (all workgroups)
};
// run_sort clears tot with a memset; 8 bytes off a 16-byte boundary every sort took about 4 us longer
// (profiles/grid3_shared/speed.md)
static_assert(offsetof(Hdr, tot) % 16 == 0, "keep tot on a 16-byte boundary");
enum { C_KEPT = 0, C_SHADOW_ERR = 1, C_OCC = 2, C_TESTED = 3, C_REMCOL = 4, C_REMPTS = 5, C_LENX = 6, C_LENZ = 7 };

__device__ __forceinline__ u64 lanes_below() { return (1ull << (threadIdx.x & 63)) - 1ull; }

// Lanes of the wave that hold the same 8-bit digit as this one (64-lane ballots, one per bit);
// lanes with valid == false are in no group.
__device__ __forceinline__ u64 match_digit(bool valid, uint32_t d) {
  u64 peers = __ballot(valid);
  #pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (d >> b) & 1u;
    const u64 bb = __ballot(valid && bit);
    peers &= bit ? bb : ~bb;
  }
  return peers;
}

// ---- the sort -----------------------------------------------------------------------------------
// One pass = digit (key >> lo) & mask.  Workgroup b owns elements [b * SORT_TILE, (b + 1) * SORT_TILE)
// in rounds of 256 consecutive elements; order inside the tile is (round, wave, lane) = index order.
__global__ void __launch_bounds__(256) sort_hist_kernel(const u64* __restrict__ keys, const int32_t* n_dev, int n_max,
                                                        int lo, uint32_t mask, uint32_t* __restrict__ table,
                                                        int nblocks, uint32_t* tot) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int n = live_n(n_dev, n_max);
  const long long base = (long long)blockIdx.x * SORT_TILE;
  for (int r = 0; r < SORT_ITEMS && base + r * 256 < n; ++r) {
    const long long i = base + r * 256 + threadIdx.x;
    const bool valid = i < n;
    const uint32_t d = valid ? (uint32_t)(keys[i] >> lo) & mask : 0u;
    const u64 peers = match_digit(valid, d);
    if (valid && !(peers & lanes_below())) atomicAdd(&h[d], (uint32_t)__popcll(peers));   // one atomic per group
  }
  __syncthreads();
  const uint32_t c = h[threadIdx.x];
  table[(size_t)threadIdx.x * nblocks + blockIdx.x] = c;
  if (c) atomicAdd(&tot[threadIdx.x], c);
}

// Workgroup d turns row d of the [256][nblocks] table into global start offsets: the elements of
// all smaller digits, plus the elements of digit d in the workgroups before.
__global__ void __launch_bounds__(256) sort_scan_kernel(uint32_t* __restrict__ table, int nblocks, const uint32_t* tot) {
  __shared__ uint32_t wsum[4];
  const int d = blockIdx.x;
  uint32_t dbase = 0;
  block_excl_scan((int)threadIdx.x < d ? tot[threadIdx.x] : 0u, wsum, &dbase);
  uint32_t* row = table + (size_t)d * nblocks;
  const int per = (nblocks + 255) / 256;
  const long long b0 = (long long)threadIdx.x * per;
  const long long b1 = b0 + per < nblocks ? b0 + per : nblocks;
  uint32_t s = 0;
  for (long long b = b0; b < b1; ++b) s += row[b];
  uint32_t run = dbase + block_excl_scan(s, wsum);
  for (long long b = b0; b < b1; ++b) {
    const uint32_t t = row[b];
    row[b] = run;
    run += t;
  }
}

// In-tile rank of an element = elements of the same digit in earlier rounds (base[] advances per
// round) + in earlier waves of this round (wc[][]) + in lower lanes of its wave (ballot groups):
// index order, so the pass is stable.
__global__ void __launch_bounds__(256) sort_scatter_kernel(const u64* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                           u64* __restrict__ keys_out, uint32_t* __restrict__ vals_out,
                                                           const int32_t* n_dev, int n_max, int lo, uint32_t mask,
                                                           const uint32_t* __restrict__ table, int nblocks) {
  __shared__ uint32_t base[256];
  __shared__ uint32_t wc[4][256];
  const int w = threadIdx.x >> 6;
  base[threadIdx.x] = table[(size_t)threadIdx.x * nblocks + blockIdx.x];
  for (int k = 0; k < 4; ++k) wc[k][threadIdx.x] = 0;
  __syncthreads();
  const int n = live_n(n_dev, n_max);
  const long long tile = (long long)blockIdx.x * SORT_TILE;
  for (int r = 0; r < SORT_ITEMS && tile + r * 256 < n; ++r) {
    const long long i = tile + r * 256 + threadIdx.x;
    const bool valid = i < n;
    const u64 key = valid ? keys[i] : 0ull;
    const uint32_t d = (uint32_t)(key >> lo) & mask;
    const u64 peers = match_digit(valid, d);
    const uint32_t rank = (uint32_t)__popcll(peers & lanes_below());
    if (valid && rank == 0) wc[w][d] = (uint32_t)__popcll(peers);
    __syncthreads();
    if (valid) {
      uint32_t off = base[d] + rank;
      for (int k = 0; k < w; ++k) off += wc[k][d];
      if (off < (uint32_t)n) {              // always true for a consistent table; never write past the live range
        keys_out[off] = key;
        vals_out[off] = vals[i];
      }
    }
    __syncthreads();
    base[threadIdx.x] += wc[0][threadIdx.x] + wc[1][threadIdx.x] + wc[2][threadIdx.x] + wc[3][threadIdx.x];
    for (int k = 0; k < 4; ++k) wc[k][threadIdx.x] = 0;
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) copy_pairs_kernel(const u64* __restrict__ k, const uint32_t* __restrict__ v,
                                                         u64* __restrict__ ko, uint32_t* __restrict__ vo,
                                                         const int32_t* n_dev, int n_max) {
  const int n = live_n(n_dev, n_max);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    ko[i] = k[i];
    vo[i] = v[i];
  }
}

int sort_blocks(int64_t n_max) { return (int)((n_max + SORT_TILE - 1) / SORT_TILE); }
int sort_passes(int bit_lo, int bit_hi) {
  int p = 0;
  for (int d = 0; d < 8; ++d) p += (8 * d < bit_hi && 8 * d + 8 > bit_lo);
  return p;
}

// Sorts (ka, va) by key bits [bit_lo, bit_hi), ping-ponging with (kb, vb).  Returns true if the
// result is in (kb, vb): an odd number of passes, which depends on bit_lo / bit_hi alone.
bool run_sort(hipStream_t s, Hdr* h, u64* ka, uint32_t* va, u64* kb, uint32_t* vb, uint32_t* table,
              const int32_t* n_dev, int n_max, int bit_lo, int bit_hi) {
  const int nb = sort_blocks(n_max);
  bool in_b = false;
  if (nb == 0 || sort_passes(bit_lo, bit_hi) == 0) return false;
  (void)hipMemsetAsync(h->tot, 0, sizeof(h->tot), s);
  for (int d = 0; d < 8; ++d) {
    const int lo = 8 * d > bit_lo ? 8 * d : bit_lo, hi = 8 * d + 8 < bit_hi ? 8 * d + 8 : bit_hi;
    if (lo >= hi) continue;
    const uint32_t mask = (1u << (hi - lo)) - 1u;
    const u64* ki = in_b ? kb : ka;
    const uint32_t* vi = in_b ? vb : va;
    hipLaunchKernelGGL(sort_hist_kernel, dim3(nb), dim3(256), 0, s, ki, n_dev, n_max, lo, mask, table, nb, h->tot[d]);
    hipLaunchKernelGGL(sort_scan_kernel, dim3(256), dim3(256), 0, s, table, nb, h->tot[d]);
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(nb), dim3(256), 0, s, ki, vi, in_b ? ka : kb, in_b ? va : vb, n_dev,
                       n_max, lo, mask, table, nb);
    in_b = !in_b;
  }
  return in_b;
}

// ---- workspace ----------------------------------------------------------------------------------
struct Ws {
  Hdr* h;
  u64 *ka, *kb;
  uint32_t *va, *vb, *table;
  char* aux;            // 24 n bytes: sorted coordinates (stray) / per-column extremes and run heads (shadows)
};
int64_t ws_bytes_for(int64_t n_max) {
  const int64_t n = n_max < 0 ? 0 : n_max;
  return al256(sizeof(Hdr)) + 2 * al256(8 * n) + 2 * al256(4 * n) + al256((int64_t)sort_blocks(n) * 1024) +
         al256(24 * n) + 256;
}
bool ws_carve(void* ws, int64_t bytes, int n_max, Ws* o) {
  if (!ws || bytes < ws_bytes_for(n_max) || ((uintptr_t)ws & 7)) return false;
  const int64_t n = n_max;
  char* p = (char*)ws;
  o->h = (Hdr*)p;         p += al256(sizeof(Hdr));
  o->ka = (u64*)p;        p += al256(8 * n);
  o->kb = (u64*)p;        p += al256(8 * n);
  o->va = (uint32_t*)p;   p += al256(4 * n);
  o->vb = (uint32_t*)p;   p += al256(4 * n);
  o->table = (uint32_t*)p; p += al256((int64_t)sort_blocks(n) * 1024);
  o->aux = p;
  return true;
}

// ---- shared by the two stages: this, and minmax3_kernel of dp_grid3.h ----------------------------
__global__ void hdr_init_kernel(Hdr* h) { grid3_reset(&h->g); }

// ---- stray points -------------------------------------------------------------------------------
// The grid (cell edge radius * EDGE_SLACK, keys, gathered coordinates) is dp_grid3.h's, and so is the
// argument why the 3 x 3 x 3 cells around a point hold every true neighbour.
// One thread per point, in sorted (cell) order.  Own (x, y) cell row first; every row's three
// z-adjacent cells are one key range.  Stops at nb_points.
__global__ void __launch_bounds__(256) stray_count_kernel(const u64* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                          const double* __restrict__ sp, const int32_t* n_dev, int n_max,
                                                          double r2, int nb, Hdr* h, uint8_t* __restrict__ keep) {
  const int n = live_n(n_dev, n_max);
  const bool err = h->g.err != 0;
  for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
    const long long t = base + threadIdx.x;
    bool kept = false;
    if (t < n) {
      const u64 key = keys[t];
      if (err) {
        kept = true;
      } else if (key != NO_KEY) {
        int cx, cy, cz;
        unpack_cell(key, cx, cy, cz);
        const double x = sp[3 * t], y = sp[3 * t + 1], z = sp[3 * t + 2];
        int cnt = 0;
        for (int row = 0; row < 9 && cnt < nb; ++row) {
          // row 0 is (0, 0); the others follow in any fixed order
          const int rr = row == 0 ? 4 : (row <= 4 ? row - 1 : row);
          const int rx = cx + rr / 3 - 1, ry = cy + rr % 3 - 1;
          if (rx < 0 || ry < 0 || rx > CELL_MAX + 1 || ry > CELL_MAX + 1) continue;
          int a, b;
          cell_row_range(keys, n, rx, ry, cz > 0 ? cz - 1 : 0, cz + 1, a, b);
          for (int c = a; c < b && cnt < nb; ++c) {
            const double dx = sp[3 * (size_t)c] - x, dy = sp[3 * (size_t)c + 1] - y, dz = sp[3 * (size_t)c + 2] - z;
            if ((dx * dx + dy * dy) + dz * dz < r2) ++cnt;
          }
        }
        kept = cnt >= nb;
      }
      if (idx[t] < (uint32_t)n) keep[idx[t]] = kept;
    }
    wave_count(&h->ctr[C_KEPT], kept);
  }
}

__global__ void stray_final_kernel(const Hdr* h, const int32_t* n_dev, int n_max, double* st) {
  const int n = live_n(n_dev, n_max);
  st[0] = (double)h->g.finite;
  st[1] = (double)h->g.nonfinite;
  st[2] = (double)h->ctr[C_KEPT];
  st[3] = (double)(n - (int)h->ctr[C_KEPT]);
  st[4] = (double)h->g.err;
  st[5] = st[6] = st[7] = 0.0;
}

// ---- shadows ------------------------------------------------------------------------------------
// np.arange(start, stop, cell) as numpy fills it: e[0] = start, e[1] = start + cell,
// e[i] = start + i * (e[1] - e[0]) from i = 2 on.
struct Bins { double start, e1, delta; int len; };
__device__ __forceinline__ double edge_at(const Bins& b, int i) {
  return i == 0 ? b.start : (i == 1 ? b.e1 : b.start + (double)i * b.delta);
}
// np.digitize(v, e) - 1: the last i with e[i] <= v (edges are non-decreasing in i)
__device__ __forceinline__ int digitize_m1(const Bins& b, double v) {
  int lo = 0, hi = b.len;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (edge_at(b, mid) <= v) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}
__device__ __forceinline__ Bins bins_of(const Hdr* h, int axis) {   // axis 0: x, 1: z
  Bins b;
  b.start = h->par[axis];
  b.e1 = b.start + h->par[2];
  b.delta = b.e1 - b.start;
  b.len = (int)h->ctr[C_LENX + axis];
  return b;
}

__global__ void shadow_setup_kernel(Hdr* h) {
  const uint32_t nf = h->g.finite;
  double cell = 0.05;
  uint32_t lx = 0, lz = 0, err = 0;
  if (nf) {
    const double x0 = unkey(h->g.mm[0]), x1 = unkey(h->g.mm[1]), z0 = unkey(h->g.mm[4]), z1 = unkey(h->g.mm[5]);
    const double density = (double)nf / ((x1 - x0) * (z1 - z0));
    const double v = 1.0 / __builtin_sqrt(density / 10.0);
    cell = v > 0.05 ? v : 0.05;                     // Python's max(0.05, v): 0.05 unless v > 0.05 (NaN included)
    const double fx = __builtin_ceil(((x1 + cell) - x0) / cell), fz = __builtin_ceil(((z1 + cell) - z0) / cell);
    h->par[0] = x0;
    h->par[1] = z0;
    // the column id must fit 31 bits; a non-finite length or edges that do not grow are refused as well
    if (!(fx >= 1.0 && fz >= 1.0 && fx * fz < 2147483648.0) || !((x0 + cell) - x0 > 0.0) || !((z0 + cell) - z0 > 0.0)) {
      err = 1;
    } else {
      lx = (uint32_t)fx;
      lz = (uint32_t)fz;
    }
  }
  h->par[2] = cell;
  h->ctr[C_LENX] = lx;
  h->ctr[C_LENZ] = lz;
  h->ctr[C_SHADOW_ERR] = err;
}

__global__ void __launch_bounds__(256) shadow_ykey_kernel(const double* __restrict__ pts, const int32_t* n_dev, int n_max,
                                                          u64* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int n = live_n(n_dev, n_max);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    keys[i] = finite3(x, y, z) ? okey(y) : ~0ull;
    vals[i] = (uint32_t)i;
  }
}

// second key: the column id of the point now at sorted position t
__global__ void __launch_bounds__(256) shadow_colkey_kernel(const double* __restrict__ pts, const uint32_t* __restrict__ idx,
                                                            const int32_t* n_dev, int n_max, const Hdr* h,
                                                            u64* __restrict__ keys) {
  const int n = live_n(n_dev, n_max);
  const bool err = h->ctr[C_SHADOW_ERR] != 0;
  const Bins bx = bins_of(h, 0), bz = bins_of(h, 1);
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) {
    const size_t i = row_of(idx[t], n);
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    uint32_t col = NO_COL;
    if (!err && finite3(x, y, z)) col = (uint32_t)digitize_m1(bx, x) * (uint32_t)bz.len + (uint32_t)digitize_m1(bz, z);
    keys[t] = col;
  }
}

// the per-run accumulators (indexed by the run's head position)
__global__ void __launch_bounds__(256) shadow_clear_kernel(const int32_t* n_dev, int n_max, u64* __restrict__ amax,
                                                           u64* __restrict__ amin, uint32_t* __restrict__ cnt) {
  const int n = live_n(n_dev, n_max);
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) {
    amax[t] = 0;
    amin[t] = ~0ull;
    cnt[t] = 0;
  }
}

// Angle of each consecutive pair of a column run, reduced onto the run's head position: number of
// angles below the limit, the largest of those, the smallest of the others, and a NaN flag (bit 31).
__global__ void __launch_bounds__(256) shadow_angle_kernel(const double* __restrict__ pts, const u64* __restrict__ keys,
                                                           const uint32_t* __restrict__ idx, const int32_t* n_dev,
                                                           int n_max, double max_angle, u64* __restrict__ amax,
                                                           u64* __restrict__ amin, uint32_t* __restrict__ cnt,
                                                           uint32_t* __restrict__ head_of) {
  const int n = live_n(n_dev, n_max), lane = threadIdx.x & 63;
  for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
    const long long t = base + threadIdx.x;
    int head = -1;
    bool below = false, isnan = false;
    u64 ak = 0;
    if (t < n) {
      const u64 col = keys[t];
      if (col != NO_COL) {
        const int hd = lower_bound(keys, n, col);
        head_of[t] = (uint32_t)hd;
        if (t > hd) {
          const size_t i = row_of(idx[t], n), j = row_of(idx[t - 1], n);
          const double vx = pts[3 * i] - pts[3 * j], vy = pts[3 * i + 1] - pts[3 * j + 1], vz = pts[3 * i + 2] - pts[3 * j + 2];
          double c = vy / __builtin_sqrt((vx * vx + vy * vy) + vz * vz);
          c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);                   // np.clip keeps NaN
          const double a = acos(c) * 180.0 / 3.141592653589793;
          head = hd;
          isnan = a != a;
          below = a < max_angle;
          ak = okey(a);
        }
      }
    }
    // one set of atomics per distinct run in the wave
    u64 todo = __ballot(head >= 0);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int lh = __shfl(head, leader);
      const bool mine = head == lh;
      const u64 nb = __ballot(mine && below), nn = __ballot(mine && isnan);
      u64 mx = mine && below ? ak : 0ull, mn = mine && !below && !isnan ? ak : ~0ull;
      #pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const u64 t0 = __shfl_xor(mx, o), t1 = __shfl_xor(mn, o);
        mx = t0 > mx ? t0 : mx;
        mn = t1 < mn ? t1 : mn;
      }
      if (lane == leader) {
        if (nb) { atomicAdd(&cnt[lh], (uint32_t)__popcll(nb)); atomicMax(&amax[lh], mx); }
        if (mn != ~0ull) atomicMin(&amin[lh], mn);
        if (nn) atomicOr(&cnt[lh], 0x80000000u);
      }
      todo &= ~__ballot(mine);
    }
  }
}

// One thread per run head: count, height (first and last y of the run: it is sorted by y) and the
// median rule.  Leaves 1 in cnt[head] if the column is removed, else 0.
__global__ void __launch_bounds__(256) shadow_decide_kernel(const double* __restrict__ pts, const u64* __restrict__ keys,
                                                            const uint32_t* __restrict__ idx, const int32_t* n_dev,
                                                            int n_max, double height_thr, double max_angle, int min_pts,
                                                            const u64* __restrict__ amax, const u64* __restrict__ amin,
                                                            uint32_t* __restrict__ cnt, Hdr* h) {
  const int n = live_n(n_dev, n_max);
  for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
    const long long t = base + threadIdx.x;
    bool is_head = false, tested = false, removed = false;
    uint32_t count = 0;
    if (t < n) {
      const u64 col = keys[t];
      is_head = col != NO_COL && (t == 0 || keys[t - 1] != col);
      if (is_head) {
        count = (uint32_t)(lower_bound(keys, n, col + 1) - (int)t);
        const double y0 = pts[3 * (size_t)row_of(idx[t], n) + 1], y1 = pts[3 * (size_t)row_of(idx[t + count - 1], n) + 1];
        tested = count >= (uint32_t)min_pts && count >= 3 && (y1 - y0) > height_thr;
        if (tested) {
          const uint32_t raw = cnt[t], c = raw & 0x7fffffffu, m = count - 1;
          if (!(raw & 0x80000000u)) {                       // a NaN angle: NaN median, kept
            if (m & 1u) removed = c >= (m + 1) / 2;
            else if (c != m / 2) removed = c > m / 2;
            else removed = (unkey(amax[t]) + unkey(amin[t])) / 2.0 < max_angle;
          }
        }
        cnt[t] = removed;
      }
    }
    wave_count(&h->ctr[C_OCC], is_head);
    wave_count(&h->ctr[C_TESTED], tested);
    wave_count(&h->ctr[C_REMCOL], removed);
    if (removed) atomicAdd(&h->ctr[C_REMPTS], count);
  }
}

__global__ void __launch_bounds__(256) shadow_mark_kernel(const u64* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                          const int32_t* n_dev, int n_max, const uint32_t* __restrict__ cnt,
                                                          const uint32_t* __restrict__ head_of, uint8_t* __restrict__ keep) {
  const int n = live_n(n_dev, n_max);
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256)
    if (idx[t] < (uint32_t)n) keep[idx[t]] = keys[t] == NO_COL ? 1 : !cnt[row_of(head_of[t], n)];
}

__global__ void shadow_final_kernel(const Hdr* h, double* st) {
  st[0] = (double)h->g.finite;
  st[1] = (double)h->g.nonfinite;
  st[2] = (double)h->ctr[C_OCC];
  st[3] = (double)h->ctr[C_TESTED];
  st[4] = (double)h->ctr[C_REMCOL];
  st[5] = (double)h->ctr[C_REMPTS];
  st[6] = h->par[2];
  st[7] = (double)h->ctr[C_SHADOW_ERR];
}

// ---- compaction ---------------------------------------------------------------------------------
// the flags' scan is scan_count_kernel and scan_blocks_kernel (dp_points.h); this moves the rows
__global__ void __launch_bounds__(256) compact_scatter_kernel(const double* __restrict__ pts, const uint8_t* __restrict__ cols,
                                                              const uint8_t* __restrict__ keep, const int32_t* n_dev,
                                                              int n_max, const uint32_t* __restrict__ bc,
                                                              double* __restrict__ pts_out, uint8_t* __restrict__ cols_out) {
  __shared__ uint32_t wsum[4];
  const int n = live_n(n_dev, n_max);
  const long long tile = (long long)blockIdx.x * SCAN_TILE;
  uint32_t run = bc[blockIdx.x];
  for (int r = 0; r < SCAN_ITEMS && tile + r * 256 < n; ++r) {
    const long long i = tile + r * 256 + threadIdx.x;
    const bool k = i < n && keep[i];
    uint32_t tot = 0;
    const uint32_t off = run + block_excl_scan(k ? 1u : 0u, wsum, &tot);
    if (k && off < (uint32_t)n) {
      pts_out[3 * (size_t)off] = pts[3 * i]; pts_out[3 * (size_t)off + 1] = pts[3 * i + 1];
      pts_out[3 * (size_t)off + 2] = pts[3 * i + 2];
      if (cols) {
        cols_out[3 * (size_t)off] = cols[3 * i]; cols_out[3 * (size_t)off + 1] = cols[3 * i + 1];
        cols_out[3 * (size_t)off + 2] = cols[3 * i + 2];
      }
    }
    run += tot;
  }
}
}  // namespace

extern "C" int64_t dp_clean_workspace_size(int64_t n_max) { return ws_bytes_for(n_max); }

extern "C" int dp_sort_pairs(uint64_t* keys, uint32_t* values, const int32_t* n_dev, int32_t n_max, int32_t bit_lo,
                             int32_t bit_hi, void* workspace, int64_t workspace_bytes, dp_stream_t stream) {
  if (n_max > 0 && (!keys || !values)) return DP_ERR_ARG;
  if (n_max < 0 || bit_lo < 0 || bit_hi > 64 || bit_lo > bit_hi) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, n_max, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (run_sort(s, w.h, (u64*)keys, values, w.kb, w.vb, w.table, n_dev, n_max, bit_lo, bit_hi))
    hipLaunchKernelGGL(copy_pairs_kernel, dim3(grid_for(n_max, GRID_CAP)), dim3(256), 0, s, w.kb, w.vb, (u64*)keys, values,
                       n_dev, n_max);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_clean_stray(const double* points, const int32_t* n_dev, int32_t n_max, double radius,
                              int32_t nb_points, uint8_t* keep_out, double* stats_out, void* workspace,
                              int64_t workspace_bytes, dp_stream_t stream) {
  if (!stats_out || (n_max > 0 && (!points || !keep_out))) return DP_ERR_ARG;
  if (n_max < 0 || nb_points < 1 || !(radius > 0.0) || !(radius < __builtin_inf())) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, n_max, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int g = grid_for(n_max, GRID_CAP);
  double* sp = (double*)w.aux;
  (void)hipMemsetAsync(w.h, 0, sizeof(Hdr), s);
  hipLaunchKernelGGL(hdr_init_kernel, dim3(1), dim3(1), 0, s, w.h);
  grid3_keys(s, &w.h->g, g, points, n_dev, n_max, radius * EDGE_SLACK, 0.0, w.ka, w.va);
  const bool in_b = run_sort(s, w.h, w.ka, w.va, w.kb, w.vb, w.table, n_dev, n_max, 0, 64);
  const u64* sk = in_b ? w.kb : w.ka;
  const uint32_t* si = in_b ? w.vb : w.va;
  hipLaunchKernelGGL(gather_points_kernel, dim3(g), dim3(256), 0, s, points, si, n_dev, n_max, sp);
  hipLaunchKernelGGL(stray_count_kernel, dim3(g), dim3(256), 0, s, sk, si, sp, n_dev, n_max, radius * radius,
                     nb_points, w.h, keep_out);
  hipLaunchKernelGGL(stray_final_kernel, dim3(1), dim3(1), 0, s, w.h, n_dev, n_max, stats_out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_clean_shadows(const double* points, const int32_t* n_dev, int32_t n_max, double height_threshold,
                                double max_angle, int32_t min_points, uint8_t* keep_out, double* stats_out,
                                void* workspace, int64_t workspace_bytes, dp_stream_t stream) {
  if (!stats_out || (n_max > 0 && (!points || !keep_out))) return DP_ERR_ARG;
  if (n_max < 0 || min_points < 1 || height_threshold != height_threshold || max_angle != max_angle) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, n_max, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int g = grid_for(n_max, GRID_CAP);
  u64* amin = (u64*)w.aux;                                        // aux: 8 n + 4 n of its 24 n bytes
  uint32_t* head_of = (uint32_t*)(w.aux + al256(8 * (int64_t)n_max));
  (void)hipMemsetAsync(w.h, 0, sizeof(Hdr), s);
  hipLaunchKernelGGL(hdr_init_kernel, dim3(1), dim3(1), 0, s, w.h);
  hipLaunchKernelGGL(minmax3_kernel, dim3(g), dim3(256), 0, s, points, n_dev, n_max, &w.h->g);
  hipLaunchKernelGGL(shadow_setup_kernel, dim3(1), dim3(1), 0, s, w.h);
  hipLaunchKernelGGL(shadow_ykey_kernel, dim3(g), dim3(256), 0, s, points, n_dev, n_max, w.ka, w.va);
  // by y (64 bits), then by column id (32 bits): the second sort is stable, so a column's run is in
  // y order with ties in index order.  8 and 4 passes: both results land in (ka, va).
  run_sort(s, w.h, w.ka, w.va, w.kb, w.vb, w.table, n_dev, n_max, 0, 64);
  hipLaunchKernelGGL(shadow_colkey_kernel, dim3(g), dim3(256), 0, s, points, w.va, n_dev, n_max, w.h, w.ka);
  run_sort(s, w.h, w.ka, w.va, w.kb, w.vb, w.table, n_dev, n_max, 0, 32);
  u64* amax = w.kb;                                               // the sort's other buffers are free after it
  uint32_t* cnt = w.vb;
  hipLaunchKernelGGL(shadow_clear_kernel, dim3(g), dim3(256), 0, s, n_dev, n_max, amax, amin, cnt);
  hipLaunchKernelGGL(shadow_angle_kernel, dim3(g), dim3(256), 0, s, points, w.ka, w.va, n_dev, n_max, max_angle, amax, amin,
                     cnt, head_of);
  hipLaunchKernelGGL(shadow_decide_kernel, dim3(g), dim3(256), 0, s, points, w.ka, w.va, n_dev, n_max, height_threshold,
                     max_angle, min_points, amax, amin, cnt, w.h);
  hipLaunchKernelGGL(shadow_mark_kernel, dim3(g), dim3(256), 0, s, w.ka, w.va, n_dev, n_max, cnt, head_of, keep_out);
  hipLaunchKernelGGL(shadow_final_kernel, dim3(1), dim3(1), 0, s, w.h, stats_out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_compact_points(const double* points, const uint8_t* colors, const uint8_t* keep, const int32_t* n_dev,
                                 int32_t n_max, double* points_out, uint8_t* colors_out, int32_t* n_out_dev,
                                 void* workspace, int64_t workspace_bytes, dp_stream_t stream) {
  if (!n_out_dev || (n_max > 0 && (!points || !keep || !points_out || (colors && !colors_out)))) return DP_ERR_ARG;
  if (n_max < 0) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, n_max, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int nb = (int)scan_blocks_for(n_max);
  uint32_t* bc = w.va;                                            // n / 2048 words
  if (nb) hipLaunchKernelGGL(scan_count_kernel, dim3(nb), dim3(256), 0, s, keep, n_dev, n_max, bc);
  hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(256), 0, s, bc, nb, (uint32_t*)n_out_dev);   // the same bits
  if (nb)
    hipLaunchKernelGGL(compact_scatter_kernel, dim3(nb), dim3(256), 0, s, points, colors, keep, n_dev, n_max, bc, points_out,
                       colors_out);
  DP_CHECK_LAUNCH();
  return 0;
}
