// Clustered point clouds (ABI 17): exact DBSCAN labels over (x, z) and a per-cluster table, on the
// stable radix sort of dp_clean.hip (dp_sort_pairs).  fp64 as numpy computes it; no FMA contraction
// anywhere in this file, so each product and sum is rounded on its own.  The specification (rules
// 1-5, sampling) is in the header; this file is the method:
//   eligibility -> scan -> stride sample -> cell keys -> sort -> core flags -> lock-free union-find
//   over core points in row-index space -> root ranks (scan) -> labels.
// No kernel waits on another workgroup's progress: union-find retries on its own CAS only, and every
// per-thread loop runs over the contents of at most 25 cells, never over n_max.
#include "dp_common.h"
#include "dp_points.h"

#pragma clang fp contract(off)

namespace {

constexpr int GRID_CAP = 4096;                  // workgroups of a per-point kernel at the most
constexpr int CELL_BITS = 21;                   // bits per axis of the packed cell key
constexpr int CELL_MAX = (1 << CELL_BITS) - 3;  // largest cell coordinate (its +2 neighbour still fits)
constexpr u64 NO_CELL = 1ull << (2 * CELL_BITS);   // key of a row that takes no part: sorts last
constexpr u64 NO_LABEL = 1ull << 32;               // table: key of an unlabelled row
constexpr uint32_t MAGIC = 0x44424331u;         // "DBC1": the workspace holds a finished run's roots

struct CHdr {
  u64 mm[4];            // keys of min / max of x, z over the participants
  uint32_t ctr[16];
  double par[4];        // x min, z min, cell edge
  uint32_t magic, stamp_n;
};
enum { C_FINITE = 0, C_NONFINITE = 1, C_ELIG = 2, C_PART = 3, C_CORE = 4, C_BORDER = 5, C_NCL = 6, C_ERR = 7,
       C_NP = 8 };

// ---- exclusive scan of a byte flag in row order: scan_count_kernel, scan_blocks_kernel (dp_points.h),
// then the ranks
__global__ void __launch_bounds__(256) scan_write_kernel(const uint8_t* __restrict__ f, const int32_t* n_dev, int n_max,
                                                         const uint32_t* __restrict__ bc, uint32_t* __restrict__ out) {
  __shared__ uint32_t wsum[4];
  const int n = live_n(n_dev, n_max);
  const long long tile = (long long)blockIdx.x * SCAN_TILE;
  uint32_t run = bc[blockIdx.x];
  for (int r = 0; r < SCAN_ITEMS && tile + r * 256 < n; ++r) {
    const long long i = tile + r * 256 + threadIdx.x;
    const bool k = i < n && f[i];
    uint32_t tot = 0;
    const uint32_t off = run + block_excl_scan(k ? 1u : 0u, wsum, &tot);
    if (i < n) out[i] = off;
    run += tot;
  }
}

// ---- participants -------------------------------------------------------------------------------
__global__ void hdr_init_kernel(CHdr* h) {
  h->mm[0] = h->mm[2] = ~0ull;
  h->mm[1] = h->mm[3] = 0;
}

__global__ void __launch_bounds__(256) elig_kernel(const double* __restrict__ pts, const int32_t* n_dev, int n_max,
                                                   double height_thr, CHdr* h, uint8_t* __restrict__ elig) {
  const int n = live_n(n_dev, n_max);
  const bool any_height = height_thr != height_thr;
  for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
    const long long i = base + threadIdx.x;
    bool finite = false, live = i < n;
    if (live) {
      const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
      finite = fin(x) && fin(y) && fin(z);
      elig[i] = finite && (any_height || y >= height_thr);
    }
    wave_count(&h->ctr[C_FINITE], finite);
    wave_count(&h->ctr[C_NONFINITE], live && !finite);
  }
}

// The stride sample: with e eligible rows and m = max_points < e, the k-th eligible row takes part
// iff floor(k m / e) != floor((k - 1) m / e) (k = 0 always): exactly m rows.  Also resets the row's
// label, its union-find parent and its root flag, and reduces the participants' extent.
__global__ void __launch_bounds__(256) part_kernel(const double* __restrict__ pts, const int32_t* n_dev, int n_max,
                                                   int max_points, const uint32_t* __restrict__ ek, CHdr* h,
                                                   uint8_t* __restrict__ part, int32_t* __restrict__ labels,
                                                   uint32_t* __restrict__ parent, uint8_t* __restrict__ rootf) {
  const int n = live_n(n_dev, n_max);
  const u64 e = h->ctr[C_ELIG], m = (u64)max_points;
  const bool all = m == 0 || e <= m;
  u64 mn[2] = {~0ull, ~0ull}, mx[2] = {0, 0};
  uint32_t cnt = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    bool p = part[i] != 0;
    if (p && !all) {
      const u64 k = ek[i];
      p = k == 0 || (k * m) / e != ((k - 1) * m) / e;
    }
    part[i] = p;
    labels[i] = p ? -1 : -2;
    parent[i] = (uint32_t)i;
    rootf[i] = 0;
    if (p) {
      ++cnt;
      const u64 k[2] = {okey(pts[3 * i]), okey(pts[3 * i + 2])};
      #pragma unroll
      for (int a = 0; a < 2; ++a) { mn[a] = k[a] < mn[a] ? k[a] : mn[a]; mx[a] = k[a] > mx[a] ? k[a] : mx[a]; }
    }
  }
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    wave_minmax(mn, mx, o);
    cnt += __shfl_xor(cnt, o);
  }
  if ((threadIdx.x & 63) == 0 && cnt) {
    flush_minmax(h->mm, mn, mx);
    atomicAdd(&h->ctr[C_PART], cnt);
  }
}

// ---- the grid -----------------------------------------------------------------------------------
// Cell edge g = eps / sqrt(2) * (1 - 2^-20), cell = floor((p - min) / g) per axis (x, z).
//  * Two points of one cell are neighbours.  Their exact quotients differ by less than 1; a computed
//    quotient (a subtraction, a division and g itself, each rounded once) is within 2^-50 relative of
//    the exact one and below 2^21, so within 2^-29 absolute: |dx|, |dz| < g (1 + 2^-28), hence
//    dx^2 + dz^2 < 2 g^2 (1 + 2^-27) = eps^2 (1 - 2^-20)^2 (1 + 2^-27), and the five roundings of the
//    distance test (2^-52 relative each) cannot lift that over eps^2: the 2^-20 margin is 2^30 times
//    larger.  This is the dense-cell rule: a cell with >= min_samples participants makes all of them
//    core, and all of them one set, without a single distance test -- k coincident points cost
//    O(k log n), not k^2.
//  * Every neighbour of a point lies in the 5 x 5 block of cells around its own: cells 3 apart on an
//    axis have exact quotients more than 2 - 2^-28 apart, a distance above 1.41 eps.  The four corner
//    cells stay in the walk: with the shrunk edge two points across a corner can be as close as
//    sqrt(2) g = eps (1 - 2^-20) < eps.
// Cells only select candidates: the distance test runs on the original coordinates.
__global__ void setup_kernel(CHdr* h, double eps) {
  const double edge = eps / __builtin_sqrt(2.0) * (1.0 - 1.0 / 1048576.0);
  const bool any = h->ctr[C_PART] != 0;
  bool err = !(edge > 0.0);
  for (int a = 0; a < 2; ++a) {
    const double mn = any ? unkey(h->mm[2 * a]) : 0.0, mx = any ? unkey(h->mm[2 * a + 1]) : 0.0;
    h->par[a] = mn;
    if (!((mx - mn) / edge < (double)CELL_MAX)) err = true;      // also catches an overflowing extent
  }
  h->par[2] = edge;
  h->ctr[C_ERR] = err;
  h->ctr[C_NP] = err ? 0u : h->ctr[C_PART];
}

__device__ __forceinline__ u64 pack_cell(u64 cx, u64 cz) { return (cx << CELL_BITS) | cz; }

__global__ void __launch_bounds__(256) key_kernel(const double* __restrict__ pts, const int32_t* n_dev, int n_max,
                                                  const CHdr* h, const uint8_t* __restrict__ part,
                                                  u64* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int n = live_n(n_dev, n_max);
  const double mx = h->par[0], mz = h->par[1], edge = h->par[2];
  const bool err = h->ctr[C_ERR] != 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    keys[i] = part[i] && !err
                  ? pack_cell(cell_of<CELL_MAX>(pts[3 * i], mx, edge), cell_of<CELL_MAX>(pts[3 * i + 2], mz, edge))
                  : NO_CELL;
    vals[i] = (uint32_t)i;
  }
}

// per sorted position: coordinates and the bounds of its cell's run
__global__ void __launch_bounds__(256) cells_kernel(const double* __restrict__ pts, const u64* __restrict__ keys,
                                                    const uint32_t* __restrict__ idx, const int32_t* n_dev, int n_max,
                                                    const CHdr* h, double* __restrict__ sx, double* __restrict__ sz,
                                                    uint32_t* __restrict__ cbeg, uint32_t* __restrict__ cend) {
  const int n = live_n(n_dev, n_max);
  const int np = (int)h->ctr[C_NP] < n ? (int)h->ctr[C_NP] : n;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < np; t += (long long)gridDim.x * 256) {
    const size_t i = row_of(idx[t], n);
    sx[t] = pts[3 * i];
    sz[t] = pts[3 * i + 2];
    const u64 key = keys[t];
    cbeg[t] = (uint32_t)lower_bound(keys, np, key);
    cend[t] = (uint32_t)lower_bound(keys, np, key + 1);
  }
}

// The walk over the 5 x 5 block around a cell: 5 rows (one x cell each), a row's five z-adjacent
// cells being one key range.  Row 0 is the point's own.
struct Walk {
  long long cx, cz;
  __device__ __forceinline__ Walk(u64 key) : cx((long long)(key >> CELL_BITS)), cz((long long)(key & ((1 << CELL_BITS) - 1))) {}
  __device__ __forceinline__ bool row(int r, const u64* __restrict__ keys, int np, int* a, int* b) const {
    const int d = r == 0 ? 0 : (r <= 2 ? r - 3 : r - 2);         // 0, -2, -1, +1, +2
    const long long rx = cx + d;
    if (rx < 0 || rx > CELL_MAX + 2) return false;
    const u64 zlo = (u64)(cz > 2 ? cz - 2 : 0), zhi = (u64)(cz + 2);
    *a = lower_bound(keys, np, pack_cell((u64)rx, zlo));
    *b = lower_bound(keys, np, pack_cell((u64)rx, zhi) + 1);
    return true;
  }
};

__device__ __forceinline__ bool is_near(const double* __restrict__ sx, const double* __restrict__ sz, int c, double x, double z,
                                     double eps2) {
  const double dx = sx[c] - x, dz = sz[c] - z;
  return dx * dx + dz * dz <= eps2;
}

// Core flags.  A cell with >= min_samples participants makes all of them core at once (the
// dense-cell rule above); the others count neighbours and stop at min_samples.
__global__ void __launch_bounds__(256) core_kernel(const u64* __restrict__ keys, const double* __restrict__ sx,
                                                   const double* __restrict__ sz, const uint32_t* __restrict__ cbeg,
                                                   const uint32_t* __restrict__ cend, double eps2, int ms, CHdr* h,
                                                   uint8_t* __restrict__ core) {
  const int np = (int)h->ctr[C_NP];
  for (long long base = (long long)blockIdx.x * 256; base < np; base += (long long)gridDim.x * 256) {
    const long long t = base + threadIdx.x;
    bool is_core = false;
    if (t < np) {
      const int cb = (int)cbeg[t], ce = (int)cend[t];
      int cnt = ce - cb;                                         // the own cell: neighbours without a test
      if (cnt < ms) {
        const Walk w(keys[t]);
        const double x = sx[t], z = sz[t];
        for (int r = 0; r < 5 && cnt < ms; ++r) {
          int a, b;
          if (!w.row(r, keys, np, &a, &b)) continue;
          for (int c = a; c < b && cnt < ms; ++c) {
            if (c >= cb && c < ce) { c = ce - 1; continue; }
            cnt += is_near(sx, sz, c, x, z, eps2);
          }
        }
      }
      is_core = cnt >= ms;
      core[t] = is_core;
    }
    wave_count(&h->ctr[C_CORE], is_core);
  }
}

// ---- union-find over core points, in row-index space (uf_find / uf_unite: dp_points.h) -----------
// A dense cell joins all its points to its first one (the smallest row of the cell: the sort is
// stable).  A neighbouring dense cell is one set already, so it is skipped when that set is the
// point's own, and left at the first neighbour found in it.
__global__ void __launch_bounds__(256) union_kernel(const u64* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                    const double* __restrict__ sx, const double* __restrict__ sz,
                                                    const uint32_t* __restrict__ cbeg, const uint32_t* __restrict__ cend,
                                                    const uint8_t* __restrict__ core, double eps2, int ms, const CHdr* h,
                                                    int n_max, uint32_t* parent) {
  const int np = (int)h->ctr[C_NP];
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < np; t += (long long)gridDim.x * 256) {
    if (!core[t]) continue;
    const uint32_t i = row_of(idx[t], n_max);
    const int cb = (int)cbeg[t], ce = (int)cend[t];
    if (ce - cb >= ms) {
      if (t != cb) uf_unite(parent, i, row_of(idx[cb], n_max));
    } else {
      for (int c = cb; c < ce; ++c)
        if (c != t && core[c]) uf_unite(parent, i, row_of(idx[c], n_max));
    }
    const Walk w(keys[t]);
    const double x = sx[t], z = sz[t];
    for (int r = 0; r < 5; ++r) {
      int a, b;
      if (!w.row(r, keys, np, &a, &b)) continue;
      for (int c = a; c < b; ++c) {
        if (c >= cb && c < ce) { c = ce - 1; continue; }
        if (!core[c]) continue;
        const int qb = (int)cbeg[c], qe = (int)cend[c];
        const bool dense = qe - qb >= ms;
        const uint32_t j = row_of(idx[c], n_max);
        if (dense && c == qb && uf_find(parent, j) == uf_find(parent, i)) { c = qe - 1; continue; }
        if (is_near(sx, sz, c, x, z, eps2)) {
          uf_unite(parent, i, j);
          if (dense) c = qe - 1;
        }
      }
    }
  }
}

__global__ void __launch_bounds__(256) compress_kernel(const uint32_t* __restrict__ idx, const uint8_t* __restrict__ core,
                                                       const CHdr* h, int n_max, uint32_t* parent,
                                                       uint8_t* __restrict__ rootf) {
  const int np = (int)h->ctr[C_NP];
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < np; t += (long long)gridDim.x * 256) {
    if (!core[t]) continue;
    const uint32_t i = row_of(idx[t], n_max);
    const uint32_t r = uf_find(parent, i);
    if (r != i) atomicMin(&parent[i], r);
    else rootf[i] = 1;
  }
}

// Labels.  rank[] is the exclusive scan of the root flags in row order, so rank[root] is the number
// of clusters with a smaller smallest core row: rule 3's numbering.  A border point takes the
// smallest cluster number among its core neighbours; one hit per dense cell is enough (the cell is
// one cluster).
__global__ void __launch_bounds__(256) label_kernel(const u64* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                    const double* __restrict__ sx, const double* __restrict__ sz,
                                                    const uint32_t* __restrict__ cbeg, const uint32_t* __restrict__ cend,
                                                    const uint8_t* __restrict__ core, const uint32_t* __restrict__ parent,
                                                    const uint32_t* __restrict__ rank, double eps2, int ms, CHdr* h,
                                                    int n_max, int32_t* __restrict__ labels, uint32_t* __restrict__ roots) {
  const int np = (int)h->ctr[C_NP];
  for (long long base = (long long)blockIdx.x * 256; base < np; base += (long long)gridDim.x * 256) {
    const long long t = base + threadIdx.x;
    bool border = false;
    if (t < np) {
      const uint32_t i = row_of(idx[t], n_max);
      if (core[t]) {
        const uint32_t root = row_of(parent[i], n_max), c = rank[root];
        labels[i] = (int32_t)c;
        if (root == i && c < (uint32_t)n_max) roots[c] = i;
      } else {
        const int cb = (int)cbeg[t], ce = (int)cend[t];
        uint32_t best = 0xffffffffu;
        for (int c = cb; c < ce; ++c)                            // the own cell (never dense here)
          if (core[c]) {
            const uint32_t l = rank[row_of(parent[row_of(idx[c], n_max)], n_max)];
            best = l < best ? l : best;
          }
        const Walk w(keys[t]);
        const double x = sx[t], z = sz[t];
        for (int r = 0; r < 5; ++r) {
          int a, b;
          if (!w.row(r, keys, np, &a, &b)) continue;
          for (int c = a; c < b; ++c) {
            if (c >= cb && c < ce) { c = ce - 1; continue; }
            if (!core[c] || !is_near(sx, sz, c, x, z, eps2)) continue;
            const uint32_t l = rank[row_of(parent[row_of(idx[c], n_max)], n_max)];
            best = l < best ? l : best;
            if ((int)(cend[c] - cbeg[c]) >= ms) c = (int)cend[c] - 1;
          }
        }
        border = best != 0xffffffffu;
        if (border) labels[i] = (int32_t)best;
      }
    }
    wave_count(&h->ctr[C_BORDER], border);
  }
}

__global__ void final_kernel(CHdr* h, int n_max, int32_t* n_clusters, double* st) {
  const uint32_t ncl = h->ctr[C_ERR] ? 0u : h->ctr[C_NCL];
  st[0] = (double)h->ctr[C_FINITE];
  st[1] = (double)h->ctr[C_NONFINITE];
  st[2] = (double)h->ctr[C_PART];
  st[3] = (double)h->ctr[C_CORE];
  st[4] = (double)h->ctr[C_BORDER];
  st[5] = (double)(h->ctr[C_PART] - h->ctr[C_CORE] - h->ctr[C_BORDER]);
  st[6] = (double)ncl;
  st[7] = (double)h->ctr[C_ERR];
  *n_clusters = (int32_t)ncl;
  h->ctr[C_NCL] = ncl;
  h->stamp_n = (uint32_t)n_max;
  h->magic = MAGIC;
}

// ---- the cluster table ----------------------------------------------------------------------------
__global__ void __launch_bounds__(256) tkey_kernel(const int32_t* __restrict__ labels, const int32_t* n_dev, int n_max,
                                                   u64* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int n = live_n(n_dev, n_max);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int32_t l = labels[i];
    keys[i] = l >= 0 ? (u64)l : NO_LABEL;
    vals[i] = (uint32_t)i;
  }
}

// rows of the table while it accumulates: slot 0 unused, 1 unused, 2..7 order-preserving keys of
// x min, x max, z min, z max, y min, y max, 8..10 the sums, 11 the spare
__global__ void __launch_bounds__(256) tinit_kernel(const int32_t* ncl, int max_clusters, double* __restrict__ table) {
  const int k = table_rows(ncl, max_clusters);
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < k; c += (long long)gridDim.x * 256) {
    u64* row = (u64*)(table + 12 * c);
    row[0] = row[1] = 0;
    for (int a = 0; a < 3; ++a) { row[2 + 2 * a] = ~0ull; row[3 + 2 * a] = 0; }
    for (int a = 8; a < 12; ++a) table[12 * c + a] = 0.0;
  }
}

__global__ void __launch_bounds__(256) toffsets_kernel(const u64* __restrict__ keys, const int32_t* n_dev, int n_max,
                                                       const int32_t* ncl, int max_clusters, int32_t* __restrict__ offsets) {
  const int n = live_n(n_dev, n_max), k = table_rows(ncl, max_clusters);
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c <= k; c += (long long)gridDim.x * 256)
    offsets[c] = lower_bound(keys, n, (u64)c);
}

// One set of atomics per distinct cluster in the wave (the rows are sorted by cluster, so that is
// one set for almost every wave): min / max through the order-preserving keys, sums reduced over
// the wave's lanes first.
__global__ void __launch_bounds__(256) taccum_kernel(const double* __restrict__ pts, const u64* __restrict__ keys,
                                                     const uint32_t* __restrict__ idx, const int32_t* n_dev, int n_max,
                                                     const int32_t* ncl, int max_clusters, double* table,
                                                     uint32_t* __restrict__ order) {
  const int n = live_n(n_dev, n_max), k = table_rows(ncl, max_clusters), lane = threadIdx.x & 63;
  for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
    const long long t = base + threadIdx.x;
    long long c = -1;
    double v[3] = {0.0, 0.0, 0.0};
    if (t < n) {
      const u64 key = keys[t];
      if (key < NO_LABEL) {
        const size_t i = row_of(idx[t], n);
        order[t] = (uint32_t)i;
        if (key < (u64)k) {
          c = (long long)key;
          v[0] = pts[3 * i]; v[1] = pts[3 * i + 2]; v[2] = pts[3 * i + 1];      // x, z, y: the table's bound order
        }
      }
    }
    u64 todo = __ballot(c >= 0);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const long long lc = __shfl(c, leader);
      const bool mine = c == lc;
      u64 mn[3], mx[3];
      double s[3];
      #pragma unroll
      for (int a = 0; a < 3; ++a) {
        mn[a] = mine ? okey(v[a]) : ~0ull;
        mx[a] = mine ? okey(v[a]) : 0ull;
        s[a] = mine ? v[a] : 0.0;
      }
      #pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        #pragma unroll
        for (int a = 0; a < 3; ++a) {
          const u64 t0 = __shfl_xor(mn[a], o), t1 = __shfl_xor(mx[a], o);
          mn[a] = t0 < mn[a] ? t0 : mn[a];
          mx[a] = t1 > mx[a] ? t1 : mx[a];
          s[a] += __shfl_xor(s[a], o);
        }
      }
      if (lane == leader) {
        u64* row = (u64*)(table + 12 * lc);
        flush_minmax(row + 2, mn, mx);
        atomicAdd(&table[12 * lc + 8], s[0]);                    // sums: x, y, z
        atomicAdd(&table[12 * lc + 9], s[2]);
        atomicAdd(&table[12 * lc + 10], s[1]);
      }
      todo &= ~__ballot(mine);
    }
  }
}

__global__ void __launch_bounds__(256) tfinal_kernel(const int32_t* ncl, int max_clusters, int n_max, const CHdr* h,
                                                     const uint32_t* __restrict__ roots,
                                                     const int32_t* __restrict__ offsets, double* __restrict__ table) {
  const int k = table_rows(ncl, max_clusters);
  const bool known = h->magic == MAGIC && h->stamp_n == (uint32_t)n_max;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < k; c += (long long)gridDim.x * 256) {
    double* row = table + 12 * c;
    for (int a = 2; a < 8; ++a) row[a] = unkey((u64)__double_as_longlong(row[a]));
    row[0] = (double)(offsets[c + 1] - offsets[c]);
    row[1] = known && c < (long long)h->ctr[C_NCL] ? (double)roots[c] : -1.0;
  }
}


// ---- workspace ----------------------------------------------------------------------------------
struct Ws {
  CHdr* h;
  uint32_t* roots;      // cluster number -> its smallest core row; with h, what dp_cluster_table reads
  void* sortws;
  int64_t sort_bytes;
  u64* keys;
  uint32_t *vals, *cbeg, *cend, *parent, *rank, *bc;
  double *sx, *sz;
  uint8_t *part, *core, *rootf;
};
int64_t ws_bytes_for(int64_t n_max) {
  const int64_t n = n_max < 0 ? 0 : n_max;
  return al256(sizeof(CHdr)) + al256(dp_clean_workspace_size(n)) + al256(8 * n) + 2 * al256(8 * n) + 6 * al256(4 * n) +
         al256(4 * scan_blocks_for(n)) + 3 * al256(n) + 256;
}
bool ws_carve(void* ws, int64_t bytes, int n_max, Ws* o) {
  if (!ws || bytes < ws_bytes_for(n_max) || ((uintptr_t)ws & 7)) return false;
  const int64_t n = n_max;
  char* p = (char*)ws;
  o->h = (CHdr*)p;            p += al256(sizeof(CHdr));
  o->roots = (uint32_t*)p;    p += al256(4 * n);
  o->sort_bytes = dp_clean_workspace_size(n);
  o->sortws = p;              p += al256(o->sort_bytes);
  o->keys = (u64*)p;          p += al256(8 * n);
  o->sx = (double*)p;         p += al256(8 * n);
  o->sz = (double*)p;         p += al256(8 * n);
  o->vals = (uint32_t*)p;     p += al256(4 * n);
  o->cbeg = (uint32_t*)p;     p += al256(4 * n);
  o->cend = (uint32_t*)p;     p += al256(4 * n);
  o->parent = (uint32_t*)p;   p += al256(4 * n);
  o->rank = (uint32_t*)p;     p += al256(4 * n);
  o->bc = (uint32_t*)p;       p += al256(4 * scan_blocks_for(n));
  o->part = (uint8_t*)p;      p += al256(n);
  o->core = (uint8_t*)p;      p += al256(n);
  o->rootf = (uint8_t*)p;
  return true;
}

// exclusive scan of f (bytes, row order) into out, the total into *tot
void run_scan(hipStream_t s, const Ws& w, const uint8_t* f, const int32_t* n_dev, int n_max, uint32_t* out, uint32_t* tot) {
  const int nb = (int)scan_blocks_for(n_max);
  if (nb) hipLaunchKernelGGL(scan_count_kernel, dim3(nb), dim3(256), 0, s, f, n_dev, n_max, w.bc);
  hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(256), 0, s, w.bc, nb, tot);
  if (nb) hipLaunchKernelGGL(scan_write_kernel, dim3(nb), dim3(256), 0, s, f, n_dev, n_max, w.bc, out);
}
}  // namespace

extern "C" int64_t dp_cluster_workspace_size(int64_t n_max) { return ws_bytes_for(n_max); }

extern "C" int dp_cluster_dbscan(const double* points, const int32_t* n_dev, int32_t n_max, double eps,
                                 int32_t min_samples, double height_threshold, int32_t max_points, int32_t* labels_out,
                                 int32_t* n_clusters_dev, double* stats_out, void* workspace, int64_t workspace_bytes,
                                 dp_stream_t stream) {
  if (!stats_out || !n_clusters_dev || (n_max > 0 && (!points || !labels_out))) return DP_ERR_ARG;
  if (n_max < 0 || min_samples < 1 || max_points < 0 || !(eps > 0.0) || !(eps < __builtin_inf())) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, n_max, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int g = grid_for(n_max, GRID_CAP);
  const double eps2 = eps * eps;
  (void)hipMemsetAsync(w.h, 0, sizeof(CHdr), s);
  hipLaunchKernelGGL(hdr_init_kernel, dim3(1), dim3(1), 0, s, w.h);
  hipLaunchKernelGGL(elig_kernel, dim3(g), dim3(256), 0, s, points, n_dev, n_max, height_threshold, w.h, w.part);
  run_scan(s, w, w.part, n_dev, n_max, w.rank, &w.h->ctr[C_ELIG]);
  hipLaunchKernelGGL(part_kernel, dim3(g), dim3(256), 0, s, points, n_dev, n_max, max_points, w.rank, w.h, w.part,
                     labels_out, w.parent, w.rootf);
  hipLaunchKernelGGL(setup_kernel, dim3(1), dim3(1), 0, s, w.h, eps);
  hipLaunchKernelGGL(key_kernel, dim3(g), dim3(256), 0, s, points, n_dev, n_max, w.h, w.part, w.keys, w.vals);
  const int rc = dp_sort_pairs((uint64_t*)w.keys, w.vals, n_dev, n_max, 0, 2 * CELL_BITS + 1, w.sortws, w.sort_bytes, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(cells_kernel, dim3(g), dim3(256), 0, s, points, w.keys, w.vals, n_dev, n_max, w.h, w.sx, w.sz, w.cbeg,
                     w.cend);
  hipLaunchKernelGGL(core_kernel, dim3(g), dim3(256), 0, s, w.keys, w.sx, w.sz, w.cbeg, w.cend, eps2, min_samples, w.h,
                     w.core);
  hipLaunchKernelGGL(union_kernel, dim3(g), dim3(256), 0, s, w.keys, w.vals, w.sx, w.sz, w.cbeg, w.cend, w.core, eps2,
                     min_samples, w.h, n_max, w.parent);
  hipLaunchKernelGGL(compress_kernel, dim3(g), dim3(256), 0, s, w.vals, w.core, w.h, n_max, w.parent, w.rootf);
  run_scan(s, w, w.rootf, n_dev, n_max, w.rank, &w.h->ctr[C_NCL]);
  hipLaunchKernelGGL(label_kernel, dim3(g), dim3(256), 0, s, w.keys, w.vals, w.sx, w.sz, w.cbeg, w.cend, w.core, w.parent,
                     w.rank, eps2, min_samples, w.h, n_max, labels_out, w.roots);
  hipLaunchKernelGGL(final_kernel, dim3(1), dim3(1), 0, s, w.h, n_max, n_clusters_dev, stats_out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_cluster_table(const double* points, const int32_t* labels, const int32_t* n_dev, int32_t n_max,
                                const int32_t* n_clusters_dev, int32_t max_clusters, double* table_out,
                                uint32_t* order_out, int32_t* offsets_out, void* workspace, int64_t workspace_bytes,
                                dp_stream_t stream) {
  if (!n_clusters_dev || !offsets_out || (max_clusters > 0 && !table_out) ||
      (n_max > 0 && (!points || !labels || !order_out)))
    return DP_ERR_ARG;
  if (n_max < 0 || max_clusters < 0) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, n_max, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int g = grid_for(n_max, GRID_CAP), gc = grid_for((int64_t)max_clusters + 1, GRID_CAP);
  hipLaunchKernelGGL(tkey_kernel, dim3(g), dim3(256), 0, s, labels, n_dev, n_max, w.keys, w.vals);
  const int rc = dp_sort_pairs((uint64_t*)w.keys, w.vals, n_dev, n_max, 0, 33, w.sortws, w.sort_bytes, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(tinit_kernel, dim3(gc), dim3(256), 0, s, n_clusters_dev, max_clusters, table_out);
  hipLaunchKernelGGL(toffsets_kernel, dim3(gc), dim3(256), 0, s, w.keys, n_dev, n_max, n_clusters_dev, max_clusters,
                     offsets_out);
  hipLaunchKernelGGL(taccum_kernel, dim3(g), dim3(256), 0, s, points, w.keys, w.vals, n_dev, n_max, n_clusters_dev,
                     max_clusters, table_out, order_out);
  hipLaunchKernelGGL(tfinal_kernel, dim3(gc), dim3(256), 0, s, n_clusters_dev, max_clusters, n_max, w.h, w.roots, offsets_out,
                     table_out);
  DP_CHECK_LAUNCH();
  return 0;
}
