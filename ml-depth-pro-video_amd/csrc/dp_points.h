// What the point-cloud stages share (dp_ground.hip, dp_clean.hip, dp_cluster.hip, dp_shapes.hip,
// dp_normals.hip, dp_floorplan.hip, dp_lshape.hip, dp_mesh.hip, dp_outline.hip, dp_slices.hip): one
// copy of every device and host helper that two or more of them use.  A helper with one user stays in
// its file.  Everything is in an anonymous namespace, so each translation unit has its own copy of the
// two kernels below.  The sorted 3-D cell grid of dp_clean.hip, dp_normals.hip and dp_mesh.hip, kernels
// included, is in dp_grid3.h, which includes this header and which only those three include; the 2-D grids
// of dp_floorplan.hip and dp_slices.hip are in dp_grid2.h in the same way.
// Floating-point contraction: every stage compiles with `#pragma clang fp contract(off)`, and the header
// sets it as well, so the helpers are built as they were inside the stages wherever the include stands.
// It is a header for files that want contraction off; cell_of (a subtraction feeding a division) has
// nothing to contract in any case.
#pragma once
#include "dp_common.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = 256 * SCAN_ITEMS;     // rows of one workgroup (flag scans, compaction)

// fp64 -> order-preserving u64 (-0.0 folded onto +0.0) and back
__device__ __forceinline__ u64 okey(double x) {
  u64 b = (u64)__double_as_longlong(x);
  if (x == 0.0) b = 0;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double unkey(u64 k) {
  const u64 b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}
// float32 -> order-preserving 32 bits (-0.0 folded onto +0.0) and back
__device__ __forceinline__ uint32_t okey32(float v) {
  uint32_t b = __float_as_uint(v);
  if (v == 0.0f) b = 0;
  return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float unkey32(uint32_t k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }

// ---- floor-plan grids (dp_floorplan.hip and dp_slices.hip through dp_grid2.h, dp_outline.hip) -------
// H, W as every stage behind the raster reads them: anything outside [0, DP_FLOOR_MAX_DIM] or beyond the
// capacity is no grid
__device__ __forceinline__ void grid_dims(const int32_t* dims, int max_cells, int& H, int& W) {
  H = dims[0]; W = dims[1];
  if (H < 0 || W < 0 || H > DP_FLOOR_MAX_DIM || W > DP_FLOOR_MAX_DIM || (long long)H * W > max_cells) { H = 0; W = 0; }
}

__device__ __forceinline__ bool fin(double v) { return __builtin_fabs(v) < __builtin_inf(); }   // false for NaN, +-inf
__device__ __forceinline__ bool finite3(double x, double y, double z) { return fin(x) && fin(y) && fin(z); }

__device__ __forceinline__ int live_n(const int32_t* n_dev, int n_max) {
  int n = n_dev ? *n_dev : n_max;
  n = n < 0 ? 0 : n;
  return n < n_max ? n : n_max;
}
__device__ __forceinline__ int table_rows(const int32_t* ncl, int max_clusters) {
  int k = *ncl;
  k = k < 0 ? 0 : k;
  return k < max_clusters ? k : max_clusters;
}
__device__ __forceinline__ void wave_count(uint32_t* c, bool p) {
  const u64 m = __ballot(p);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(c, (uint32_t)__popcll(m));
}
// A payload of the sort is a row index below n by construction; the clamp only keeps a read inside
// the array whatever the buffers hold.  A row index: widen it to size_t before multiplying by 3.
__device__ __forceinline__ uint32_t row_of(uint32_t v, int n) { return v < (uint32_t)n ? v : (uint32_t)(n - 1); }

// exclusive scan over the 256 threads of the workgroup (wsum: 4 shared words).  The second barrier
// lets the caller use wsum again at once.
template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* wsum, T* total = nullptr) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T inc = v;
  #pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  T pre = 0, tot = 0;
  for (int k = 0; k < 4; ++k) {
    const T s = wsum[k];
    if (k < w) pre += s;
    tot += s;
  }
  __syncthreads();
  if (total) *total = tot;
  return pre + inc - v;
}

// first position in keys[0, n) with keys[pos] >= k
__device__ __forceinline__ int lower_bound(const u64* __restrict__ keys, int n, u64 k) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// grid cell of a coordinate, clamped to [0, CELL_MAX] (each stage's own largest cell coordinate)
template <int CELL_MAX>
__device__ __forceinline__ u64 cell_of(double v, double mn, double edge) {
  const double q = __builtin_floor((v - mn) / edge);
  return (u64)(q < 0.0 ? 0.0 : (q > (double)CELL_MAX ? (double)CELL_MAX : q));
}

// A pairs of (smallest, largest) order-preserving keys.  wave_minmax is one butterfly step of their
// reduction over the wave: after o = 32, 16, ..., 1 every lane holds the result.  It is a step so that
// a kernel's counters ride in the same unrolled loop.  flush_minmax issues one atomicMin / atomicMax
// pair each into dst[2a], dst[2a + 1].
template <int A>
__device__ __forceinline__ void wave_minmax(u64 (&mn)[A], u64 (&mx)[A], int o) {
  #pragma unroll
  for (int a = 0; a < A; ++a) {
    const u64 t0 = __shfl_xor(mn[a], o), t1 = __shfl_xor(mx[a], o);
    mn[a] = t0 < mn[a] ? t0 : mn[a];
    mx[a] = t1 > mx[a] ? t1 : mx[a];
  }
}
template <int A>
__device__ __forceinline__ void flush_minmax(u64* dst, const u64 (&mn)[A], const u64 (&mx)[A]) {
  for (int a = 0; a < A; ++a) { atomicMin(&dst[2 * a], mn[a]); atomicMax(&dst[2 * a + 1], mx[a]); }
}

// ---- lock-free union-find over 32-bit indices (cluster rows, grid cells) ---------------------------
// parent[i] <= i always: a root is only ever hooked under a smaller root (CAS on the root's own
// word), and path halving only lowers a word to one of its ancestors (atomicMin).  So there are no
// cycles, a find terminates, and when all unions are done every root is its set's smallest row.
__device__ __forceinline__ uint32_t ld(const uint32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ uint32_t uf_find(uint32_t* p, uint32_t i) {
  uint32_t q = ld(&p[i]);
  while (q != i) {
    const uint32_t g = ld(&p[q]);
    if (g != q) atomicMin(&p[i], g);
    i = q;
    q = g;
  }
  return i;
}
__device__ __forceinline__ void uf_unite(uint32_t* p, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find(p, a);
    b = uf_find(p, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    if (atomicCAS(&p[a], a, b) == a) return;                     // lost: someone else hooked a; find again
  }
}

// number of entries of a[0, n) that are <= v (a ascending)
__device__ __forceinline__ int upper_bound(const int32_t* __restrict__ a, int n, int v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- convex hull and minimum-area rectangle of one chunk in LDS: rules 2 and 3 of "Cluster shapes" ----
// For a workgroup of HULL_NT threads (dp_shapes.hip's hull chunks, dp_lshape.hip's occupied components).
// The caller loads P slots (P a power of two >= m, at most HULL_MAX): m members with st < HULL_PAD and
// st distinct, the rest st = HULL_PAD, in any order, and passes a barrier.
constexpr int HULL_NT = 256;
constexpr int HULL_MAX = DP_SHAPES_H_MAX;
constexpr uint32_t HULL_PAD = 0xffffffffu;     // the sort's filler: after every member
constexpr double HULL_DEG = 57.29577951308232; // 180 / pi

struct HullLds {
  double su[HULL_MAX], sv[HULL_MAX];
  uint32_t st[HULL_MAX];
  int lo[HULL_MAX], up[HULL_MAX];
};

// o(a, b, c) of the header: > 0 for a left turn
__device__ __forceinline__ double orient(double au, double av, double bu, double bv, double cu, double cv) {
  return (bu - au) * (cv - av) - (bv - av) * (cu - au);
}

__device__ __forceinline__ bool hull_before(const HullLds& s, int x, int y) {
  const uint32_t tx = s.st[x], ty = s.st[y];
  if (tx == HULL_PAD) return false;
  if (ty == HULL_PAD) return true;
  const double ux = s.su[x], uy = s.su[y];
  if (ux != uy) return ux < uy;
  const double vx = s.sv[x], vy = s.sv[y];
  if (vx != vy) return vx < vy;
  return tx < ty;
}

// Bitonic sort by (u, v, st), then the monotone chain: the lower hull left to right on wave 0, the
// upper hull right to left on wave 1.  Only the first of a run of coincident members takes part; a
// point leaves the stack unless it is a strict left turn.  Returns the number of vertices; vertex e
// (counter-clockwise from the smallest (u, v)) is slot hull_vertex(s, kl, e).  cnt: 2 shared ints.
__device__ __forceinline__ int hull_sort_chain(HullLds& s, int m, int P, int* cnt, int* kl_out) {
  const int tid = threadIdx.x;
  for (int kk = 2; kk <= P; kk <<= 1)
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
      for (int i = tid; i < (P >> 1); i += HULL_NT) {
        const int a = 2 * jj * (i / jj) + (i % jj), z = a + jj;
        const bool asc = (a & kk) == 0;
        if (asc ? hull_before(s, z, a) : hull_before(s, a, z)) {
          const double tu = s.su[a], tv = s.sv[a];
          const uint32_t tt = s.st[a];
          s.su[a] = s.su[z]; s.sv[a] = s.sv[z]; s.st[a] = s.st[z];
          s.su[z] = tu; s.sv[z] = tv; s.st[z] = tt;
        }
      }
      __syncthreads();
    }
  if (tid == 0 || tid == 64) {
    int* stack = tid == 0 ? s.lo : s.up;
    int top = 0;
    for (int step = 0; step < m; ++step) {
      const int i = tid == 0 ? step : m - 1 - step;
      const double cu = s.su[i], cv = s.sv[i];
      if (i > 0 && s.su[i - 1] == cu && s.sv[i - 1] == cv) continue;
      while (top >= 2) {
        const int p1 = stack[top - 1], p0 = stack[top - 2];
        if (orient(s.su[p0], s.sv[p0], s.su[p1], s.sv[p1], cu, cv) > 0.0) break;
        --top;
      }
      stack[top++] = i;
    }
    cnt[tid == 0 ? 0 : 1] = top;
  }
  __syncthreads();
  const int kl = cnt[0], ku = cnt[1];
  *kl_out = kl;
  return kl <= 1 ? kl : (kl - 1) + (ku - 1);
}
__device__ __forceinline__ int hull_vertex(const HullLds& s, int kl, int e) {
  return e < kl - 1 || kl <= 1 ? s.lo[e] : s.up[e - (kl - 1)];
}

// Rule 3 over the hn vertices at the front of s.su / s.sv (the caller has moved them there and passed
// a barrier; the stacks are free): one edge per lane, the extents of every vertex along e and n, the
// smallest area with ties to the smallest edge.  One thread writes out[0..6) = centre u, centre v,
// width, height, angle, area; hn < 2: a 0 x 0 rectangle at the first vertex.  No barrier after the write.
__device__ __forceinline__ void hull_min_rect(HullLds& s, int hn, double* out) {
  const int tid = threadIdx.x;
  double best = __builtin_inf();
  int besti = 0x7fffffff;
  double bw = 0.0, bh = 0.0, bcu = 0.0, bcv = 0.0, beu = 1.0, bev = 0.0;
  if (hn >= 2) {
    for (int i = tid; i < hn; i += HULL_NT) {
      const int i1 = i + 1 < hn ? i + 1 : 0;
      const double du = s.su[i1] - s.su[i], dv = s.sv[i1] - s.sv[i];
      const double len = __builtin_sqrt(du * du + dv * dv);
      const double eu = du / len, ev = dv / len;
      double pmn = __builtin_inf(), pmx = -__builtin_inf(), qmn = __builtin_inf(), qmx = -__builtin_inf();
      for (int v = 0; v < hn; ++v) {
        const double u_ = s.su[v], v_ = s.sv[v];
        const double p = u_ * eu + v_ * ev, q = v_ * eu - u_ * ev;
        pmn = p < pmn ? p : pmn; pmx = p > pmx ? p : pmx;
        qmn = q < qmn ? q : qmn; qmx = q > qmx ? q : qmx;
      }
      const double w = pmx - pmn, hh = qmx - qmn, a = w * hh;
      if (a < best) {                                            // a lane's edges come in increasing i
        best = a; besti = i; bw = w; bh = hh; beu = eu; bev = ev;
        const double pc = (pmn + pmx) / 2.0, qc = (qmn + qmx) / 2.0;
        bcu = eu * pc - ev * qc;
        bcv = ev * pc + eu * qc;
      }
    }
  }
  double* ra = (double*)s.lo;
  int* ri = s.up;
  ra[tid] = best;
  ri[tid] = besti;
  __syncthreads();
  for (int o = HULL_NT / 2; o > 0; o >>= 1) {
    if (tid < o) {
      const double a2 = ra[tid + o];
      const int i2 = ri[tid + o];
      if (a2 < ra[tid] || (a2 == ra[tid] && i2 < ri[tid])) { ra[tid] = a2; ri[tid] = i2; }
    }
    __syncthreads();
  }
  const int win = ri[0];
  if (tid == 0 && (hn < 2 || win == 0x7fffffff)) {               // one vertex (or nothing comparable): 0 x 0 at p0
    out[0] = s.su[0]; out[1] = s.sv[0];
    out[2] = out[3] = out[4] = out[5] = 0.0;
  }
  if (hn >= 2 && win != 0x7fffffff && besti == win) {
    double ang = atan2(bev, beu) * HULL_DEG;
    double kq = __builtin_floor(ang / 90.0);
    ang = ang - 90.0 * kq;
    if (ang >= 90.0) { ang = 0.0; kq = kq + 1.0; }               // a tiny negative angle rounds up to 90
    const bool swap = __builtin_fmod(kq, 2.0) != 0.0;
    out[0] = bcu; out[1] = bcv;
    out[2] = swap ? bh : bw;
    out[3] = swap ? bw : bh;
    out[4] = ang;
    out[5] = best;
  }
}

// ---- exclusive scan of a byte flag in row order: per-tile counts, then one workgroup turns them into
// offsets.  The third step (ranks, or moving rows) is the caller's.
__global__ void __launch_bounds__(256) scan_count_kernel(const uint8_t* __restrict__ f, const int32_t* n_dev, int n_max,
                                                         uint32_t* __restrict__ bc) {
  __shared__ uint32_t wsum[4];
  const int n = live_n(n_dev, n_max);
  const long long tile = (long long)blockIdx.x * SCAN_TILE;
  uint32_t c = 0;
  for (int r = 0; r < SCAN_ITEMS; ++r) {
    const long long i = tile + r * 256 + threadIdx.x;
    c += i < n && f[i];
  }
  uint32_t tot = 0;
  block_excl_scan(c, wsum, &tot);
  if (threadIdx.x == 0) bc[blockIdx.x] = tot;
}

// one workgroup: block counts -> exclusive offsets, total -> *tot_out
__global__ void __launch_bounds__(256) scan_blocks_kernel(uint32_t* __restrict__ bc, int nblocks, uint32_t* tot_out) {
  __shared__ uint32_t wsum[4];
  const int per = (nblocks + 255) / 256;
  const long long b0 = (long long)threadIdx.x * per;
  const long long b1 = b0 + per < nblocks ? b0 + per : nblocks;
  uint32_t s = 0, tot = 0;
  for (long long b = b0; b < b1; ++b) s += bc[b];
  uint32_t run = block_excl_scan(s, wsum, &tot);
  for (long long b = b0; b < b1; ++b) {
    const uint32_t t = bc[b];
    bc[b] = run;
    run += t;
  }
  if (threadIdx.x == 0) *tot_out = tot;
}

// ---- host ----------------------------------------------------------------------------------------
int64_t al256(int64_t b) { return (b + 255) / 256 * 256; }
// workgroups of the flag scan (tiles of SCAN_TILE rows) for n rows
int64_t scan_blocks_for(int64_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }
// workgroups of 256 threads for n elements in a grid-stride loop: at least one, at most cap
int grid_for(int64_t n, int cap) {
  const int64_t g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace
