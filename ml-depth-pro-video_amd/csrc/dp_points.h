// What the point-cloud stages share (dp_ground.hip, dp_clean.hip, dp_cluster.hip, dp_shapes.hip,
// dp_normals.hip, dp_floorplan.hip): one
// copy of every device and host helper that two or more of them use.  A helper with one user stays in
// its file.  Everything is in an anonymous namespace, so each translation unit has its own copy of the
// two kernels below.
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
// workgroups of 256 threads for n elements in a grid-stride loop: at least one, at most cap
int grid_for(int64_t n, int cap) {
  const int64_t g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace
