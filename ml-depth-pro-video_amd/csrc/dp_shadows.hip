// Depth-discontinuity shadow mask: find_depth_shadows (:1110-1170) and the ground fill of remove_depth_shadows
// (:1857-1944) of the reference's OLD_SCRIPTS/mesh_from_depth.py, in image space, on the GPU.  The rules are in
// include/dp_mi355x.h ("Depth shadows") and restated in tests/shadows_numpy.py.
//
// Gradient: scipy.ndimage.sobel on float32 is two 1-D passes, each accumulated in fp64 in scipy's order (the centre
// tap times its weight first, then (left -+ right) * weight) and rounded to float32 once.  A thread recomputes the
// three pass-1 values of each direction from its 3 x 3 neighbourhood (9 loads that the vector L1 serves) and rounds
// each to float32 before pass 2.  Contraction is off for the whole file: dx * dx + dy * dy is three roundings.
//
// Regions: a 4-connected labeller that produces sizes, not a numbering.
//   1. sh_tile_kernel: one workgroup per 64 x 64 tile, one wave per row of 64 pixels (16 rows per wave).  The runs of
//      a row come from one ballot (a pixel's provisional label is its run's first pixel); rows are joined where a run
//      of one overlaps a run of the row above, one union per overlap, in an LDS union-find (atomicMin links the larger
//      root to the smaller).  The tile's components are counted in LDS, lanes with the same root electing one adder.
//      Out: labels[p] = global index of p's tile-local root (-1: not free), sizes[root] = the tile-local count.
//   2. sh_border_kernel: one thread per pixel pair across a tile border, the same union in global memory.  A pair
//      whose left (upper) neighbour pair in the same two tiles is also free is skipped: it joins the same two roots.
//   3. sh_flatten_kernel: every tile-local root finds its global root, points at it, and adds its count to it: one
//      global atomic per tile-local component, not per pixel or per wave.
//   4. sh_mask_kernel: shadow = not free, or sizes[root] < min_region_size; the counts of the statistics.
// A stage boundary is a kernel boundary; no workgroup waits on another; nothing is read back.
#include "dp_common.h"

#pragma clang fp contract(off)      // every product and sum below is rounded on its own

namespace {

constexpr int TILE = 64;
constexpr int ROWS_PER_WAVE = TILE / 4;
constexpr int64_t HDR_BYTES = 256;
constexpr int MAX_BLOCKS = 2048;

// workspace header: six 64-bit counters, then two 32-bit words
enum { C_EDGE = 0, C_SHADOW, C_COMP, C_KEPT, C_NONFINITE, C_NONPOS, C_COUNT };
struct Header {
  unsigned long long cnt[8];
  uint32_t gmax_bits;       // the gradient's maximum, as the bit pattern of a non-negative float
  uint32_t largest;         // pixels of the largest free component
};

inline int64_t align256(int64_t b) { return (b + 255) & ~(int64_t)255; }

struct Layout {
  int64_t labels, sizes, grad, free_, total;
};
inline Layout layout(int64_t n) {
  Layout l;
  l.labels = HDR_BYTES;
  l.sizes = l.labels + align256(4 * n);
  l.grad = l.sizes + align256(4 * n);
  l.free_ = l.grad + align256(4 * n);
  l.total = l.free_ + align256(n);
  return l;
}

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__global__ void sh_init_kernel(Header* __restrict__ hd) {
  if (threadIdx.x < 8) hd->cnt[threadIdx.x] = 0ull;
  if (threadIdx.x == 8) hd->gmax_bits = 0u;
  if (threadIdx.x == 9) hd->largest = 0u;
}

// the workgroup's sum of v added to *dst by one thread (nothing when the sum is 0); every thread of a 256-thread
// workgroup calls it
__device__ __forceinline__ void block_add(unsigned long long* dst, int v, int* red) {
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int s = red[0] + red[1] + red[2] + red[3];
    if (s) atomicAdd(dst, (unsigned long long)s);
  }
}
__device__ __forceinline__ void block_max(uint32_t* dst, uint32_t v, int* red) {
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t t = __shfl_xor(v, o);
    v = t > v ? t : v;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = (int)v;
  __syncthreads();
  if (threadIdx.x == 0) {
    #pragma unroll
    for (int k = 1; k < 4; ++k) v = (uint32_t)red[k] > v ? (uint32_t)red[k] : v;
    if (v) atomicMax(dst, v);
  }
}

// scipy's correlate1d on three taps, fp64 accumulation in its order, one rounding to float32
__device__ __forceinline__ float deriv3(float l, float c, float r) {      // weights [-1, 0, 1]
  double t = (double)c * 0.0;
  t += ((double)l - (double)r) * -1.0;
  return (float)t;
}
__device__ __forceinline__ float smooth3(float l, float c, float r) {     // weights [1, 2, 1]
  double t = (double)c * 2.0;
  t += ((double)l + (double)r) * 1.0;
  return (float)t;
}

__global__ void __launch_bounds__(256) sh_gradient_kernel(const float* __restrict__ d, int h, int w, float* __restrict__ g,
                                                          Header* __restrict__ hd) {
  __shared__ int red[4];
  const long long n = (long long)h * w;
  uint32_t gmax = 0u;
  int bad = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int y = (int)((uint32_t)i / (uint32_t)w), x = (int)(i - (long long)y * w);      // h * w < 2^31
    const int xs[3] = {x > 0 ? x - 1 : 0, x, x + 1 < w ? x + 1 : w - 1};       // mode='reflect': the edge sample again
    const int ys[3] = {y > 0 ? y - 1 : 0, y, y + 1 < h ? y + 1 : h - 1};
    float v[3][3];
    #pragma unroll
    for (int r = 0; r < 3; ++r) {
      #pragma unroll
      for (int c = 0; c < 3; ++c) v[r][c] = d[(long long)ys[r] * w + xs[c]];
    }
    // sobel(axis=1): derivative along x on each row, then smoothing along y; sobel(axis=0): the other way round
    const float dx = smooth3(deriv3(v[0][0], v[0][1], v[0][2]), deriv3(v[1][0], v[1][1], v[1][2]), deriv3(v[2][0], v[2][1], v[2][2]));
    const float dy = smooth3(deriv3(v[0][0], v[1][0], v[2][0]), deriv3(v[0][1], v[1][1], v[2][1]), deriv3(v[0][2], v[1][2], v[2][2]));
    const float xx = dx * dx, yy = dy * dy;
    const float ss = xx + yy;
    const float m = sqrtf(ss);                                                    // correctly rounded (no fast-math flags)
    g[i] = m;
    const uint32_t mb = __float_as_uint(m);
    gmax = mb > gmax ? mb : gmax;
    bad += finite_f(v[1][1]) ? 0 : 1;
  }
  block_max(&hd->gmax_bits, gmax, red);
  block_add(&hd->cnt[C_NONFINITE], bad, red);
}

// edge = (gmax > 0 ? g / gmax : g) > thr, in float32; a frame with a non-finite depth has no edges.  Writes 1 for an
// edge (invert = 0) or 1 for a free pixel (invert = 1).
__global__ void __launch_bounds__(256) sh_edge_kernel(const float* __restrict__ g, long long n, float thr, int invert,
                                                      uint8_t* __restrict__ out, Header* __restrict__ hd) {
  __shared__ int red[4];
  const float gmax = __uint_as_float(hd->gmax_bits);
  const bool none = hd->cnt[C_NONFINITE] != 0ull;
  int edges = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float v = g[i];
    const float q = gmax > 0.f ? __fdiv_rn(v, gmax) : v;
    const bool e = !none && q > thr;
    edges += e ? 1 : 0;
    out[i] = (uint8_t)((e ? 1 : 0) ^ invert);
  }
  block_add(&hd->cnt[C_EDGE], edges, red);
}

// ---- union-find: parent[i] <= i always; atomicMin links the larger of two roots to the smaller ----

template <bool LDS>
__device__ __forceinline__ int uf_load(const int* p) {
  if constexpr (LDS) return *(const volatile int*)p;
  else return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool LDS>
__device__ __forceinline__ int uf_find(const int* parent, int i) {
  int p;
  while ((p = uf_load<LDS>(parent + i)) != i) i = p;                  // strictly decreasing: ends
  return i;
}
template <bool LDS>
__device__ __forceinline__ void uf_union(int* parent, int a, int b) {
  a = uf_find<LDS>(parent, a);
  b = uf_find<LDS>(parent, b);
  while (a != b) {                                                    // a + b falls in every round
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(parent + a, b);
    if (old == a) break;                                              // a was a root and now points at b
    a = old;                                                          // a had a parent: that one joins b
  }
}

// adds 1 to cnt[root] for every lane with root >= 0; lanes of the wave that share a root elect one adder (three
// rounds, then each lane that is left adds for itself).  The whole wave calls it.
__device__ __forceinline__ void wave_count(int* cnt, int root, int lane) {
  bool act = root >= 0;
  #pragma unroll 1
  for (int round = 0; round < 3; ++round) {
    const unsigned long long rem = __ballot(act);
    if (rem == 0ull) return;
    const int leader = __ffsll((long long)rem) - 1;
    const int lr = __shfl(root, leader);
    const bool same = act && root == lr;
    const unsigned long long m = __ballot(same);
    if (lane == leader) atomicAdd(cnt + lr, __popcll(m));
    if (same) act = false;
  }
  if (act) atomicAdd(cnt + root, 1);
}

__global__ void __launch_bounds__(256) sh_tile_kernel(const uint8_t* __restrict__ free_, int h, int w, int tiles_x,
                                                      int* __restrict__ labels, int* __restrict__ sizes) {
  __shared__ int parent[TILE * TILE];
  __shared__ int cnt[TILE * TILE];
  __shared__ unsigned long long bits[TILE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int tx0 = ((int)blockIdx.x % tiles_x) * TILE, ty0 = ((int)blockIdx.x / tiles_x) * TILE;
  const int x = tx0 + lane;
  // 1. runs of every row: a free pixel starts at its run's first pixel
  #pragma unroll 1
  for (int k = 0; k < ROWS_PER_WAVE; ++k) {
    const int r = wv * ROWS_PER_WAVE + k, y = ty0 + r;
    const bool f = x < w && y < h && free_[(long long)y * w + x] != 0;
    const unsigned long long b = __ballot(f);
    if (lane == 0) bits[r] = b;
    const unsigned long long z = ~b & ((1ull << lane) - 1ull);          // the holes to the left of this lane
    const int start = z ? 64 - __clzll((long long)z) : 0;
    parent[r * TILE + lane] = f ? r * TILE + start : -1;
    cnt[r * TILE + lane] = 0;
  }
  __syncthreads();
  // 2. join with the row above: one union per stretch of columns free in both rows
  #pragma unroll 1
  for (int k = 0; k < ROWS_PER_WAVE; ++k) {
    const int r = wv * ROWS_PER_WAVE + k;
    if (r == 0) continue;
    const unsigned long long m = bits[r] & bits[r - 1];
    const bool first = ((m >> lane) & 1ull) && (lane == 0 || !((m >> (lane - 1)) & 1ull));
    if (first) uf_union<true>(parent, r * TILE + lane, (r - 1) * TILE + lane);
  }
  __syncthreads();
  // 3. roots and the tile-local counts
  int roots[ROWS_PER_WAVE];
  #pragma unroll
  for (int k = 0; k < ROWS_PER_WAVE; ++k) {
    const int idx = (wv * ROWS_PER_WAVE + k) * TILE + lane;
    roots[k] = parent[idx] >= 0 ? uf_find<true>(parent, idx) : -1;
    wave_count(cnt, roots[k], lane);
  }
  __syncthreads();
  // 4. out: the root's global index per pixel, the count at the root's own pixel, 0 elsewhere
  #pragma unroll
  for (int k = 0; k < ROWS_PER_WAVE; ++k) {
    const int r = wv * ROWS_PER_WAVE + k, y = ty0 + r;
    if (x < w && y < h) {
      const long long gi = (long long)y * w + x;
      const int root = roots[k];
      labels[gi] = root < 0 ? -1 : (ty0 + root / TILE) * w + tx0 + root % TILE;
      sizes[gi] = root == r * TILE + lane ? cnt[root] : 0;
    }
  }
}

__global__ void __launch_bounds__(256) sh_border_kernel(int* __restrict__ labels, int h, int w) {
  const long long nh = (long long)((h - 1) / TILE) * w;      // pairs across the horizontal borders y = 64 k
  const long long nv = (long long)((w - 1) / TILE) * h;      // pairs across the vertical borders x = 64 k
  long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= nh + nv) return;
  long long a, b, a2, b2;                                     // the pair, and the pair before it along the border
  bool inner;                                                 // the pair before it lies in the same two tiles
  if (t < nh) {
    const int y = (int)(t / w + 1) * TILE, x = (int)(t % w);
    a = (long long)y * w + x; b = a - w; a2 = a - 1; b2 = b - 1;
    inner = (x % TILE) != 0;
  } else {
    t -= nh;
    const int x = (int)(t / h + 1) * TILE, y = (int)(t % h);
    a = (long long)y * w + x; b = a - 1; a2 = a - w; b2 = b - w;
    inner = (y % TILE) != 0;
  }
  if (labels[a] < 0 || labels[b] < 0) return;                 // (the sign of a label never changes)
  if (inner && labels[a2] >= 0 && labels[b2] >= 0) return;    // that pair joins the same two tile-local components
  uf_union<false>(labels, (int)a, (int)b);
}

__global__ void __launch_bounds__(256) sh_flatten_kernel(int* __restrict__ labels, int* __restrict__ sizes, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int s = sizes[i];
  if (s <= 0) return;                                         // not a tile-local root
  const int r = uf_find<false>(labels, (int)i);
  if (r != (int)i) {                                          // nobody adds to sizes[i]: i is not a global root
    labels[i] = r;
    atomicAdd(sizes + r, s);
  }
}

__global__ void __launch_bounds__(256) sh_mask_kernel(const int* __restrict__ labels, const int* __restrict__ sizes, long long n,
                                                      int min_size, int count_edges, const float* __restrict__ depth,
                                                      uint8_t* __restrict__ mask, float* __restrict__ depth_out,
                                                      Header* __restrict__ hd) {
  __shared__ int red[4];
  int shadow = 0, comp = 0, kept = 0, nonpos = 0, edges = 0;
  uint32_t largest = 0u;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int l = labels[i];
    bool sh = true;
    if (l >= 0) {
      const int r = labels[l];                                // a tile-local root points at its global root
      sh = sizes[r] < min_size;
      if (l == (int)i && r == l) {                            // this pixel is a global root
        const int s = sizes[i];
        ++comp;
        kept += s >= min_size ? 1 : 0;
        largest = (uint32_t)s > largest ? (uint32_t)s : largest;
      }
    } else {
      ++edges;
    }
    mask[i] = sh ? 1 : 0;
    shadow += sh ? 1 : 0;
    if (depth) {
      const float d = depth[i];
      nonpos += (sh && d <= 0.f) ? 1 : 0;
      if (depth_out) depth_out[i] = sh ? __builtin_nanf("") : d;
    }
  }
  block_add(&hd->cnt[C_SHADOW], shadow, red);
  block_add(&hd->cnt[C_COMP], comp, red);
  block_add(&hd->cnt[C_KEPT], kept, red);
  block_add(&hd->cnt[C_NONPOS], nonpos, red);
  if (count_edges) block_add(&hd->cnt[C_EDGE], edges, red);
  block_max(&hd->largest, largest, red);
}

__global__ void sh_stats_kernel(const Header* __restrict__ hd, double* __restrict__ stats, float* __restrict__ gmax_out) {
  if (threadIdx.x != 0) return;
  const float gmax = __uint_as_float(hd->gmax_bits);
  stats[DP_SHADOW_STAT_EDGE] = (double)hd->cnt[C_EDGE];
  stats[DP_SHADOW_STAT_SHADOW] = (double)hd->cnt[C_SHADOW];
  stats[DP_SHADOW_STAT_COMPONENTS] = (double)hd->cnt[C_COMP];
  stats[DP_SHADOW_STAT_KEPT] = (double)hd->cnt[C_KEPT];
  stats[DP_SHADOW_STAT_LARGEST] = (double)hd->largest;
  stats[DP_SHADOW_STAT_GMAX] = (double)gmax;
  stats[DP_SHADOW_STAT_NONFINITE] = (double)hd->cnt[C_NONFINITE];
  stats[DP_SHADOW_STAT_ERROR] = hd->cnt[C_NONFINITE] ? 1.0 : 0.0;
  stats[DP_SHADOW_STAT_NONPOSITIVE] = (double)hd->cnt[C_NONPOS];
  if (gmax_out) *gmax_out = gmax;
}

// mode 0: z = (-n0 x - n1 y - d) / n2; mode 1 (horizontal plane): z = pf / (yi - cy), pf = (-d / n1) * f
__global__ void __launch_bounds__(256) sh_fill_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ shadow, int h, int w,
                                                      int row0, int mode, double n0, double n1, double n2, double dd, double pf,
                                                      float* __restrict__ out, unsigned long long* __restrict__ filled) {
  __shared__ int red[4];
  const long long n = (long long)h * w;
  const double cx = (double)w / 2.0, cy = (double)h / 2.0, f = (double)(w > h ? w : h);
  int cnt = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int yi = (int)((uint32_t)i / (uint32_t)w), xi = (int)(i - (long long)yi * w);   // h * w < 2^31
    float v = depth[i];
    if (yi >= row0 && shadow[i] != 0) {
      double z;
      if (mode == 0) {
        const double x = ((double)xi - cx) * 1.0 / f, y = ((double)yi - cy) * 1.0 / f;
        const double a = -n0 * x, b = n1 * y;
        z = (a - b - dd) / n2;
      } else {
        double den = (double)yi - cy;
        if (__builtin_fabs(den) < 1e-6) den = 1e-6;
        z = pf / den;
      }
      z = z < 0.1 ? 0.1 : z;                                  // np.maximum(z, 0.1): a NaN stays
      v = (float)z;
      ++cnt;
    }
    out[i] = v;
  }
  block_add(filled, cnt, red);
}

inline bool dims_ok(int32_t h, int32_t w) { return h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 31); }
inline bool finite_host(double v) { return v == v && v - v == 0.0; }
inline unsigned grid_for(long long n) {
  const long long b = (n + 255) / 256;
  return (unsigned)(b < MAX_BLOCKS ? b : MAX_BLOCKS);
}
inline bool ws_ok(const void* ws, int64_t bytes, int64_t n) {
  return ws && ((uintptr_t)ws & 7) == 0 && bytes >= layout(n).total;
}

// the region stages on a free mask already in place: labels, borders, flatten, mask
inline void launch_regions(const uint8_t* free_, int h, int w, int min_size, int count_edges, const float* depth, uint8_t* mask,
                           float* depth_out, char* ws, hipStream_t s) {
  const long long n = (long long)h * w;
  const Layout l = layout(n);
  Header* hd = (Header*)ws;
  int* labels = (int*)(ws + l.labels);
  int* sizes = (int*)(ws + l.sizes);
  const int tiles_x = (w + TILE - 1) / TILE, tiles_y = (h + TILE - 1) / TILE;
  hipLaunchKernelGGL(sh_tile_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(256), 0, s, free_, h, w, tiles_x, labels, sizes);
  const long long pairs = (long long)((h - 1) / TILE) * w + (long long)((w - 1) / TILE) * h;
  if (pairs > 0) hipLaunchKernelGGL(sh_border_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, s, labels, h, w);
  hipLaunchKernelGGL(sh_flatten_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, labels, sizes, n);
  hipLaunchKernelGGL(sh_mask_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const int*)labels, (const int*)sizes, n, min_size,
                     count_edges, depth, mask, depth_out, hd);
}
}  // namespace

extern "C" int64_t dp_shadows_workspace_size(int32_t h, int32_t w) {
  if (!dims_ok(h, w)) return 0;
  return layout((int64_t)h * w).total;
}

extern "C" int dp_depth_gradient(const float* depth, int32_t h, int32_t w, float* grad_out, float* gmax_out, double* stats_out,
                                 void* workspace, int64_t workspace_bytes, dp_stream_t stream) {
  if (!depth || !grad_out || !gmax_out || !stats_out) return DP_ERR_ARG;
  if (!dims_ok(h, w) || !ws_ok(workspace, workspace_bytes, (int64_t)h * w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  Header* hd = (Header*)workspace;
  const long long n = (long long)h * w;
  hipLaunchKernelGGL(sh_init_kernel, dim3(1), dim3(64), 0, s, hd);
  hipLaunchKernelGGL(sh_gradient_kernel, dim3(grid_for(n)), dim3(256), 0, s, depth, h, w, grad_out, hd);
  hipLaunchKernelGGL(sh_stats_kernel, dim3(1), dim3(64), 0, s, (const Header*)hd, stats_out, gmax_out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_depth_edges(const float* depth, int32_t h, int32_t w, double threshold_factor, uint8_t* edge_out,
                              double* stats_out, void* workspace, int64_t workspace_bytes, dp_stream_t stream) {
  if (!depth || !edge_out || !stats_out || !finite_host(threshold_factor)) return DP_ERR_ARG;
  if (!dims_ok(h, w) || !ws_ok(workspace, workspace_bytes, (int64_t)h * w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  Header* hd = (Header*)ws;
  const long long n = (long long)h * w;
  float* grad = (float*)(ws + layout(n).grad);
  hipLaunchKernelGGL(sh_init_kernel, dim3(1), dim3(64), 0, s, hd);
  hipLaunchKernelGGL(sh_gradient_kernel, dim3(grid_for(n)), dim3(256), 0, s, depth, h, w, grad, hd);
  hipLaunchKernelGGL(sh_edge_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const float*)grad, n, (float)threshold_factor, 0, edge_out, hd);
  hipLaunchKernelGGL(sh_stats_kernel, dim3(1), dim3(64), 0, s, (const Header*)hd, stats_out, (float*)nullptr);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_region_filter(const uint8_t* free_mask, int32_t h, int32_t w, int32_t min_region_size, uint8_t* mask_out,
                                double* stats_out, void* workspace, int64_t workspace_bytes, dp_stream_t stream) {
  if (!free_mask || !mask_out || !stats_out || min_region_size < 0) return DP_ERR_ARG;
  if (!dims_ok(h, w) || !ws_ok(workspace, workspace_bytes, (int64_t)h * w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  hipLaunchKernelGGL(sh_init_kernel, dim3(1), dim3(64), 0, s, (Header*)ws);
  launch_regions(free_mask, h, w, min_region_size, 1, nullptr, mask_out, nullptr, ws, s);
  hipLaunchKernelGGL(sh_stats_kernel, dim3(1), dim3(64), 0, s, (const Header*)ws, stats_out, (float*)nullptr);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_depth_shadows(const float* depth, int32_t h, int32_t w, double threshold_factor, int32_t min_region_size,
                                uint8_t* mask_out, float* depth_out, double* stats_out, void* workspace, int64_t workspace_bytes,
                                dp_stream_t stream) {
  if (!depth || !mask_out || !stats_out || !finite_host(threshold_factor) || min_region_size < 0) return DP_ERR_ARG;
  if (!dims_ok(h, w) || !ws_ok(workspace, workspace_bytes, (int64_t)h * w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  Header* hd = (Header*)ws;
  const long long n = (long long)h * w;
  const Layout l = layout(n);
  float* grad = (float*)(ws + l.grad);
  uint8_t* free_ = (uint8_t*)(ws + l.free_);
  hipLaunchKernelGGL(sh_init_kernel, dim3(1), dim3(64), 0, s, hd);
  hipLaunchKernelGGL(sh_gradient_kernel, dim3(grid_for(n)), dim3(256), 0, s, depth, h, w, grad, hd);
  hipLaunchKernelGGL(sh_edge_kernel, dim3(grid_for(n)), dim3(256), 0, s, (const float*)grad, n, (float)threshold_factor, 1, free_, hd);
  launch_regions(free_, h, w, min_region_size, 0, depth, mask_out, depth_out, ws, s);
  hipLaunchKernelGGL(sh_stats_kernel, dim3(1), dim3(64), 0, s, (const Header*)hd, stats_out, (float*)nullptr);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_fill_ground_shadows(const float* depth, const uint8_t* shadow, int32_t h, int32_t w, const double* plane,
                                      double ground_rows, float* depth_out, int64_t* filled_out, dp_stream_t stream) {
  if (!depth || !shadow || !plane || !depth_out || !filled_out || ((uintptr_t)filled_out & 7)) return DP_ERR_ARG;
  if (!dims_ok(h, w) || !finite_host(ground_rows)) return DP_ERR_ARG;
  const double n0 = plane[0], n1 = plane[1], n2 = plane[2], dd = plane[3];
  if (!(finite_host(n0) && finite_host(n1) && finite_host(n2) && finite_host(dd))) return DP_ERR_ARG;
  int mode;
  if ((n2 < 0 ? -n2 : n2) > 1e-6) mode = 0;
  else if ((n0 < 0 ? -n0 : n0) > 1e-6) return DP_ERR_ARG;      // the reference's 100-step depth search: not built
  else mode = 1;
  double r = ground_rows * (double)h;                           // int(ground_rows * h): towards zero
  r = r < 0.0 ? 0.0 : (r > (double)h ? (double)h : r);
  const int row0 = (int)r;
  const double f = (double)(w > h ? w : h);
  const double plane_y = -dd / n1;
  const double pf = plane_y * f;
  hipStream_t s = (hipStream_t)stream;
  const long long n = (long long)h * w;
  if (hipMemsetAsync(filled_out, 0, 8, s) != hipSuccess) return (int)hipGetLastError();
  hipLaunchKernelGGL(sh_fill_kernel, dim3(grid_for(n)), dim3(256), 0, s, depth, shadow, h, w, row0, mode, n0, n1, n2, dd, pf, depth_out,
                     (unsigned long long*)filled_out);
  DP_CHECK_LAUNCH();
  return 0;
}
