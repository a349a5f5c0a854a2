// Ground-normalised point clouds (ABI 15): segmented order statistics by MSD radix passes, the
// ground trace of the plane fit, the signed-distance percentile, normalise-to-ground and the
// per-cell grid adjustment -- img_to_normalized_pointcloud.py:601-816, :880-981, :983-1118.
// Everything is fp64 as numpy computes it; no FMA contraction anywhere in this file, so each
// product and sum is rounded on its own as numpy's ufuncs do.
#include "dp_common.h"
#include "dp_points.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_SEG = DP_GROUND_MAX_SEG;       // 1024
constexpr int MAX_GRID = DP_GROUND_MAX_GRID;     // 32
constexpr int LDS_SEG = 32;                      // segments whose 256-bin histograms fit one block's LDS (32 KiB)
constexpr int GRID_CAP = 2048;                   // workgroups of a per-point kernel at the most

// Scratch header at the start of the caller's workspace.  `hist` is zero between passes (the scan
// kernel clears the rows it read); everything else is cleared at the start of each entry point.
struct Hdr {
  u64 prefix[MAX_SEG];         // selected key bits so far (order-preserving key)
  u64 nextkey[MAX_SEG];        // smallest key above the selected one (percentile's upper neighbour)
  uint32_t idxprefix[MAX_SEG]; // index phase (ties at the cut in index order): selected index bits
  uint32_t rem[MAX_SEG];       // 0-based rank still to resolve inside the current prefix group
  uint32_t cnt[MAX_SEG];       // keys in the segment
  uint32_t ksel[MAX_SEG];      // 1-based rank selected (k-th smallest) / floor index + 1 (percentile)
  uint32_t active[MAX_SEG];
  uint32_t dup[MAX_SEG];       // the next rank holds the same key
  uint32_t cell_all[MAX_SEG];  // grid adjustment: all finite points of the cell
  double tfrac[MAX_SEG];       // percentile: fractional part of the virtual index
  double value[MAX_SEG];
  double sums[MAX_GRID * 3];
  u64 mm[4];                   // keys of min x, max x, min z, max z
  uint32_t ctr[16];
  uint32_t hist[MAX_SEG * 256];
};
enum { C_NONFINITE = 0, C_FINITE = 1, C_A = 2, C_B = 3, C_C = 4, C_D = 5, C_SLOT = 6 };

// One atomic per distinct bin of the wave (pixel neighbours mostly share a segment and a digit).
__device__ __forceinline__ void wave_hist_add(uint32_t* hist, int bin) {
  const int lane = threadIdx.x & 63;
  u64 todo = __ballot(bin >= 0);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int lb = __shfl(bin, leader);
    const u64 m = __ballot(bin == lb);
    if (lane == leader) atomicAdd(&hist[lb], (uint32_t)__popcll(m));
    todo &= ~m;
  }
}

__global__ void hdr_init_kernel(Hdr* h) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < MAX_SEG) h->nextkey[t] = ~0ull;
  if (t == 0) { h->mm[0] = ~0ull; h->mm[1] = 0; h->mm[2] = ~0ull; h->mm[3] = 0; }
}

// ---- selection ---------------------------------------------------------------------------------
// PHASE 0: digit `shift` of the key among the keys whose higher bits equal the prefix.
// PHASE 1: digit `shift` of the element index among the elements whose key equals the selected key.
// LDS: per-block histograms (n_seg <= LDS_SEG), flushed once; otherwise wave-aggregated global atomics.
template <int PHASE, bool LDS>
__global__ void __launch_bounds__(256) select_pass_kernel(const double* __restrict__ keys, long long stride,
                                                          const int32_t* __restrict__ seg, const int32_t* n_dev,
                                                          int n_max, int n_seg, int shift, Hdr* h) {
  __shared__ uint32_t lh[LDS ? LDS_SEG * 256 : 1];
  if (LDS) {
    for (int t = threadIdx.x; t < n_seg * 256; t += 256) lh[t] = 0;
    __syncthreads();
  }
  const int n = live_n(n_dev, n_max);
  for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
    const long long i = base + threadIdx.x;
    int bin = -1;
    if (i < n) {
      const int s = seg[i];
      // the first pass counts every segment (its scan then decides which take part)
      if (s >= 0 && s < n_seg && ((PHASE == 0 && shift == 56) || h->active[s])) {
        const u64 u = okey(keys[i * stride]);
        if (PHASE == 0) {
          if (shift == 56 || (u >> (shift + 8)) == (h->prefix[s] >> (shift + 8)))
            bin = s * 256 + (int)((u >> shift) & 255);
        } else {
          const uint32_t ii = (uint32_t)i;
          if (u == h->prefix[s] && (shift == 24 || (ii >> (shift + 8)) == (h->idxprefix[s] >> (shift + 8))))
            bin = s * 256 + (int)((ii >> shift) & 255);
        }
      }
    }
    wave_hist_add(LDS ? lh : h->hist, bin);
  }
  if (LDS) {
    __syncthreads();
    for (int t = threadIdx.x; t < n_seg * 256; t += 256)
      if (lh[t]) atomicAdd(&h->hist[t], lh[t]);
  }
}

struct SelRule {
  int mode;          // DP_SEL_PERCENTILE / DP_SEL_KTH
  double p;          // q / 100, or the fraction of the count
  int kmin;          // KTH: k = min(count, max(kmin, int(p * count)))
  int min_count;     // the segment takes part only if count > min_count
};

// One thread per segment: walk the 256 buckets, fix the next digit, clear the row.
__global__ void select_scan_kernel(Hdr* h, int n_seg, int shift, int phase, int first, int last, SelRule r) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seg) return;
  uint32_t* row = h->hist + s * 256;
  if (first) {
    uint32_t c = 0;
    for (int b = 0; b < 256; ++b) c += row[b];
    h->cnt[s] = c;
    uint32_t act = (c > (uint32_t)r.min_count) && c > 0;
    if (act) {
      if (r.mode == DP_SEL_PERCENTILE) {
        const double vi = (double)(c - 1) * r.p;
        double lo = __builtin_floor(vi);
        const double t = vi - lo;
        if (vi >= (double)(c - 1)) lo = (double)(c - 1);
        if (vi < 0.0) lo = 0.0;
        h->rem[s] = (uint32_t)lo;
        h->tfrac[s] = t;
      } else {
        int k = (int)(r.p * (double)c);
        k = k < r.kmin ? r.kmin : k;
        k = k > (int)c ? (int)c : k;
        h->rem[s] = (uint32_t)(k - 1);
      }
      h->ksel[s] = h->rem[s] + 1;
    }
    h->active[s] = act;
  }
  if (h->active[s]) {
    uint32_t rem = h->rem[s], cum = 0, hb = 0;
    int d = 255;
    for (int b = 0; b < 256; ++b) {
      hb = row[b];
      if (cum + hb > rem) { d = b; break; }
      cum += hb;
    }
    rem -= cum;
    h->rem[s] = rem;
    if (phase == 0) {
      h->prefix[s] |= (u64)d << shift;
      if (last) h->dup[s] = rem + 1 < hb;
    } else {
      h->idxprefix[s] |= (uint32_t)d << shift;
    }
  }
  for (int b = 0; b < 256; ++b) row[b] = 0;
}

// smallest key above the selected one, per segment (upper neighbour of the percentile).  Almost every
// key of a low percentile is a candidate at first, so the wave reduces its candidates per segment
// and issues one atomicMin for each, and only while they beat the value already there.
__global__ void __launch_bounds__(256) select_next_kernel(const double* __restrict__ keys, long long stride,
                                                          const int32_t* __restrict__ seg, const int32_t* n_dev,
                                                          int n_max, int n_seg, Hdr* h) {
  const int n = live_n(n_dev, n_max), lane = threadIdx.x & 63;
  for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
    const long long i = base + threadIdx.x;
    int s = -1;
    u64 u = ~0ull;
    if (i < n) {
      s = seg[i];
      if (s >= 0 && s < n_seg && h->active[s] && !h->dup[s]) {
        u = okey(keys[i * stride]);
        // the plain read is only a filter: a stale value lets a needless atomic through, never drops one
        if (!(u > h->prefix[s] && u < *(volatile u64*)&h->nextkey[s])) s = -1;
      } else {
        s = -1;
      }
    }
    u64 todo = __ballot(s >= 0);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int ls = __shfl(s, leader);
      const bool mine = s == ls;
      u64 m = mine ? u : ~0ull;
      #pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const u64 t = __shfl_xor(m, o);
        m = t < m ? t : m;
      }
      if (lane == leader) atomicMin(&h->nextkey[ls], m);
      todo &= ~__ballot(mine);
    }
  }
}

__global__ void select_final_kernel(Hdr* h, int n_seg, SelRule r, int32_t* counts_out, double* values_out) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seg) return;
  double v = __builtin_nan("");
  if (h->active[s]) {
    const double a = unkey(h->prefix[s]);
    if (r.mode == DP_SEL_PERCENTILE) {
      double b = a;
      if (!h->dup[s] && h->ksel[s] < h->cnt[s] && h->nextkey[s] != ~0ull) b = unkey(h->nextkey[s]);
      const double t = h->tfrac[s];
      const double diff = b - a;
      v = a + diff * t;                               // numpy's _lerp, both sides
      if (t >= 0.5) v = b - diff * (1.0 - t);
    } else {
      v = a;
    }
  }
  h->value[s] = v;
  if (counts_out) counts_out[s] = (int32_t)h->cnt[s];
  if (values_out) values_out[s] = v;
}

// The whole selection on stream s: 8 key passes (+ 4 index passes with `by_index`), then the
// percentile's neighbour + lerp.  Results stay in the header (value / prefix / idxprefix / ksel).
void run_select(hipStream_t s, Hdr* h, const double* keys, long long stride, const int32_t* seg, const int32_t* n_dev,
                int n_max, int n_seg, SelRule r, bool by_index, int32_t* counts_out, double* values_out) {
  const int g = grid_for(n_max, GRID_CAP), sg = (n_seg + 63) / 64;
  const bool lds = n_seg <= LDS_SEG;
  for (int p = 0; p < 8; ++p) {
    const int shift = 56 - 8 * p;
    if (lds)
      hipLaunchKernelGGL((select_pass_kernel<0, true>), dim3(g), dim3(256), 0, s, keys, stride, seg, n_dev, n_max, n_seg, shift, h);
    else
      hipLaunchKernelGGL((select_pass_kernel<0, false>), dim3(g), dim3(256), 0, s, keys, stride, seg, n_dev, n_max, n_seg, shift, h);
    hipLaunchKernelGGL(select_scan_kernel, dim3(sg), dim3(64), 0, s, h, n_seg, shift, 0, p == 0, p == 7, r);
  }
  if (by_index) {
    for (int p = 0; p < 4; ++p) {
      const int shift = 24 - 8 * p;
      if (lds)
        hipLaunchKernelGGL((select_pass_kernel<1, true>), dim3(g), dim3(256), 0, s, keys, stride, seg, n_dev, n_max, n_seg, shift, h);
      else
        hipLaunchKernelGGL((select_pass_kernel<1, false>), dim3(g), dim3(256), 0, s, keys, stride, seg, n_dev, n_max, n_seg, shift, h);
      hipLaunchKernelGGL(select_scan_kernel, dim3(sg), dim3(64), 0, s, h, n_seg, shift, 1, 0, p == 3, r);
    }
  }
  if (r.mode == DP_SEL_PERCENTILE)
    hipLaunchKernelGGL(select_next_kernel, dim3(g), dim3(256), 0, s, keys, stride, seg, n_dev, n_max, n_seg, h);
  hipLaunchKernelGGL(select_final_kernel, dim3(sg), dim3(64), 0, s, h, n_seg, r, counts_out, values_out);
}

void clear_hdr(hipStream_t s, Hdr* h) {
  (void)hipMemsetAsync(h, 0, sizeof(Hdr), s);
  hipLaunchKernelGGL(hdr_init_kernel, dim3(MAX_SEG / 256), dim3(256), 0, s, h);
}

struct Ws {
  Hdr* h;
  int32_t* seg;
  double* tmp;
};
int64_t ws_bytes_for(int64_t n_max) {
  const int64_t n = n_max < 0 ? 0 : n_max;
  return (int64_t)sizeof(Hdr) + al256(n * 4) + n * 8 + 256;
}
bool ws_carve(void* ws, int64_t bytes, int n_max, Ws* o) {
  if (!ws || bytes < ws_bytes_for(n_max) || ((uintptr_t)ws & 7)) return false;
  char* p = (char*)ws;
  o->h = (Hdr*)p;
  p += sizeof(Hdr);
  o->seg = (int32_t*)p;
  p += al256((int64_t)n_max * 4);
  o->tmp = (double*)p;
  return true;
}

// ---- per-point stages --------------------------------------------------------------------------
// min / max of x and z over the finite points, and the finite / non-finite counts
__global__ void __launch_bounds__(256) minmax_xz_kernel(const double* __restrict__ pts, const int32_t* n_dev, int n_max,
                                                        Hdr* h) {
  const int n = live_n(n_dev, n_max);
  u64 mn[2] = {~0ull, ~0ull}, mx[2] = {0, 0};                    // x, z
  uint32_t bad = 0, good = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    if (!finite3(x, y, z)) { ++bad; continue; }
    ++good;
    const u64 k[2] = {okey(x), okey(z)};
    #pragma unroll
    for (int a = 0; a < 2; ++a) { mn[a] = k[a] < mn[a] ? k[a] : mn[a]; mx[a] = k[a] > mx[a] ? k[a] : mx[a]; }
  }
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    wave_minmax(mn, mx, o);
    bad += __shfl_xor(bad, o);
    good += __shfl_xor(good, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (good) {
      flush_minmax(h->mm, mn, mx);
      atomicAdd(&h->ctr[C_FINITE], good);
    }
    if (bad) atomicAdd(&h->ctr[C_NONFINITE], bad);
  }
}

// np.linspace(mn, mx, g + 1): start + i * step, the last edge set to stop
__device__ __forceinline__ void make_edges(double* e, double mn, double mx, int g) {
  const double step = (mx - mn) / (double)g;
  for (int i = threadIdx.x; i <= g; i += blockDim.x) e[i] = i < g ? (double)i * step + mn : mx;
}
// np.digitize(v, e) - 1 for non-decreasing e[0..g]: (number of edges <= v) - 1
__device__ __forceinline__ int digitize_m1(const double* e, int g, double v) {
  int lo = 0, hi = g + 1;          // first index with e[idx] > v
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (e[mid] <= v) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

// ground trace: z bin of every finite point (-1: outside every bin, as z == z_max is, or non-finite)
__global__ void __launch_bounds__(256) trace_assign_kernel(const double* __restrict__ pts, const int32_t* n_dev, int n_max,
                                                           int g, Hdr* h, int32_t* __restrict__ seg) {
  __shared__ double e[MAX_GRID + 1];
  make_edges(e, unkey(h->mm[2]), unkey(h->mm[3]), g);
  __syncthreads();
  const int n = live_n(n_dev, n_max);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    int s = -1;
    if (finite3(x, y, z)) {
      s = digitize_m1(e, g, z);
      if (s >= g || s < 0) s = -1;
    }
    seg[i] = s;
  }
}

// every finite point in segment 0 (fallback trace, distance percentile)
__global__ void __launch_bounds__(256) all_assign_kernel(const double* __restrict__ pts, const int32_t* n_dev, int n_max,
                                                         int32_t* __restrict__ seg) {
  const int n = live_n(n_dev, n_max);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    seg[i] = finite3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]) ? 0 : -1;
}

__device__ __forceinline__ bool in_lowest(const Hdr* h, int s, double y, long long i) {
  const u64 u = okey(y), cut = h->prefix[s];
  return u < cut || (u == cut && (uint32_t)i <= h->idxprefix[s]);
}

// sums of the selected (lowest-k by y, ties in index order) points of each z bin
__global__ void __launch_bounds__(256) trace_sum_kernel(const double* __restrict__ pts, const int32_t* __restrict__ seg,
                                                        const int32_t* n_dev, int n_max, Hdr* h) {
  const int n = live_n(n_dev, n_max), lane = threadIdx.x & 63;
  for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
    const long long i = base + threadIdx.x;
    int s = -1;
    double x = 0, y = 0, z = 0;
    if (i < n) {
      s = seg[i];
      if (s >= 0 && h->active[s]) {
        x = pts[3 * i]; y = pts[3 * i + 1]; z = pts[3 * i + 2];
        if (!in_lowest(h, s, y, i)) s = -1;
      } else {
        s = -1;
      }
    }
    u64 todo = __ballot(s >= 0);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int ls = __shfl(s, leader);
      const bool mine = s == ls;
      double ax = mine ? x : 0.0, ay = mine ? y : 0.0, az = mine ? z : 0.0;
      #pragma unroll
      for (int o = 32; o > 0; o >>= 1) { ax += __shfl_xor(ax, o); ay += __shfl_xor(ay, o); az += __shfl_xor(az, o); }
      if (lane == 0) {
        atomicAdd(&h->sums[3 * ls], ax); atomicAdd(&h->sums[3 * ls + 1], ay); atomicAdd(&h->sums[3 * ls + 2], az);
      }
      todo &= ~__ballot(mine);
    }
  }
}

__global__ void trace_final_kernel(Hdr* h, int g, double* trace, int32_t* valid, double* info) {
  const int s = threadIdx.x;
  if (s < g) {
    const bool a = h->active[s] != 0;
    const double k = (double)h->ksel[s];
    trace[4 * s + 0] = a ? h->sums[3 * s] / k : 0.0;
    trace[4 * s + 1] = a ? h->sums[3 * s + 1] / k : 0.0;
    trace[4 * s + 2] = a ? h->sums[3 * s + 2] / k : 0.0;
    trace[4 * s + 3] = (double)h->cnt[s];
    valid[s] = a;
  }
  if (s == 0) {
    const bool any = h->ctr[C_FINITE] != 0;
    info[0] = (double)h->ctr[C_FINITE];
    info[1] = (double)h->ctr[C_NONFINITE];
    info[2] = any ? unkey(h->mm[2]) : 0.0;
    info[3] = any ? unkey(h->mm[3]) : 0.0;
  }
}

// fallback trace: the selected points and their indices, in any order (the caller sorts by index)
__global__ void __launch_bounds__(256) lowest_gather_kernel(const double* __restrict__ pts, const int32_t* __restrict__ seg,
                                                            const int32_t* n_dev, int n_max, Hdr* h, double* out_pts,
                                                            int32_t* out_idx, int cap) {
  const int n = live_n(n_dev, n_max), lane = threadIdx.x & 63;
  for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
    const long long i = base + threadIdx.x;
    bool sel = false;
    if (i < n && seg[i] == 0 && h->active[0]) sel = in_lowest(h, 0, pts[3 * i + 1], i);
    const u64 m = __ballot(sel);
    if (!m) continue;
    uint32_t b = 0;
    if (lane == 0) b = atomicAdd(&h->ctr[C_SLOT], (uint32_t)__popcll(m));
    b = __shfl(b, 0);
    if (sel) {
      const uint32_t slot = b + (uint32_t)__popcll(m & ((1ull << lane) - 1));
      if (slot < (uint32_t)cap) {
        out_pts[3 * slot] = pts[3 * i]; out_pts[3 * slot + 1] = pts[3 * i + 1]; out_pts[3 * slot + 2] = pts[3 * i + 2];
        out_idx[slot] = (int32_t)i;
      }
    }
  }
}
__global__ void lowest_final_kernel(Hdr* h, double* info) {
  info[0] = h->active[0] ? (double)h->ksel[0] : 0.0;
  info[1] = (double)h->cnt[0];
}

struct Plane { double nx, ny, nz, d; };
__device__ __forceinline__ double plane_dist(const Plane& p, double x, double y, double z) {
  return ((x * p.nx + y * p.ny) + z * p.nz) + p.d;
}

__global__ void __launch_bounds__(256) dist_kernel(const double* __restrict__ pts, const int32_t* n_dev, int n_max, Plane pl,
                                                   Hdr* h, int32_t* __restrict__ seg, double* __restrict__ dist) {
  const int n = live_n(n_dev, n_max);
  for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
    const long long i = base + threadIdx.x;
    bool bad = false, below = false;
    if (i < n) {
      const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
      bad = !finite3(x, y, z);
      const double dd = bad ? 0.0 : plane_dist(pl, x, y, z);
      below = !bad && dd < 0.0;
      seg[i] = bad ? -1 : 0;
      dist[i] = dd;
    }
    wave_count(&h->ctr[C_NONFINITE], bad);
    wave_count(&h->ctr[C_A], below);
  }
}
__global__ void dist_final_kernel(Hdr* h, double* out) {
  out[0] = h->value[0];
  out[1] = (double)h->ctr[C_A];
  out[2] = (double)h->cnt[0];
  out[3] = (double)h->ctr[C_NONFINITE];
}

struct NormArgs { Plane pl; double R[9]; double cst; int rotate; };

// p' = R p, y' -= const (or a copy in the no-rotation branch); segment 0 = |dist| < 0.1
__global__ void __launch_bounds__(256) norm_rotate_kernel(const double* __restrict__ pts, double* __restrict__ out,
                                                          const int32_t* n_dev, int n_max, NormArgs a, Hdr* h,
                                                          int32_t* __restrict__ seg) {
  const int n = live_n(n_dev, n_max);
  for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
    const long long i = base + threadIdx.x;
    bool bad = false;
    if (i < n) {
      const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
      bad = !finite3(x, y, z);
      double ox = x, oy = y, oz = z;
      int s = -1;
      if (!bad) {
        const double dd = plane_dist(a.pl, x, y, z);
        if (a.rotate) {
          ox = (a.R[0] * x + a.R[1] * y) + a.R[2] * z;
          oy = ((a.R[3] * x + a.R[4] * y) + a.R[5] * z) - a.cst;
          oz = (a.R[6] * x + a.R[7] * y) + a.R[8] * z;
        }
        if (__builtin_fabs(dd) < 0.1) s = 0;
      }
      out[3 * i] = ox; out[3 * i + 1] = oy; out[3 * i + 2] = oz;
      seg[i] = s;
    }
    wave_count(&h->ctr[C_NONFINITE], bad);
    wave_count(&h->ctr[C_FINITE], i < n && !bad);
  }
}

// y' -= ground level (if it was taken), then the two clamps
__global__ void __launch_bounds__(256) norm_clamp_kernel(const double* __restrict__ pts, double* __restrict__ out,
                                                         const int32_t* n_dev, int n_max, NormArgs a, Hdr* h) {
  const int n = live_n(n_dev, n_max);
  const bool shift = h->active[0] != 0;
  const double level = shift ? h->value[0] : 0.0;
  for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
    const long long i = base + threadIdx.x;
    bool ground = false, zeroed = false, limited = false;
    if (i < n) {
      const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
      if (finite3(x, y, z)) {
        ground = __builtin_fabs(plane_dist(a.pl, x, y, z)) < 0.05;
        double v = out[3 * i + 1];
        if (shift) v -= level;
        if (ground && v < 0.0) { v = 0.0; zeroed = true; }
        if (!ground && v < -0.1) { v = -0.1; limited = true; }
        out[3 * i + 1] = v;
      }
    }
    wave_count(&h->ctr[C_A], ground);
    wave_count(&h->ctr[C_B], zeroed);
    wave_count(&h->ctr[C_C], limited);
  }
}
__global__ void norm_final_kernel(Hdr* h, double* st) {
  st[0] = (double)h->ctr[C_FINITE];
  st[1] = (double)h->ctr[C_NONFINITE];
  st[2] = (double)h->cnt[0];
  st[3] = h->active[0] ? h->value[0] : 0.0;
  st[4] = (double)h->active[0];
  st[5] = (double)h->ctr[C_A];
  st[6] = (double)h->ctr[C_B];
  st[7] = (double)h->ctr[C_C];
}

// grid adjustment: cell = x bin * g + z bin (digitize - 1, clipped); seg = cell for the points with
// y < 0.2, -(cell + 2) for the others (not in any selection segment), -1 for non-finite points
__global__ void __launch_bounds__(256) adjust_assign_kernel(const double* __restrict__ pts, const int32_t* n_dev, int n_max,
                                                            int g, Hdr* h, int32_t* __restrict__ seg) {
  __shared__ double ex[MAX_GRID + 1], ez[MAX_GRID + 1];
  make_edges(ex, unkey(h->mm[0]), unkey(h->mm[1]), g);
  make_edges(ez, unkey(h->mm[2]), unkey(h->mm[3]), g);
  __syncthreads();
  const int n = live_n(n_dev, n_max);
  for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
    const long long i = base + threadIdx.x;
    int cell = -1;
    if (i < n) {
      const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
      int s = -1;
      if (finite3(x, y, z)) {
        int xi = digitize_m1(ex, g, x), zi = digitize_m1(ez, g, z);
        xi = xi < 0 ? 0 : (xi > g - 1 ? g - 1 : xi);
        zi = zi < 0 ? 0 : (zi > g - 1 ? g - 1 : zi);
        cell = xi * g + zi;
        s = y < 0.2 ? cell : -(cell + 2);
      }
      seg[i] = s;
    }
    wave_hist_add(h->cell_all, cell);
  }
}

__global__ void __launch_bounds__(256) adjust_apply_kernel(const double* __restrict__ pts, double* __restrict__ out,
                                                           const int32_t* __restrict__ seg, const int32_t* n_dev,
                                                           int n_max, Hdr* h) {
  const int n = live_n(n_dev, n_max);
  for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {
    const long long i = base + threadIdx.x;
    bool adjusted = false;
    if (i < n) {
      const double x = pts[3 * i], z = pts[3 * i + 2];
      double y = pts[3 * i + 1];
      const int s = seg[i];
      if (s != -1) {
        const int cell = s >= 0 ? s : -(s + 2);
        const double p = h->value[cell];
        if (h->cell_all[cell] >= 10 && h->cnt[cell] >= 5 && p > 0.01) {
          double adj = 0.0;
          if (y < 0.1) adj = p;
          else if (y < 1.5) adj = p * (1.0 - (y - 0.1) / 1.4);
          y = y - adj;
          if (y < 0.0) y = 0.0;
          adjusted = adj > 0.0;
        }
      }
      out[3 * i] = x; out[3 * i + 1] = y; out[3 * i + 2] = z;
    }
    wave_count(&h->ctr[C_A], adjusted);
  }
}
__global__ void adjust_final_kernel(Hdr* h, int cells, double* st) {
  __shared__ uint32_t c[3];
  if (threadIdx.x < 3) c[threadIdx.x] = 0;
  __syncthreads();
  for (int s = threadIdx.x; s < cells; s += blockDim.x) {
    const uint32_t all = h->cell_all[s];
    if (all) atomicAdd(&c[0], 1u);
    if (all >= 10) atomicAdd(&c[1], 1u);
    if (all >= 10 && h->cnt[s] >= 5 && h->value[s] > 0.01) atomicAdd(&c[2], 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    st[0] = (double)h->ctr[C_FINITE];
    st[1] = (double)h->ctr[C_NONFINITE];
    st[2] = (double)c[0];
    st[3] = (double)c[1];
    st[4] = (double)c[2];
    st[5] = (double)h->ctr[C_A];
    st[6] = 0.0;
    st[7] = 0.0;
  }
}
}  // namespace

extern "C" int64_t dp_ground_workspace_size(int64_t n_max) { return ws_bytes_for(n_max); }

extern "C" int dp_seg_select(const double* keys, int64_t key_stride, const int32_t* seg, const int32_t* n_dev,
                             int32_t n_max, int32_t n_seg, int32_t mode, double param, int32_t kmin, int32_t min_count,
                             int32_t* counts_out, double* values_out, void* workspace, int64_t workspace_bytes,
                             dp_stream_t stream) {
  if (!counts_out || !values_out || (n_max > 0 && (!keys || !seg))) return DP_ERR_ARG;
  if (mode != DP_SEL_PERCENTILE && mode != DP_SEL_KTH) return DP_ERR_ARG;
  if (n_max < 0 || n_seg < 1 || n_seg > MAX_SEG || key_stride < 1 || kmin < 1 || min_count < 0) return DP_ERR_SHAPE;
  if (mode == DP_SEL_PERCENTILE && !(param >= 0.0 && param <= 100.0)) return DP_ERR_ARG;
  if (mode == DP_SEL_KTH && !(param >= 0.0 && param <= 1.0)) return DP_ERR_ARG;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, n_max, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  clear_hdr(s, w.h);
  const SelRule r = {mode, mode == DP_SEL_PERCENTILE ? param / 100.0 : param, kmin, min_count};
  run_select(s, w.h, keys, key_stride, seg, n_dev, n_max, n_seg, r, false, counts_out, values_out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_ground_trace(const double* points, const int32_t* n_dev, int32_t n_max, int32_t grid_size,
                               double* trace_out, int32_t* valid_out, double* info_out, void* workspace,
                               int64_t workspace_bytes, dp_stream_t stream) {
  if (!trace_out || !valid_out || !info_out || (n_max > 0 && !points)) return DP_ERR_ARG;
  if (n_max < 0 || grid_size < 1 || grid_size > MAX_GRID) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, n_max, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int g = grid_for(n_max, GRID_CAP);
  clear_hdr(s, w.h);
  hipLaunchKernelGGL(minmax_xz_kernel, dim3(g), dim3(256), 0, s, points, n_dev, n_max, w.h);
  hipLaunchKernelGGL(trace_assign_kernel, dim3(g), dim3(256), 0, s, points, n_dev, n_max, grid_size, w.h, w.seg);
  const SelRule r = {DP_SEL_KTH, 0.05, 1, 10};
  run_select(s, w.h, points + 1, 3, w.seg, n_dev, n_max, grid_size, r, true, nullptr, nullptr);
  hipLaunchKernelGGL(trace_sum_kernel, dim3(g), dim3(256), 0, s, points, w.seg, n_dev, n_max, w.h);
  hipLaunchKernelGGL(trace_final_kernel, dim3(1), dim3(64), 0, s, w.h, grid_size, trace_out, valid_out, info_out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_ground_lowest(const double* points, const int32_t* n_dev, int32_t n_max, double* points_out,
                                int32_t* index_out, int32_t capacity, double* info_out, void* workspace,
                                int64_t workspace_bytes, dp_stream_t stream) {
  if (!info_out || (n_max > 0 && !points) || (capacity > 0 && (!points_out || !index_out))) return DP_ERR_ARG;
  if (n_max < 0 || capacity < 0) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, n_max, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int g = grid_for(n_max, GRID_CAP);
  clear_hdr(s, w.h);
  hipLaunchKernelGGL(all_assign_kernel, dim3(g), dim3(256), 0, s, points, n_dev, n_max, w.seg);
  const SelRule r = {DP_SEL_KTH, 0.05, 10, 0};
  run_select(s, w.h, points + 1, 3, w.seg, n_dev, n_max, 1, r, true, nullptr, nullptr);
  hipLaunchKernelGGL(lowest_gather_kernel, dim3(g), dim3(256), 0, s, points, w.seg, n_dev, n_max, w.h, points_out,
                     index_out, capacity);
  hipLaunchKernelGGL(lowest_final_kernel, dim3(1), dim3(1), 0, s, w.h, info_out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_ground_dist_percentile(const double* points, const int32_t* n_dev, int32_t n_max,
                                         const double* plane, double q, double* out, void* workspace,
                                         int64_t workspace_bytes, dp_stream_t stream) {
  if (!plane || !out || (n_max > 0 && !points)) return DP_ERR_ARG;
  if (n_max < 0) return DP_ERR_SHAPE;
  if (!(q >= 0.0 && q <= 100.0)) return DP_ERR_ARG;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, n_max, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int g = grid_for(n_max, GRID_CAP);
  clear_hdr(s, w.h);
  const Plane pl = {plane[0], plane[1], plane[2], plane[3]};
  hipLaunchKernelGGL(dist_kernel, dim3(g), dim3(256), 0, s, points, n_dev, n_max, pl, w.h, w.seg, w.tmp);
  const SelRule r = {DP_SEL_PERCENTILE, q / 100.0, 1, 0};
  run_select(s, w.h, w.tmp, 1, w.seg, n_dev, n_max, 1, r, false, nullptr, nullptr);
  hipLaunchKernelGGL(dist_final_kernel, dim3(1), dim3(1), 0, s, w.h, out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_ground_normalize(const double* points, double* points_out, const int32_t* n_dev, int32_t n_max,
                                   const double* model, double* stats_out, void* workspace, int64_t workspace_bytes,
                                   dp_stream_t stream) {
  if (!model || !stats_out || (n_max > 0 && (!points || !points_out))) return DP_ERR_ARG;
  if (n_max < 0) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, n_max, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int g = grid_for(n_max, GRID_CAP);
  clear_hdr(s, w.h);
  NormArgs a;
  a.pl = {model[0], model[1], model[2], model[3]};
  for (int i = 0; i < 9; ++i) a.R[i] = model[4 + i];
  a.cst = model[13];
  a.rotate = model[14] != 0.0;
  hipLaunchKernelGGL(norm_rotate_kernel, dim3(g), dim3(256), 0, s, points, points_out, n_dev, n_max, a, w.h, w.seg);
  const SelRule r = {DP_SEL_PERCENTILE, 2.0 / 100.0, 1, 10};
  run_select(s, w.h, points_out + 1, 3, w.seg, n_dev, n_max, 1, r, false, nullptr, nullptr);
  hipLaunchKernelGGL(norm_clamp_kernel, dim3(g), dim3(256), 0, s, points, points_out, n_dev, n_max, a, w.h);
  hipLaunchKernelGGL(norm_final_kernel, dim3(1), dim3(1), 0, s, w.h, stats_out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_ground_adjust(const double* points, double* points_out, const int32_t* n_dev, int32_t n_max,
                                int32_t grid_size, double percentile, double* stats_out, void* workspace,
                                int64_t workspace_bytes, dp_stream_t stream) {
  if (!stats_out || (n_max > 0 && (!points || !points_out))) return DP_ERR_ARG;
  if (n_max < 0 || grid_size < 1 || grid_size > MAX_GRID) return DP_ERR_SHAPE;
  if (!(percentile >= 0.0 && percentile <= 100.0)) return DP_ERR_ARG;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, n_max, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int g = grid_for(n_max, GRID_CAP), cells = grid_size * grid_size;
  clear_hdr(s, w.h);
  hipLaunchKernelGGL(minmax_xz_kernel, dim3(g), dim3(256), 0, s, points, n_dev, n_max, w.h);
  hipLaunchKernelGGL(adjust_assign_kernel, dim3(g), dim3(256), 0, s, points, n_dev, n_max, grid_size, w.h, w.seg);
  const SelRule r = {DP_SEL_PERCENTILE, percentile / 100.0, 1, 0};
  run_select(s, w.h, points + 1, 3, w.seg, n_dev, n_max, cells, r, false, nullptr, nullptr);
  hipLaunchKernelGGL(adjust_apply_kernel, dim3(g), dim3(256), 0, s, points, points_out, w.seg, n_dev, n_max, w.h);
  hipLaunchKernelGGL(adjust_final_kernel, dim3(1), dim3(256), 0, s, w.h, cells, stats_out);
  DP_CHECK_LAUNCH();
  return 0;
}
