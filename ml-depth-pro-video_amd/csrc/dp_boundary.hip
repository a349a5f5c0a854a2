// Scale-invariant boundary metric (csrc/dp_boundary.hip): the edge counts behind SI_boundary_F1 and
// SI_boundary_Recall of the reference's depth_pro/eval/boundary_metrics.py, and the edge maps themselves.
// The specification is in dp_mi355x.h.  fp32 with IEEE division and denormals, no fast-math.
//
// A threshold reaches the kernels as f = the largest float32 <= t (floor_f32): for a float32 ratio r,
// (double)r > t  <=>  r > f.  (If r > t then r > t >= f.  If r > f then r >= the float32 after f, which is > t
// unless f == t, and then r > t as it stands.  A t past the float32 range gives f = FLT_MAX or -inf, and the
// equivalence holds with r = +-inf too.)  So the comparison is the header's, made in fp32.
//
// Thinned edges.  A line (a row of a horizontal map, a column of a vertical one) is cut into segments of SEG
// cells.  walk_kernel: one lane walks one segment of one line and keeps, per threshold, the run that is open
// (largest ratio so far, the target bit there).  A run that begins and ends inside the segment is counted at
// once; the run that touches the segment's first cell (head) and the one still open at its last cell (tail)
// go to the workspace, a segment that is one run throughout as head with the tail marked WHOLE.
// combine_kernel: one lane per line, threshold and direction joins the segments in order.  Both passes are
// bounded by the image's size whatever the runs' lengths.
#include "dp_common.h"

namespace {

typedef unsigned long long u64;

constexpr int SEG = DP_BOUNDARY_SEGMENT;        // cells of a line's segment
constexpr int TK = 16;                          // thresholds a walk pass keeps in registers
constexpr int MAX_T = DP_BOUNDARY_MAX_T;
constexpr uint32_t NONE = 0xfffffffeu;          // no head / tail run (a NaN pattern: a run's largest ratio is never NaN)
constexpr uint32_t WHOLE = 0xffffffffu;         // tail: the head run is still open at the segment's end
static_assert(SEG == 64, "a lane keeps a segment's target bits in one 64-bit word");

struct Thr { float f[MAX_T]; };                 // floor_f32 of the thresholds

__device__ __forceinline__ float inv_depth(float d, int inverse) {
  if (inverse) return d;
  return 1.0f / (d < 1e-6f ? 1e-6f : d);        // NaN stays NaN (numpy's clip)
}

// thresholds from the kernel arguments into LDS with constant indices (a dynamic index would copy the struct)
__device__ __forceinline__ void stage_thresholds(const Thr& thr, float* sth) {
  #pragma unroll
  for (int k = 0; k < MAX_T; ++k)
    if (threadIdx.x == k) sth[k] = thr.f[k];
}

// ---- plain edges of two depths: all thresholds in one pass ------------------------------------------
constexpr int PL_ROWS = 16, PL_ITEMS = 4;       // rows of a workgroup's tile (256 columns wide), rows per thread and step

struct Ratios { float r[4]; };                  // left, top, right, bottom of the pixel pair that starts here

__device__ __forceinline__ Ratios ratios_at(const float* __restrict__ img, int64_t ld, int H, int W, int y, int x, int inverse) {
  const float nan = __builtin_nanf("");
  Ratios o;
  o.r[0] = o.r[1] = o.r[2] = o.r[3] = nan;
  if (y < H && x < W) {
    const float c = inv_depth(img[(int64_t)y * ld + x], inverse);
    if (x + 1 < W) {
      const float e = inv_depth(img[(int64_t)y * ld + x + 1], inverse);
      o.r[0] = c / e; o.r[2] = e / c;
    }
    if (y + 1 < H) {
      const float s = inv_depth(img[(int64_t)(y + 1) * ld + x], inverse);
      o.r[1] = c / s; o.r[3] = s / c;
    }
  }
  return o;
}

__global__ void __launch_bounds__(256) plain_counts_kernel(const float* __restrict__ pred, int64_t ldp, const float* __restrict__ tgt,
                                                           int64_t ldt, int H, int W, int inverse, Thr thr, int n_t,
                                                           u64* __restrict__ counts) {
  __shared__ uint32_t acc[MAX_T * 12];
  __shared__ float sth[MAX_T];
  for (int j = threadIdx.x; j < MAX_T * 12; j += 256) acc[j] = 0;
  stage_thresholds(thr, sth);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int x = blockIdx.x * 256 + threadIdx.x, y0 = blockIdx.y * PL_ROWS;
  for (int yy = 0; yy < PL_ROWS && y0 + yy < H; yy += PL_ITEMS) {      // uniform over the workgroup
    Ratios p[PL_ITEMS], g[PL_ITEMS];
    #pragma unroll
    for (int i = 0; i < PL_ITEMS; ++i) {
      const int y = y0 + yy + i;
      p[i] = ratios_at(pred, ldp, H, W, y, x, inverse);
      g[i] = ratios_at(tgt, ldt, H, W, y, x, inverse);
    }
    for (int k = 0; k < n_t; ++k) {
      const float f = sth[k];
      uint32_t s[12];
      #pragma unroll
      for (int d = 0; d < 4; ++d) {
        uint32_t both = 0, tg = 0, pr = 0;
        #pragma unroll
        for (int i = 0; i < PL_ITEMS; ++i) {
          const bool ep = p[i].r[d] > f, eg = g[i].r[d] > f;
          both += (uint32_t)__popcll(__ballot(ep && eg));
          tg += (uint32_t)__popcll(__ballot(eg));
          pr += (uint32_t)__popcll(__ballot(ep));
        }
        s[3 * d] = both; s[3 * d + 1] = tg; s[3 * d + 2] = pr;
      }
      uint32_t v = 0;
      #pragma unroll
      for (int j = 0; j < 12; ++j) v = lane == j ? s[j] : v;
      if (lane < 12 && v) atomicAdd(&acc[k * 12 + lane], v);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < n_t * 12; j += 256)
    if (acc[j]) atomicAdd(&counts[j], (u64)acc[j]);
}

__global__ void __launch_bounds__(256) plain_edges_kernel(const float* __restrict__ depth, int64_t ld, int H, int W, float f,
                                                          uint8_t* __restrict__ maps) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= W) return;
  const Ratios r = ratios_at(depth, ld, H, W, y, x, 0);
  const int64_t plane = (int64_t)H * W, at = (int64_t)y * W + x;
  #pragma unroll
  for (int d = 0; d < 4; ++d) maps[d * plane + at] = r.r[d] > f;      // NaN outside the map's extent: 0
}

// ---- thinned edges ----------------------------------------------------------------------------------
struct Summ {                                   // one orientation's part of the workspace
  uint32_t* head;                               // [2 dirs][n_t][nseg][lines] largest ratio's bits, NONE
  uint32_t* tail;                               //   the same, NONE or WHOLE
  uint32_t* tbits;                              // [2 dirs][passes][nseg][lines] target bits: head k at bit k, tail k at 16 + k
  int32_t* hpos;                                // [2 dirs][nseg][lines] the kept cell's place on the line (edge maps only)
  int32_t* tpos;
};

// VERT: a line is a column (top, bottom), else a row (left, right).  EDGES: one threshold, the kept cells are
// written to `maps`; else up to TK thresholds from 16 * blockIdx.y on and the counts.
// A workgroup is two waves, each with a tile of 64 lines x one segment: 65 values per line, staged through LDS
// so that the global reads are coalesced in both orientations and the walk reads its own line.
template <bool VERT, bool EDGES>
__global__ void __launch_bounds__(128) walk_kernel(const float* __restrict__ pred, int64_t ldp, const uint8_t* __restrict__ mask,
                                                   int64_t ldm, int H, int W, int inverse, Thr thr, int n_t, Summ sm,
                                                   u64* __restrict__ counts, uint8_t* __restrict__ maps) {
  constexpr int NK = EDGES ? 1 : TK;
  constexpr int dirA = VERT ? 1 : 0;            // top / left: value[c] / value[c + 1]; dirA + 2 is the inverse ratio
  __shared__ float tile[2][(SEG + 1) * 64];
  __shared__ uint32_t acc[2][NK], tacc[2];
  __shared__ float sth[MAX_T];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lines = VERT ? W : H, len = (VERT ? H : W) - 1;            // len >= 1: the host launches nothing else
  const int nseg = (len + SEG - 1) / SEG, nlg = (lines + 63) / 64;
  const long long t = (long long)blockIdx.x * 2 + wv;
  const bool live = t < (long long)nseg * nlg;                         // per wave
  const int seg = live ? (int)(t / nlg) : 0, line0 = live ? (int)(t % nlg) * 64 : 0, c0 = seg * SEG;
  const int k0 = blockIdx.y * NK;
  const int nk = n_t - k0 < NK ? n_t - k0 : NK;
  if (threadIdx.x < 2 * NK) acc[threadIdx.x / NK][threadIdx.x % NK] = 0;
  if (threadIdx.x < 2) tacc[threadIdx.x] = 0;
  stage_thresholds(thr, sth);

  // stage: T(line, p) = value at place c0 + p of the line, NaN outside the image; mb / mlast = the target's bits
  float* T = tile[wv];
  auto at = [&](int ln, int p) { return VERT ? p * 64 + ln : ln * (SEG + 1) + p; };
  const float nan = __builtin_nanf("");
  u64 mb = 0;
  uint32_t mlast = 0;
  if (live) {
    if (VERT) {
      const int x = line0 + lane;
      #pragma unroll 5
      for (int p = 0; p <= SEG; ++p) {
        const int y = c0 + p;
        const bool in = x < W && y < H;
        T[at(lane, p)] = in ? inv_depth(pred[(int64_t)y * ldp + x], inverse) : nan;
        const uint32_t m = in && mask ? mask[(int64_t)y * ldm + x] != 0 : 0;
        if (p < SEG) mb |= (u64)m << p; else mlast = m;
      }
    } else {
      const int x = c0 + lane;
      #pragma unroll 4
      for (int rr = 0; rr < 64; ++rr) {
        const int y = line0 + rr;
        const bool in = x < W && y < H;
        T[at(rr, lane)] = in ? inv_depth(pred[(int64_t)y * ldp + x], inverse) : nan;
        const u64 b = __ballot(in && mask ? mask[(int64_t)y * ldm + x] != 0 : false);
        if (lane == rr) mb = b;
      }
      const int y = line0 + lane, xl = c0 + SEG;
      const bool in = xl < W && y < H;
      T[at(lane, SEG)] = in ? inv_depth(pred[(int64_t)y * ldp + xl], inverse) : nan;
      mlast = in && mask ? mask[(int64_t)y * ldm + xl] != 0 : 0;
    }
  }
  __syncthreads();

  float f[NK];
  #pragma unroll
  for (int k = 0; k < NK; ++k) f[k] = sth[(k0 + k) & (MAX_T - 1)];
  const int line = line0 + lane;
  const bool mine = live && line < lines;
  const long long E = (long long)nseg * lines, slot = (long long)seg * lines + line;
  const long long plane = (long long)H * W;
  auto pixel = [&](int pos) { return VERT ? (long long)pos * W + line : (long long)line * W + pos; };

  float cur[2][NK];
  uint32_t cnt[2][NK];                          // runs closed inside the segment: their number | target bits there << 16
  uint32_t open[2] = {0, 0}, done[2] = {0, 0}, hset[2] = {0, 0}, ct[2] = {0, 0}, ht[2] = {0, 0}, tcnt[2] = {0, 0};
  int cpos[2] = {0, 0};
  #pragma unroll
  for (int d = 0; d < 2; ++d)
    #pragma unroll
    for (int k = 0; k < NK; ++k) { cur[d][k] = 0.0f; cnt[d][k] = 0; }

  const int ncell = !live ? 0 : (len - c0 < SEG ? len - c0 : SEG);
  float v0 = T[at(lane, 0)];
  for (int c = 0; c < ncell; ++c) {
    const float v1 = T[at(lane, c + 1)];
    const float r[2] = {v0 / v1, v1 / v0};
    const uint32_t m0 = (uint32_t)(mb >> c) & 1u, m1 = c + 1 < SEG ? (uint32_t)(mb >> (c + 1)) & 1u : mlast;
    const uint32_t tb[2] = {m0 & ~m1 & 1u, m1 & ~m0 & 1u};
    #pragma unroll
    for (int d = 0; d < 2; ++d) {
      tcnt[d] += tb[d];
      #pragma unroll
      for (int k = 0; k < NK; ++k) {
        if (k < nk) {
          const uint32_t bit = 1u << k;
          const bool e = r[d] > f[k], isopen = open[d] & bit, isdone = done[d] & bit;
          const bool take = e && (!isopen || r[d] > cur[d][k]);       // the first of equal maxima stays
          cur[d][k] = take ? r[d] : cur[d][k];
          if (take) ct[d] = (ct[d] & ~bit) | (tb[d] << k);
          if (EDGES && take) cpos[d] = c0 + c;
          if (!e && isopen) {
            const uint32_t tbit = (ct[d] >> k) & 1u;
            if (isdone) {
              cnt[d][k] += 1u | (tbit << 16);
              if (EDGES) maps[(dirA + 2 * d) * plane + pixel(cpos[d])] = 1;
            } else if (mine) {                                         // the head run ends here
              sm.head[((long long)d * n_t + k0 + k) * E + slot] = __float_as_uint(cur[d][k]);
              ht[d] |= tbit << k;
              hset[d] |= bit;
              if (EDGES) sm.hpos[(long long)d * E + slot] = cpos[d];
            }
          }
          open[d] = e ? (open[d] | bit) : (open[d] & ~bit);
          if (!e) done[d] |= bit;
        }
      }
    }
    v0 = v1;
  }

  if (mine) {
    #pragma unroll
    for (int d = 0; d < 2; ++d) {
      uint32_t tt = 0;
      #pragma unroll
      for (int k = 0; k < NK; ++k) {
        if (k < nk) {
          const uint32_t bit = 1u << k;
          const bool isopen = open[d] & bit, whole = isopen && !(done[d] & bit);
          const long long e = ((long long)d * n_t + k0 + k) * E + slot;
          const uint32_t tbit = (ct[d] >> k) & 1u;
          if (whole) {
            sm.head[e] = __float_as_uint(cur[d][k]);
            ht[d] |= tbit << k;
            if (EDGES) sm.hpos[(long long)d * E + slot] = cpos[d];
          } else if (!(hset[d] & bit)) {
            sm.head[e] = NONE;
          }
          sm.tail[e] = whole ? WHOLE : (isopen ? __float_as_uint(cur[d][k]) : NONE);
          if (isopen && !whole) {
            tt |= tbit << k;
            if (EDGES) sm.tpos[(long long)d * E + slot] = cpos[d];
          }
        }
      }
      if (!EDGES) sm.tbits[((long long)d * gridDim.y + blockIdx.y) * E + slot] = (ht[d] & 0xffffu) | (tt << 16);
    }
  }

  if (!EDGES) {                                 // at most 64 lanes x 32 runs x 2 waves per counter: 16 bits each
    #pragma unroll
    for (int d = 0; d < 2; ++d) {
      #pragma unroll
      for (int k = 0; k < NK; ++k)
        if (cnt[d][k]) atomicAdd(&acc[d][k], cnt[d][k]);
      if (tcnt[d]) atomicAdd(&tacc[d], tcnt[d]);
    }
    __syncthreads();
    if (threadIdx.x < 2 * NK) {
      const int d = threadIdx.x / NK, k = threadIdx.x % NK;
      if (k < nk) {
        u64* c3 = counts + ((long long)(k0 + k) * 4 + dirA + 2 * d) * 3;
        const uint32_t v = acc[d][k];
        if (v >> 16) atomicAdd(&c3[0], (u64)(v >> 16));
        if (tacc[d]) atomicAdd(&c3[1], (u64)tacc[d]);
        if (v & 0xffffu) atomicAdd(&c3[2], (u64)(v & 0xffffu));
      }
    }
  }
}

// One lane per line; blockIdx.y = direction of the pair * n_t + threshold.  The segments of the line in order:
// the run carried over from the segments before joins this segment's head, or ends at its first cell.
template <bool EDGES>
__global__ void __launch_bounds__(64) combine_kernel(Summ sm, int lines, int nseg, int n_t, int passes, int vert, int H, int W,
                                                     u64* __restrict__ counts, uint8_t* __restrict__ maps) {
  const int line = blockIdx.x * 64 + threadIdx.x;
  const int d = blockIdx.y / n_t, k = blockIdx.y % n_t, dir = (vert ? 1 : 0) + 2 * d;
  const long long E = (long long)nseg * lines;
  const uint32_t* head = sm.head + ((long long)d * n_t + k) * E;
  const uint32_t* tail = sm.tail + ((long long)d * n_t + k) * E;
  const uint32_t* tbits = EDGES ? nullptr : sm.tbits + ((long long)d * passes + k / TK) * E;
  const int kk = k % TK;
  uint8_t* map = EDGES ? maps + (long long)dir * H * W : nullptr;
  uint32_t runs = 0, both = 0;
  if (line < lines) {
    bool carry = false;
    float cv = 0.0f;
    uint32_t ctb = 0;
    int cp = 0;
    auto close = [&]() {
      ++runs;
      both += ctb;
      if (EDGES && (unsigned)cp < (unsigned)((vert ? H : W) - 1)) map[vert ? (long long)cp * W + line : (long long)line * W + cp] = 1;
      carry = false;
    };
    for (int s = 0; s < nseg; ++s) {
      const long long e = (long long)s * lines + line;
      const uint32_t h = head[e], tl = tail[e], tb = EDGES ? 0u : tbits[e];
      if (h != NONE) {
        const float hv = __uint_as_float(h);
        if (!carry || hv > cv) {                                       // the earlier of equal maxima stays
          cv = hv;
          ctb = (tb >> kk) & 1u;
          if (EDGES) cp = sm.hpos[(long long)d * E + e];
        }
        carry = true;
        if (tl == WHOLE) continue;
        close();
      } else if (carry) {
        close();
      }
      if (tl != NONE) {
        carry = true;
        cv = __uint_as_float(tl);
        ctb = (tb >> (16 + kk)) & 1u;
        if (EDGES) cp = sm.tpos[(long long)d * E + e];
      }
    }
    if (carry) close();
  }
  if (!EDGES) {
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) { runs += __shfl_xor(runs, o); both += __shfl_xor(both, o); }
    if (threadIdx.x == 0) {
      u64* c3 = counts + ((long long)k * 4 + dir) * 3;
      if (both) atomicAdd(&c3[0], (u64)both);
      if (runs) atomicAdd(&c3[2], (u64)runs);
    }
  }
}

// ---- host -------------------------------------------------------------------------------------------
int64_t al256(int64_t v) { return (v + 255) & ~(int64_t)255; }
int64_t nseg_for(int64_t len) { return (len + SEG - 1) / SEG; }
// summaries of one orientation: lines x segments of its maps
int64_t slots_h(int64_t H, int64_t W) { return H * nseg_for(W - 1); }
int64_t slots_v(int64_t H, int64_t W) { return W * nseg_for(H - 1); }
int64_t passes_for(int64_t n_t) { return (n_t + TK - 1) / TK; }
int64_t ws_bytes_for(int64_t H, int64_t W, int64_t n_t) {
  if (H < 1 || W < 1 || n_t < 1) return 256;
  const int64_t E = slots_h(H, W) + slots_v(H, W);
  // head + tail, target bits, places: each [2 directions][...][slots] of 4 bytes
  return 256 + 2 * al256(8 * n_t * E) + al256(8 * passes_for(n_t) * E) + 2 * al256(8 * E);
}
// [0]: rows (left, right), [1]: columns (top, bottom)
void ws_carve(void* ws, int64_t H, int64_t W, int64_t n_t, Summ o[2]) {
  const int64_t Eh = slots_h(H, W), Ev = slots_v(H, W), E = Eh + Ev, P = passes_for(n_t);
  char* p = (char*)ws;
  o[0].head = (uint32_t*)p;  o[1].head = o[0].head + 2 * n_t * Eh;   p += al256(8 * n_t * E);
  o[0].tail = (uint32_t*)p;  o[1].tail = o[0].tail + 2 * n_t * Eh;   p += al256(8 * n_t * E);
  o[0].tbits = (uint32_t*)p; o[1].tbits = o[0].tbits + 2 * P * Eh;   p += al256(8 * P * E);
  o[0].hpos = (int32_t*)p;   o[1].hpos = o[0].hpos + 2 * Eh;         p += al256(8 * E);
  o[0].tpos = (int32_t*)p;   o[1].tpos = o[0].tpos + 2 * Eh;
}

bool is_finite(double v) { return v == v && v != __builtin_inf() && v != -__builtin_inf(); }
// the largest float32 <= t
float floor_f32(double t) {
  float f = (float)t;
  if ((double)f > t) f = __builtin_nextafterf(f, -__builtin_inff());
  return f;
}
bool dims_ok(int H, int W) { return H >= 1 && W >= 1 && H <= DP_BOUNDARY_MAX_DIM && W <= DP_BOUNDARY_MAX_DIM; }

template <bool EDGES>
void launch_thinned(const float* pred, int64_t ldp, const uint8_t* mask, int64_t ldm, int H, int W, int inverse, const Thr& thr,
                    int n_t, Summ sm[2], u64* counts, uint8_t* maps, hipStream_t s) {
  const int passes = EDGES ? 1 : (int)passes_for(n_t);
  for (int vert = 0; vert < 2; ++vert) {
    const int lines = vert ? W : H, len = (vert ? H : W) - 1;
    if (len < 1) continue;
    const int nseg = (int)nseg_for(len);
    const long long tiles = (long long)nseg * ((lines + 63) / 64);
    const dim3 gw((unsigned)((tiles + 1) / 2), passes), gc((lines + 63) / 64, 2 * n_t);
    if (vert) hipLaunchKernelGGL((walk_kernel<true, EDGES>), gw, dim3(128), 0, s, pred, ldp, mask, ldm, H, W, inverse, thr, n_t, sm[1], counts, maps);
    else hipLaunchKernelGGL((walk_kernel<false, EDGES>), gw, dim3(128), 0, s, pred, ldp, mask, ldm, H, W, inverse, thr, n_t, sm[0], counts, maps);
    hipLaunchKernelGGL((combine_kernel<EDGES>), gc, dim3(64), 0, s, sm[vert], lines, nseg, n_t, passes, vert, H, W, counts, maps);
  }
}

}  // namespace

extern "C" int64_t dp_boundary_workspace_size(int32_t H, int32_t W, int32_t n_t) { return ws_bytes_for(H, W, n_t); }

extern "C" int dp_boundary_counts(const float* pred, int64_t ld_pred, const void* target, int64_t ld_target, int32_t target_kind,
                                  int32_t H, int32_t W, const double* thresholds, int32_t n_t, uint64_t* counts, void* ws,
                                  int64_t ws_bytes, dp_stream_t stream) {
  if (!pred || !target || !thresholds || !counts || !ws) return DP_ERR_ARG;
  const int kind = target_kind & ~DP_BOUNDARY_INVERSE, inverse = (target_kind & DP_BOUNDARY_INVERSE) != 0;
  if (target_kind < 0 || (kind != DP_BOUNDARY_DEPTH && kind != DP_BOUNDARY_MASK)) return DP_ERR_ARG;
  if (!dims_ok(H, W) || n_t < 1 || n_t > MAX_T || ld_pred < W || ld_target < W) return DP_ERR_SHAPE;
  Thr thr = {};
  for (int k = 0; k < n_t; ++k) {
    if (!is_finite(thresholds[k])) return DP_ERR_ARG;
    thr.f[k] = floor_f32(thresholds[k]);
  }
  if (ws_bytes < ws_bytes_for(H, W, n_t) || ((uintptr_t)ws & 3) || ((uintptr_t)counts & 7)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  u64* cnt = (u64*)counts;
  hipError_t e = hipMemsetAsync(cnt, 0, sizeof(u64) * 12 * n_t, s);
  if (e != hipSuccess) return (int)e;
  if (kind == DP_BOUNDARY_DEPTH) {
    const dim3 g((W + 255) / 256, (H + PL_ROWS - 1) / PL_ROWS);
    hipLaunchKernelGGL(plain_counts_kernel, g, dim3(256), 0, s, pred, ld_pred, (const float*)target, ld_target, H, W, inverse, thr,
                       n_t, cnt);
  } else {
    Summ sm[2];
    ws_carve(ws, H, W, n_t, sm);
    launch_thinned<false>(pred, ld_pred, (const uint8_t*)target, ld_target, H, W, inverse, thr, n_t, sm, cnt, nullptr, s);
  }
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_boundary_edges(const float* depth, int64_t ld, int32_t H, int32_t W, double t, int32_t thinned, uint8_t* maps,
                                 void* ws, int64_t ws_bytes, dp_stream_t stream) {
  if (!depth || !maps || !ws || !is_finite(t)) return DP_ERR_ARG;
  if (!dims_ok(H, W) || ld < W) return DP_ERR_SHAPE;
  if (ws_bytes < ws_bytes_for(H, W, 1) || ((uintptr_t)ws & 3)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  Thr thr = {};
  thr.f[0] = floor_f32(t);
  if (!thinned) {
    hipLaunchKernelGGL(plain_edges_kernel, dim3((W + 255) / 256, H), dim3(256), 0, s, depth, ld, H, W, thr.f[0], maps);
  } else {
    hipError_t e = hipMemsetAsync(maps, 0, (size_t)4 * H * W, s);
    if (e != hipSuccess) return (int)e;
    Summ sm[2];
    ws_carve(ws, H, W, 1, sm);
    launch_thinned<true>(depth, ld, nullptr, 0, H, W, 0, thr, 1, sm, nullptr, maps, s);
  }
  DP_CHECK_LAUNCH();
  return 0;
}
