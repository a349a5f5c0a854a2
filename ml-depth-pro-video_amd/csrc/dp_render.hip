// Point-cloud views (include/dp_mi355x.h, "Point-cloud views"): z-buffered square splats of the
// cloud from up to four perspective cameras and the top-down plan, for gfx950.
//   bounds    per-axis min / max of the finite live rows (and of the plan's shown rows) by the wave-reduced key
//             atomics of dp_points.h
//   camera    one thread: every view's camera record from the bounds, on the device
//   project   one pass over the cloud for all views: a row is read once, projected into every view, and its key
//             (float32 depth bits << 32 | row) goes to the view's centre buffer with one 64-bit atomicMin
//   resolve   per output pixel the smallest key of the size x size window of the centre buffer (a row pass and a column
//             pass in LDS per tile), the colour of its row, RGB stored a dword at a time
// The gather in `resolve` equals scattering size^2 z-tested pixels per point, at one atomic per point.  All arithmetic
// is fp64 in the order tests/render_numpy.py writes it, contraction off; the picture does not depend on the order the
// hardware serves the rows (the key's low word is the row).
#include "dp_points.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAXV = DP_RENDER_MAX_VIEWS + 1;      // the perspective views and the plan
constexpr int CAM = DP_RENDER_CAMERA_DOUBLES;
constexpr int HEADER_BYTES = 256;
constexpr int MAX_BLOCKS = 1024;
constexpr int TX = 64, TY = 16;                    // output pixels of one resolve workgroup
constexpr int HALO = DP_RENDER_MAX_SIZE - 1;
constexpr u64 EMPTY = ~0ull;
// bench-only switches (dp_render_debug_flags): 1 no plain-load filter, 2 no in-wave agreement, 4 / 8 / 16 leave out
// bounds + cameras / project / resolve (what they would have written is whatever an earlier call left)
constexpr int F_NO_FILTER = 1, F_NO_WAVE = 2, F_SKIP_BOUNDS = 4, F_SKIP_PROJECT = 8, F_SKIP_RESOLVE = 16;
int g_flags = 0;

struct Header {
  u64 mm[12];                // (min, max) keys: x, y, z of the finite rows; -x, z, y of the plan's shown rows
  uint32_t cnt[4];           // finite, non-finite, shown
  uint32_t view[MAXV][4];    // drawn, clipped, outside, covered pixels
};
static_assert(sizeof(Header) <= HEADER_BYTES, "header");

struct Views {
  double v[DP_RENDER_MAX_VIEWS][7];                // front, up, zoom
  double min_height, t;
  int n, plan, has_min, W, H;
};
struct Colours { uint8_t c[2][3]; };

__global__ void rd_init_kernel(Header* hd) {
  const int t = threadIdx.x;
  if (t < 12) hd->mm[t] = (t & 1) ? 0ull : EMPTY;
  if (t < 4) hd->cnt[t] = 0;
  if (t < MAXV * 4) hd->view[t >> 2][t & 3] = 0;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ void __launch_bounds__(256) rd_bounds_kernel(const double* __restrict__ pts, const int32_t* n_dev, int n_max, int has_min,
                                                        double min_h, Header* hd) {
  const int n = live_n(n_dev, n_max);
  u64 mn[6], mx[6];
  #pragma unroll
  for (int a = 0; a < 6; ++a) { mn[a] = EMPTY; mx[a] = 0; }
  uint32_t c_fin = 0, c_non = 0, c_shown = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    if (!finite3(x, y, z)) { ++c_non; continue; }
    ++c_fin;
    const u64 k[3] = {okey(x), okey(y), okey(z)};
    #pragma unroll
    for (int a = 0; a < 3; ++a) { mn[a] = k[a] < mn[a] ? k[a] : mn[a]; mx[a] = k[a] > mx[a] ? k[a] : mx[a]; }
    if (!has_min || y >= min_h) {
      ++c_shown;
      const u64 s[3] = {okey(-x), k[2], k[1]};
      #pragma unroll
      for (int a = 0; a < 3; ++a) { mn[3 + a] = s[a] < mn[3 + a] ? s[a] : mn[3 + a]; mx[3 + a] = s[a] > mx[3 + a] ? s[a] : mx[3 + a]; }
    }
  }
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) wave_minmax<6>(mn, mx, o);
  c_fin = wave_sum(c_fin); c_non = wave_sum(c_non); c_shown = wave_sum(c_shown);
  if ((threadIdx.x & 63) == 0) {
    if (c_fin) { flush_minmax<6>(hd->mm, mn, mx); atomicAdd(&hd->cnt[0], c_fin); }
    if (c_non) atomicAdd(&hd->cnt[1], c_non);
    if (c_shown) atomicAdd(&hd->cnt[2], c_shown);
  }
}

__device__ __forceinline__ double norm3(const double* a) { return __builtin_sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }
__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
// the bounds' extent: max over the axes of (max - min); 0 without a finite row
__device__ __forceinline__ double extent_of(const Header* hd, double* center) {
  double ext = 0.0;
  for (int a = 0; a < 3; ++a) {
    const double lo = unkey(hd->mm[2 * a]), hi = unkey(hd->mm[2 * a + 1]);
    const double d = hi - lo;
    if (center) center[a] = (lo + hi) / 2.0;
    ext = (a == 0 || d > ext) ? d : ext;
  }
  return ext;
}

// one thread: the camera records of every view, perspective first, the plan last
__global__ void rd_camera_kernel(Views vs, const Header* hd, double* __restrict__ cams) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double Wd = (double)vs.W, Hd = (double)vs.H;
  for (int v = 0; v < vs.n; ++v) {
    double* c = cams + (long long)v * CAM;
    for (int k = 0; k < CAM; ++k) c[k] = 0.0;
    c[21] = vs.t * (Wd / Hd);
    c[22] = vs.t;
    if (hd->cnt[0] == 0) { c[1] = 1.0; continue; }
    double center[3];
    const double ext = extent_of(hd, center);
    c[17] = ext;
    c[18] = center[0]; c[19] = center[1]; c[20] = center[2];
    if (!(ext > 0.0)) { c[1] = 1.0; continue; }
    const double* front = vs.v[v];
    const double* up = vs.v[v] + 3;
    const double zoom = vs.v[v][6];
    const double fn = norm3(front);
    const double f[3] = {front[0] / fn, front[1] / fn, front[2] / fn};
    const double dist = zoom * ext / vs.t;
    const double F[3] = {-f[0], -f[1], -f[2]};
    double s[3], u[3];
    cross3(F, up, s);
    const double sn = norm3(s);
    s[0] = s[0] / sn; s[1] = s[1] / sn; s[2] = s[2] / sn;
    cross3(s, F, u);
    const double na = 0.01 * ext, nb = dist - 3.0 * ext;
    for (int a = 0; a < 3; ++a) {
      c[2 + a] = center[a] + f[a] * dist;
      c[5 + a] = s[a];
      c[8 + a] = u[a];
      c[11 + a] = F[a];
    }
    c[14] = nb > na ? nb : na;
    c[15] = dist + 3.0 * ext;
    c[16] = dist;
  }
  if (vs.plan) {
    double* c = cams + (long long)vs.n * CAM;
    for (int k = 0; k < CAM; ++k) c[k] = 0.0;
    c[0] = 1.0;
    c[6] = vs.has_min ? vs.min_height : __builtin_nan("");
    c[7] = (Wd - 1.0) / 2.0;
    c[8] = (Hd - 1.0) / 2.0;
    if (hd->cnt[2] == 0) { c[1] = 1.0; return; }
    const double x0 = unkey(hd->mm[6]), x1 = unkey(hd->mm[7]), z0 = unkey(hd->mm[8]), z1 = unkey(hd->mm[9]);
    double span_x = x1 - x0, span_z = z1 - z0;
    span_x = span_x == 0.0 ? 1.0 : span_x;
    span_z = span_z == 0.0 ? 1.0 : span_z;
    c[2] = (x0 + x1) / 2.0;
    c[3] = (z0 + z1) / 2.0;
    const double sa = (Wd - 1.0) / span_x, sb = (Hd - 1.0) / span_z;
    c[4] = sb < sa ? sb : sa;
    c[5] = unkey(hd->mm[11]);
  }
}

// stride: u64 words of one view's centre buffer, (H + size - 1) rows of BW = W + size - 1
__global__ void __launch_bounds__(256) rd_project_kernel(const double* __restrict__ pts, const int32_t* n_dev, int n_max,
                                                         const double* __restrict__ cams, int nv, int W, int H, int size,
                                                         u64* __restrict__ centre, long long stride, int flags, Header* hd) {
  __shared__ double sc[MAXV * CAM];
  for (int k = threadIdx.x; k < nv * CAM; k += 256) sc[k] = cams[k];
  __syncthreads();
  const int n = live_n(n_dev, n_max);
  const int R = (size - 1) / 2, BW = W + size - 1;
  const double Wd = (double)W, Hd = (double)H, aspect = Wd / Hd;
  const double x_lo = (double)(-R), x_hi = (double)(W - 1 + R), y_lo = (double)(-R), y_hi = (double)(H - 1 + R);
  uint32_t cnt[MAXV][3];
  #pragma unroll
  for (int v = 0; v < MAXV; ++v) cnt[v][0] = cnt[v][1] = cnt[v][2] = 0;
  for (long long base = (long long)blockIdx.x * 256; base < n; base += (long long)gridDim.x * 256) {   // uniform per workgroup
    const long long i = base + threadIdx.x;
    double x = 0.0, y = 0.0, z = 0.0;
    bool fin = false;
    if (i < n) {
      x = pts[3 * i]; y = pts[3 * i + 1]; z = pts[3 * i + 2];
      fin = finite3(x, y, z);
    }
    #pragma unroll
    for (int v = 0; v < MAXV; ++v) {
      if (v >= nv) break;
      const double* c = sc + v * CAM;
      bool issue = false;
      u64 key = EMPTY;
      long long addr = -1 - (long long)threadIdx.x;              // no two lanes alike
      if (fin && c[1] == 0.0) {
        bool inside;
        double fx = 0.0, fy = 0.0, d = 0.0;
        if (c[0] == 0.0) {
          const double q0 = x - c[2], q1 = y - c[3], q2 = z - c[4];
          const double xc = c[5] * q0 + c[6] * q1 + c[7] * q2;
          const double yc = c[8] * q0 + c[9] * q1 + c[10] * q2;
          const double w = c[11] * q0 + c[12] * q1 + c[13] * q2;
          inside = w >= c[14] && w <= c[15];
          if (inside) {                                          // w >= near > 0: nothing divides by zero
            const double dy = w * c[22];
            const double dx = dy * aspect;
            fx = __builtin_floor((xc / dx * 0.5 + 0.5) * Wd);
            fy = __builtin_floor((0.5 - yc / dy * 0.5) * Hd);
            d = w;
          }
        } else {
          inside = !(c[6] == c[6]) || y >= c[6];
          fx = __builtin_floor(((-x) - c[2]) * c[4] + c[7] + 0.5);
          fy = __builtin_floor(c[8] - (z - c[3]) * c[4] + 0.5);
          d = c[5] - y;
        }
        if (!inside) ++cnt[v][1];
        else if (!(fx >= x_lo && fx <= x_hi && fy >= y_lo && fy <= y_hi)) ++cnt[v][2];
        else {
          ++cnt[v][0];
          issue = true;
          key = ((u64)__float_as_uint((float)d) << 32) | (u64)i;
          addr = (long long)v * stride + (long long)((int)fy + R) * BW + ((int)fx + R);
        }
      }
      if (!(flags & F_NO_WAVE)) {                                // lanes on one pixel: the larger key of a pair stays home
        bool drop = false;
        #pragma unroll
        for (int o = 1; o <= 4; o <<= 1) {
          const long long ta = __shfl_xor(addr, o);
          const u64 tk = __shfl_xor(key, o);
          drop |= ta == addr && tk < key;
        }
        issue = issue && !drop;
      }
      if (issue) {
        if ((flags & F_NO_FILTER) || centre[addr] > key) atomicMin(&centre[addr], key);
      }
    }
  }
  #pragma unroll
  for (int v = 0; v < MAXV; ++v) {
    if (v >= nv) break;
    #pragma unroll
    for (int k = 0; k < 3; ++k) {
      const uint32_t s = wave_sum(cnt[v][k]);
      if ((threadIdx.x & 63) == 0 && s) atomicAdd(&hd->view[v][k], s);
    }
  }
}

// grid (tiles_x * tiles_y, views); view v goes to out + v * H * W * 3, or with `sheet` into its quadrant of 2H x 2W
__global__ void __launch_bounds__(256) rd_resolve_kernel(const u64* __restrict__ centre, long long stride, const uint8_t* __restrict__ cols,
                                                         int n_max, int W, int H, int size, int tiles_x, int sheet, int plan_view,
                                                         Colours bg, uint8_t* __restrict__ out, Header* hd) {
  __shared__ u64 in[TY + HALO][TX + HALO];
  __shared__ u64 rowmin[TY + HALO][TX];
  __shared__ uint8_t px[TY][TX * 3];
  __shared__ uint32_t red[4];
  const int v = blockIdx.y;
  const int tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * TX, ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * TY;
  const int BW = W + size - 1, BH = H + size - 1;
  const int in_w = TX + size - 1, in_h = TY + size - 1;
  const u64* buf = centre + (long long)v * stride;
  for (int idx = threadIdx.x; idx < in_h * in_w; idx += 256) {
    const int r = idx / in_w, c = idx - r * in_w;
    const int gy = ty0 + r, gx = tx0 + c;
    in[r][c] = (gy < BH && gx < BW) ? buf[(long long)gy * BW + gx] : EMPTY;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < in_h * TX; idx += 256) {
    const int r = idx / TX, c = idx - r * TX;
    u64 m = EMPTY;
    for (int k = 0; k < size; ++k) { const u64 t = in[r][c + k]; m = t < m ? t : m; }
    rowmin[r][c] = m;
  }
  __syncthreads();
  const uint8_t* b = bg.c[v == plan_view ? 1 : 0];
  uint32_t covered = 0;
  for (int idx = threadIdx.x; idx < TY * TX; idx += 256) {
    const int r = idx / TX, c = idx - r * TX;
    u64 m = EMPTY;
    for (int k = 0; k < size; ++k) { const u64 t = rowmin[r + k][c]; m = t < m ? t : m; }
    uint8_t c0 = b[0], c1 = b[1], c2 = b[2];
    if (m != EMPTY && n_max > 0) {
      const size_t row = row_of((uint32_t)m, n_max);
      c0 = c1 = c2 = 128;
      if (cols) { c0 = cols[3 * row]; c1 = cols[3 * row + 1]; c2 = cols[3 * row + 2]; }
      covered += tx0 + c < W && ty0 + r < H;
    }
    px[r][3 * c] = c0; px[r][3 * c + 1] = c1; px[r][3 * c + 2] = c2;
  }
  __syncthreads();
  // the tile's rows, a dword at a time where a whole dword lies inside the row's bytes, single bytes at its ends
  const int wvalid = W - tx0 < TX ? W - tx0 : TX;
  const int nbytes = wvalid * 3;
  const long long OW = sheet ? 2LL * W : W;
  const long long ox = sheet ? (long long)(v & 1) * W : 0, oy = sheet ? (long long)(v >> 1) * H : 0;
  uint8_t* vout = out + (sheet ? 0LL : (long long)v * H * W * 3);
  constexpr int WORDS = TX * 3 / 4 + 1;
  for (int idx = threadIdx.x; idx < TY * WORDS; idx += 256) {
    const int r = idx / WORDS, j = idx - r * WORDS;
    if (ty0 + r >= H) continue;
    uint8_t* p0 = vout + ((oy + ty0 + r) * OW + ox + tx0) * 3;
    const int lead = (int)((uintptr_t)p0 & 3);
    const int off = 4 * j - lead;                                // byte offset of this dword within the row's bytes
    if (off >= 0 && off + 4 <= nbytes) {
      const uint32_t wv = (uint32_t)px[r][off] | ((uint32_t)px[r][off + 1] << 8) | ((uint32_t)px[r][off + 2] << 16) |
                          ((uint32_t)px[r][off + 3] << 24);
      *(uint32_t*)(p0 + off) = wv;
    } else {
      for (int k = 0; k < 4; ++k)
        if (off + k >= 0 && off + k < nbytes) p0[off + k] = px[r][off + k];
    }
  }
  covered = wave_sum(covered);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = covered;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t s = red[0] + red[1] + red[2] + red[3];
    if (s) atomicAdd(&hd->view[v][3], s);
  }
}

__global__ void rd_stats_kernel(const Header* hd, int nv, double* __restrict__ stats) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int k = 0; k < DP_RENDER_STATS; ++k) stats[k] = 0.0;
  stats[DP_RENDER_STAT_LIVE] = (double)hd->cnt[0] + (double)hd->cnt[1];
  stats[DP_RENDER_STAT_NONFINITE] = (double)hd->cnt[1];
  stats[DP_RENDER_STAT_DEGENERATE] = (hd->cnt[0] == 0 || !(extent_of(hd, nullptr) > 0.0)) ? 1.0 : 0.0;
  stats[DP_RENDER_STAT_ERROR] = hd->cnt[1] ? 1.0 : 0.0;
  for (int v = 0; v < nv; ++v)
    for (int k = 0; k < 4; ++k) stats[DP_RENDER_STAT_VIEWS + 4 * v + k] = (double)hd->view[v][k];
}

inline bool finite_host(double v) { return v == v && v - v == 0.0; }
inline bool dims_ok(int32_t W, int32_t H) { return W >= 1 && H >= 1 && (int64_t)W * H < ((int64_t)1 << 31); }
inline bool size_ok(int32_t size) { return size >= 1 && size <= DP_RENDER_MAX_SIZE && (size & 1); }
inline int64_t centre_words(int32_t W, int32_t H, int32_t size) {
  return al256((int64_t)(H + size - 1) * (W + size - 1) * 8) / 8;
}

// the host checks of a view list; fills vs
bool views_ok(const double* views, int32_t n_views, int32_t plan, double min_height, int32_t W, int32_t H, double t, Views& vs) {
  if (n_views < 0 || n_views > DP_RENDER_MAX_VIEWS || plan < 0 || plan > 2 || (n_views == 0 && !plan)) return false;
  if (n_views > 0 && !views) return false;
  if (!finite_host(t) || !(t > 0.0)) return false;
  if (plan == 2 && !finite_host(min_height)) return false;
  for (int v = 0; v < n_views; ++v) {
    const double* p = views + 7 * v;
    for (int k = 0; k < 7; ++k) {
      if (!finite_host(p[k])) return false;
      vs.v[v][k] = p[k];
    }
    const double cx = p[1] * p[5] - p[2] * p[4], cy = p[2] * p[3] - p[0] * p[5], cz = p[0] * p[4] - p[1] * p[3];
    if ((p[0] == 0.0 && p[1] == 0.0 && p[2] == 0.0) || (p[3] == 0.0 && p[4] == 0.0 && p[5] == 0.0)) return false;
    if (!(p[6] > 0.0)) return false;
    if (cx == 0.0 && cy == 0.0 && cz == 0.0) return false;      // up parallel to front
  }
  vs.n = n_views; vs.plan = plan ? 1 : 0; vs.has_min = plan == 2; vs.min_height = plan == 2 ? min_height : 0.0;
  vs.t = t; vs.W = W; vs.H = H;
  return true;
}

void launch_cameras(const double* points, const int32_t* count, int32_t n, const Views& vs, Header* hd, double* cams, hipStream_t s) {
  hipLaunchKernelGGL(rd_init_kernel, dim3(1), dim3(64), 0, s, hd);
  hipLaunchKernelGGL(rd_bounds_kernel, dim3(grid_for(n, MAX_BLOCKS)), dim3(256), 0, s, points, count, n, vs.has_min, vs.min_height, hd);
  hipLaunchKernelGGL(rd_camera_kernel, dim3(1), dim3(64), 0, s, vs, (const Header*)hd, cams);
}
}  // namespace

extern "C" int dp_render_debug_flags(int flags) {
  const int old = g_flags;
  g_flags = flags;
  return old;
}

extern "C" int64_t dp_render_workspace_size(int32_t W, int32_t H, int32_t size, int32_t n_views) {
  if (!dims_ok(W, H) || !size_ok(size) || n_views < 1 || n_views > MAXV) return 0;
  return HEADER_BYTES + (int64_t)n_views * centre_words(W, H, size) * 8;
}

extern "C" int dp_render_cameras(const double* points, const int32_t* count, int32_t n, const double* views, int32_t n_views,
                                 int32_t plan, double min_height, int32_t W, int32_t H, double tan_half_fov, double* cameras_out,
                                 double* stats_out, void* workspace, int64_t workspace_bytes, dp_stream_t stream) {
  if (!points || !cameras_out || !stats_out || n < 0 || !dims_ok(W, H)) return DP_ERR_ARG;
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < HEADER_BYTES) return DP_ERR_ARG;
  Views vs;
  if (!views_ok(views, n_views, plan, min_height, W, H, tan_half_fov, vs)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  Header* hd = (Header*)workspace;
  launch_cameras(points, count, n, vs, hd, cameras_out, s);
  hipLaunchKernelGGL(rd_stats_kernel, dim3(1), dim3(64), 0, s, (const Header*)hd, 0, stats_out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_render_points(const double* points, const uint8_t* colors, const int32_t* count, int32_t n, const double* views,
                                int32_t n_views, int32_t plan, double min_height, int32_t W, int32_t H, int32_t size,
                                const uint8_t* background, double tan_half_fov, int32_t sheet, uint8_t* image_out,
                                double* cameras_out, double* stats_out, void* workspace, int64_t workspace_bytes,
                                dp_stream_t stream) {
  if (!points || !background || !image_out || !cameras_out || !stats_out || n < 0) return DP_ERR_ARG;
  if (!dims_ok(W, H) || !size_ok(size)) return DP_ERR_ARG;
  Views vs;
  if (!views_ok(views, n_views, plan, min_height, W, H, tan_half_fov, vs)) return DP_ERR_ARG;
  if (sheet && (n_views != DP_RENDER_MAX_VIEWS || plan)) return DP_ERR_ARG;
  const int nv = n_views + (plan ? 1 : 0);
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < dp_render_workspace_size(W, H, size, nv)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  Header* hd = (Header*)ws;
  u64* centre = (u64*)(ws + HEADER_BYTES);
  const long long stride = centre_words(W, H, size);
  const int flags = g_flags;
  if (!(flags & F_SKIP_BOUNDS)) launch_cameras(points, count, n, vs, hd, cameras_out, s);
  if (!(flags & F_SKIP_PROJECT)) {
    if (hipMemsetAsync(centre, 0xff, (size_t)stride * 8 * nv, s) != hipSuccess) return (int)hipGetLastError();
    hipLaunchKernelGGL(rd_project_kernel, dim3(grid_for(n, MAX_BLOCKS)), dim3(256), 0, s, points, count, n, (const double*)cameras_out, nv,
                       W, H, size, centre, stride, flags, hd);
  }
  if (!(flags & F_SKIP_RESOLVE)) {
    const int tiles_x = (W + TX - 1) / TX, tiles_y = (H + TY - 1) / TY;
    Colours bg;
    for (int k = 0; k < 6; ++k) bg.c[k / 3][k % 3] = background[k];
    hipLaunchKernelGGL(rd_resolve_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)nv), dim3(256), 0, s, (const u64*)centre, stride,
                       colors, n, W, H, size, tiles_x, sheet ? 1 : 0, plan ? n_views : -1, bg, image_out, hd);
  }
  hipLaunchKernelGGL(rd_stats_kernel, dim3(1), dim3(64), 0, s, (const Header*)hd, nv, stats_out);
  DP_CHECK_LAUNCH();
  return 0;
}
