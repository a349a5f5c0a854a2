// Shape overlays on the plan view (include/dp_mi355x.h, "Shape overlays on the plan view"): the
// fitted rectangles and circles stroked on the plan picture of dp_render.hip, each with its number, for gfx950.
//   flags     per row of the shapes table: is it a circle; the header's counters are cleared
//   (scan)    the flag scan of dp_points.h numbers the circles in table order
//   records   one thread per shape: a table row and the device camera record become a pixel-space record (centre, half
//             sides or radius, cos, sin, colour, number, the boxes of the stroke and of the label, flags)
//   draw      one workgroup per 64 x 16 tile, in place: the records are walked in chunks of 256, each thread tests one
//             record's box against the tile, the survivors are compacted into LDS in list order (ballot prefix), and
//             every pixel of the tile walks that list and blends; all chunks for the strokes, then all for the labels
//   stats     the header's counters as fp64
// All arithmetic is fp64 in the order tests/overlay_numpy.py writes it, contraction off.  No list can overflow (a chunk
// has as many slots as records), no workgroup waits on another, a tile that no record touches is not written.
#include "dp_points.h"

#pragma clang fp contract(off)

namespace {

constexpr int REC = DP_OVERLAY_RECORD_DOUBLES;
constexpr int HEADER_BYTES = 256;
constexpr int MAX_BLOCKS = 1024;
constexpr int TX = 64, TY = 16;                    // the tile of dp_render.hip's resolve
constexpr int NT = 256, PER = TX * TY / NT;        // pixels per thread
constexpr double PI = 3.14159265358979323846;
constexpr int F_STROKE = 1, F_LABEL = 2, F_DROPPED = 4, F_SKIPPED = 8;
__constant__ uint8_t FONT[10][7] = DP_OVERLAY_FONT;
// bench-only switches (dp_overlay_debug_flags): 1 leaves out flags + scan + records, 2 leaves out draw (what they would
// have written, the header's counters included, is whatever an earlier call left)
constexpr int F_SKIP_RECORDS = 1, F_SKIP_DRAW = 2;
int g_flags = 0;

struct Header {
  int32_t nr, degenerate;
  uint32_t nc;                                     // the scan's total: the circles
  uint32_t cnt[5];                                 // rectangles drawn, circles drawn, skipped, off-screen, labels dropped
  uint32_t painted, error;
};
static_assert(sizeof(Header) <= HEADER_BYTES, "header");

struct Palette { uint8_t c[16][3]; };
struct Cam { double cx, cz, scale, hw, hh; bool ok; };

__device__ __forceinline__ Cam camera_of(const double* __restrict__ c) {
  Cam k;
  k.cx = c[2]; k.cz = c[3]; k.scale = c[4]; k.hw = c[7]; k.hh = c[8];
  k.ok = c[0] == 1.0 && c[1] == 0.0 && fin(k.cx) && fin(k.cz) && fin(k.scale) && fin(k.hw) && fin(k.hh);
  return k;
}

// grid over the table's rows: the circle flags; thread 0 clears the header and settles the rectangle count
__global__ void __launch_bounds__(256) ov_flags_kernel(const double* __restrict__ shapes, const int32_t* ncl, int max_clusters,
                                                       const int32_t* n_rects, int max_rects, const double* __restrict__ cam,
                                                       uint8_t* __restrict__ flag, Header* hd) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const bool ok = camera_of(cam).ok;
    hd->nr = ok ? live_n(n_rects, max_rects) : 0;
    hd->degenerate = ok ? 0 : 1;
    hd->nc = 0;
    for (int k = 0; k < 5; ++k) hd->cnt[k] = 0;
    hd->painted = 0;
    hd->error = ok ? 0u : 2u;
  }
  const int k = live_n(ncl, max_clusters);
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < k; c += (long long)gridDim.x * 256) flag[c] = shapes[16 * c] == 2.0;
}

// One record.  geo: X, Y in pixels are made here from (u, v); p0, p1: w, h (rectangle) or r (circle); ang in degrees.
__device__ __forceinline__ void write_record(double* __restrict__ o, int kind, double u, double v, double p0, double p1, double ang,
                                             const Cam& cam, const uint8_t* col, long long number, double t, int L, int W, int H,
                                             Header* hd) {
  const bool rect = kind == 1;
  const double colour = (double)((uint32_t)col[0] | ((uint32_t)col[1] << 8) | ((uint32_t)col[2] << 16));
  bool skip = !(fin(u) && fin(v) && fin(p0) && fin(p1) && fin(ang)) || p0 < 0.0 || p1 < 0.0;
  double X = 0.0, Y = 0.0, a = 0.0, b = 0.0, c = 1.0, s = 0.0, ex = 0.0, ey = 0.0;
  if (!skip) {
    X = (u - cam.cx) * cam.scale + cam.hw;
    Y = cam.hh - (v - cam.cz) * cam.scale;
    if (rect) {
      a = p0 * cam.scale / 2.0;
      b = p1 * cam.scale / 2.0;
      const double rad = ang * PI / 180.0;
      c = cos(rad);
      s = sin(rad);
    } else {
      a = p0 * cam.scale;
    }
    if (rect) {
      const double ac = __builtin_fabs(c), as = __builtin_fabs(s);
      ex = ac * (a + t) + as * (b + t);
      ey = as * (a + t) + ac * (b + t);
    } else {
      ex = ey = a + t;
    }
    skip = !(fin(X) && fin(Y) && fin(a) && fin(b) && fin(ex) && fin(ey));
  }
  for (int k = 0; k < REC; ++k) o[k] = 0.0;
  o[0] = (double)kind;
  o[8] = colour;
  o[9] = (double)number;
  o[12] = o[13] = o[16] = o[17] = -1.0;
  int flags = 0;
  if (skip) {
    flags = F_SKIPPED;
  } else {
    const double x0 = __builtin_floor(X - ex), x1 = __builtin_ceil(X + ex), y0 = __builtin_floor(Y - ey), y1 = __builtin_ceil(Y + ey);
    const double wm = (double)(W - 1), hm = (double)(H - 1);
    if (x1 >= 0.0 && x0 <= wm && y1 >= 0.0 && y0 <= hm) flags |= F_STROKE;
    o[2] = X; o[3] = Y; o[4] = a; o[5] = b; o[6] = c; o[7] = s;
    o[10] = x0; o[11] = y0; o[12] = x1; o[13] = y1;
    if (L > 0) {
      if (number > 9999) {
        flags |= F_DROPPED;
      } else {
        const int nd = number > 999 ? 4 : (number > 99 ? 3 : (number > 9 ? 2 : 1));
        const int bw = (6 * nd - 1) * L, bh = 7 * L;
        const double lx = __builtin_floor(X + 0.5) - (double)(bw / 2), ly = __builtin_floor(Y + 0.5) - (double)(bh / 2);
        const double l0 = lx - (double)L, l1 = ly - (double)L, l2 = lx + (double)(bw - 1 + L), l3 = ly + (double)(bh - 1 + L);
        if (l2 >= 0.0 && l0 <= wm && l3 >= 0.0 && l1 <= hm) flags |= F_LABEL;
        o[14] = l0; o[15] = l1; o[16] = l2; o[17] = l3;
        o[18] = (double)nd;
      }
    }
  }
  o[1] = (double)flags;
  const bool drawn = (flags & (F_STROKE | F_LABEL)) != 0;
  if (skip) { atomicAdd(&hd->cnt[2], 1u); atomicOr(&hd->error, 1u); }
  else if (!drawn) atomicAdd(&hd->cnt[3], 1u);
  else atomicAdd(&hd->cnt[rect ? 0 : 1], 1u);
  if (flags & F_DROPPED) atomicAdd(&hd->cnt[4], 1u);
}

__global__ void __launch_bounds__(256) ov_rect_records_kernel(const double* __restrict__ rects, const double* __restrict__ camrec,
                                                              Palette pal, double t, int L, int W, int H, double* __restrict__ rec,
                                                              Header* hd) {
  const int nr = hd->nr;
  const Cam cam = camera_of(camrec);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nr; i += (long long)gridDim.x * 256) {
    const double* r = rects + 8 * i;
    write_record(rec + REC * i, 1, r[0], r[1], r[2], r[3], r[4], cam, pal.c[i & 7], i + 1, t, L, W, H, hd);
  }
}

// third step of the flag scan: circle k of the table, in table order
__global__ void __launch_bounds__(256) ov_circle_records_kernel(const double* __restrict__ shapes, const int32_t* ncl, int max_clusters,
                                                                const uint8_t* __restrict__ flag, const uint32_t* __restrict__ bc,
                                                                const double* __restrict__ camrec, Palette pal, double t, int L, int W,
                                                                int H, double* __restrict__ rec, Header* hd) {
  __shared__ uint32_t wsum[4];
  if (hd->degenerate) return;
  const int n = live_n(ncl, max_clusters);
  const long long nr = hd->nr;
  const Cam cam = camera_of(camrec);
  const long long tile = (long long)blockIdx.x * SCAN_TILE;
  uint32_t run = bc[blockIdx.x];
  for (int r = 0; r < SCAN_ITEMS && tile + r * 256 < n; ++r) {
    const long long c = tile + r * 256 + threadIdx.x;
    const uint32_t f = c < n ? flag[c] : 0u;
    uint32_t tot = 0;
    const long long k = run + block_excl_scan(f, wsum, &tot);
    if (f) {
      const double* row = shapes + 16 * c;
      write_record(rec + REC * (nr + k), 2, row[8], row[9], row[10], 0.0, 0.0, cam, pal.c[8 + (k & 7)], nr + k + 1, t, L, W, H, hd);
    }
    run += tot;
  }
}

struct Stroke { double X, Y, c, s, a, b; uint32_t col, kind; int x0, x1, y0, y1; };   // the stroke box, cut to the tile
struct Label { int lx, ly; uint32_t col, digits; };        // digits: four nibbles, the most significant digit lowest; count << 16
union Slot { Stroke s; Label l; };

__device__ __forceinline__ uint32_t blend1(uint32_t p, uint32_t c, uint32_t A) { return (A * c + (255u - A) * p + 127u) / 255u; }

// the survivors of one chunk, in list order: slot of this thread's record (keep), the chunk's count in *total
__device__ __forceinline__ int compact_slot(bool keep, uint32_t* wcnt, int* total) {
  const u64 m = __ballot(keep);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) wcnt[w] = (uint32_t)__popcll(m);
  __syncthreads();
  int pre = 0, tot = 0;
  for (int k = 0; k < NT / 64; ++k) {
    const int s = (int)wcnt[k];
    if (k < w) pre += s;
    tot += s;
  }
  *total = tot;
  return pre + __popcll(m & ((1ull << lane) - 1ull));
}

__global__ void __launch_bounds__(NT) ov_draw_kernel(uint8_t* __restrict__ image, int W, int H, int tiles_x, const double* __restrict__ rec,
                                                     double t, uint32_t A, int L, Header* hd) {
  __shared__ Slot list[NT];
  __shared__ uint32_t wcnt[NT / 64];
  __shared__ uint8_t px[TY][TX * 3];
  __shared__ uint32_t red[NT / 64];
  const int n = hd->degenerate ? 0 : hd->nr + (int)hd->nc;
  if (n <= 0) return;
  const int tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * TX, ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * TY;
  const int col = threadIdx.x & (TX - 1), row0 = threadIdx.x >> 6;         // this thread: column col, rows row0 + 4 k
  const int gx = tx0 + col;
  const double tx_lo = (double)tx0, tx_hi = (double)(tx0 + TX - 1 < W - 1 ? tx0 + TX - 1 : W - 1);
  const double ty_lo = (double)ty0, ty_hi = (double)(ty0 + TY - 1 < H - 1 ? ty0 + TY - 1 : H - 1);
  uint32_t p[PER][3];
  bool hit[PER];
  #pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int gy = ty0 + row0 + 4 * k;
    hit[k] = false;
    p[k][0] = p[k][1] = p[k][2] = 0;
    if (gx < W && gy < H) {
      const uint8_t* q = image + ((long long)gy * W + gx) * 3;
      p[k][0] = q[0]; p[k][1] = q[1]; p[k][2] = q[2];
    }
  }
  bool touched = false;                            // uniform over the workgroup
  const double fx = (double)gx;
  // ---- the strokes of every chunk
  for (int base = 0; base < n; base += NT) {
    const int i = base + threadIdx.x;
    bool keep = false;
    const double* r = rec + (long long)REC * i;
    if (i < n) keep = ((int)r[1] & F_STROKE) && r[12] >= tx_lo && r[10] <= tx_hi && r[13] >= ty_lo && r[11] <= ty_hi;
    int cnt;
    const int slot = compact_slot(keep, wcnt, &cnt);
    if (keep) {
      Stroke& s = list[slot].s;
      s.X = r[2]; s.Y = r[3]; s.a = r[4]; s.b = r[5]; s.c = r[6]; s.s = r[7];
      s.col = (uint32_t)r[8]; s.kind = (uint32_t)r[0];
      s.x0 = (int)(r[10] > tx_lo ? r[10] : tx_lo); s.x1 = (int)(r[12] < tx_hi ? r[12] : tx_hi);
      s.y0 = (int)(r[11] > ty_lo ? r[11] : ty_lo); s.y1 = (int)(r[13] < ty_hi ? r[13] : ty_hi);
    }
    __syncthreads();
    touched |= cnt > 0;
    for (int e = 0; e < cnt; ++e) {
      const Stroke s = list[e].s;
      if (gx < s.x0 || gx > s.x1) continue;
      const double dx = fx - s.X;
      const uint32_t c0 = s.col & 255u, c1 = (s.col >> 8) & 255u, c2 = (s.col >> 16) & 255u;
      #pragma unroll
      for (int k = 0; k < PER; ++k) {
        const int gy = ty0 + row0 + 4 * k;
        if (gy < s.y0 || gy > s.y1) continue;
        const double dy = (double)gy - s.Y;
        bool on;
        if (s.kind == 1u) {
          const double xr = __builtin_fabs(dx * s.c - dy * s.s), yr = __builtin_fabs(dx * s.s + dy * s.c);
          on = xr <= s.a + t && yr <= s.b + t && !(xr < s.a - t && yr < s.b - t);
        } else {
          const double d2 = dx * dx + dy * dy;
          double lo = s.a - t;
          lo = lo > 0.0 ? lo : 0.0;
          on = lo * lo <= d2 && d2 <= (s.a + t) * (s.a + t);
        }
        if (on) {
          p[k][0] = blend1(p[k][0], c0, A); p[k][1] = blend1(p[k][1], c1, A); p[k][2] = blend1(p[k][2], c2, A);
          hit[k] = true;
        }
      }
    }
    __syncthreads();
  }
  // ---- then the labels
  if (L > 0) {
    for (int base = 0; base < n; base += NT) {
      const int i = base + threadIdx.x;
      bool keep = false;
      const double* r = rec + (long long)REC * i;
      if (i < n) keep = ((int)r[1] & F_LABEL) && r[16] >= tx_lo && r[14] <= tx_hi && r[17] >= ty_lo && r[15] <= ty_hi;
      int cnt;
      const int slot = compact_slot(keep, wcnt, &cnt);
      if (keep) {                                  // the box meets this tile: its corner is within a label of the picture
        Label& l = list[slot].l;
        l.lx = (int)r[14] + L; l.ly = (int)r[15] + L;
        l.col = (uint32_t)r[8];
        const uint32_t num = (uint32_t)r[9], nd = (uint32_t)r[18];
        uint32_t d = 0, q = num;
        for (uint32_t k = 0; k < nd; ++k) { d |= (q % 10u) << (4u * (nd - 1u - k)); q /= 10u; }
        l.digits = d | (nd << 16);
      }
      __syncthreads();
      touched |= cnt > 0;
      for (int e = 0; e < cnt; ++e) {
        const Label l = list[e].l;
        const int nd = (int)(l.digits >> 16);
        const int bw = (6 * nd - 1) * L, bh = 7 * L;
        const int ox = gx - l.lx;
        if (ox >= -L && ox < bw + L) {
          #pragma unroll
          for (int k = 0; k < PER; ++k) {
            const int oy = ty0 + row0 + 4 * k - l.ly;
            if (oy < -L || oy >= bh + L) continue;
            p[k][0] = blend1(p[k][0], 255u, DP_OVERLAY_LABEL_ALPHA);
            p[k][1] = blend1(p[k][1], 255u, DP_OVERLAY_LABEL_ALPHA);
            p[k][2] = blend1(p[k][2], 255u, DP_OVERLAY_LABEL_ALPHA);
            hit[k] = true;
            if (ox >= 0 && ox < bw && oy >= 0 && oy < bh) {
              const int q = ox / L, dg = q / 6, cc = q - 6 * dg;
              const uint32_t digit = (l.digits >> (4 * dg)) & 15u;
              if (cc < 5 && digit < 10u && ((FONT[digit][oy / L] >> (4 - cc)) & 1)) {
                p[k][0] = l.col & 255u; p[k][1] = (l.col >> 8) & 255u; p[k][2] = (l.col >> 16) & 255u;
              }
            }
          }
        }
      }
      __syncthreads();
    }
  }
  if (!touched) return;
  uint32_t painted = 0;
  #pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int r = row0 + 4 * k;
    px[r][3 * col] = (uint8_t)p[k][0]; px[r][3 * col + 1] = (uint8_t)p[k][1]; px[r][3 * col + 2] = (uint8_t)p[k][2];
    painted += hit[k] && gx < W && ty0 + r < H;
  }
  __syncthreads();
  // the tile's rows as dp_render.hip's resolve stores them: a dword where a whole dword lies inside the row's bytes,
  // single bytes at its ends
  const int wvalid = W - tx0 < TX ? W - tx0 : TX;
  const int nbytes = wvalid * 3;
  constexpr int WORDS = TX * 3 / 4 + 1;
  for (int idx = threadIdx.x; idx < TY * WORDS; idx += NT) {
    const int r = idx / WORDS, j = idx - r * WORDS;
    if (ty0 + r >= H) continue;
    uint8_t* p0 = image + ((long long)(ty0 + r) * W + tx0) * 3;
    const int lead = (int)((uintptr_t)p0 & 3);
    const int off = 4 * j - lead;
    if (off >= 0 && off + 4 <= nbytes) {
      const uint32_t wv = (uint32_t)px[r][off] | ((uint32_t)px[r][off + 1] << 8) | ((uint32_t)px[r][off + 2] << 16) |
                          ((uint32_t)px[r][off + 3] << 24);
      *(uint32_t*)(p0 + off) = wv;
    } else {
      for (int k = 0; k < 4; ++k)
        if (off + k >= 0 && off + k < nbytes) p0[off + k] = px[r][off + k];
    }
  }
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) painted += __shfl_xor(painted, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = painted;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t s = red[0] + red[1] + red[2] + red[3];
    if (s) atomicAdd(&hd->painted, s);
  }
}

__global__ void ov_stats_kernel(const Header* hd, double* __restrict__ stats) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int k = 0; k < 5; ++k) stats[k] = (double)hd->cnt[k];
  stats[5] = (double)hd->painted;
  stats[6] = (double)hd->error;
  stats[7] = 0.0;
}

inline bool finite_host(double v) { return v == v && v - v == 0.0; }
inline bool al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool caps_ok(int64_t max_rects, int64_t max_circles) {
  return max_rects >= 0 && max_circles >= 0 && max_rects + max_circles < ((int64_t)1 << 31);
}
}  // namespace

extern "C" int dp_overlay_debug_flags(int flags) {
  const int old = g_flags;
  g_flags = flags;
  return old;
}

extern "C" int64_t dp_overlay_workspace_size(int64_t max_rects, int64_t max_circles) {
  if (!caps_ok(max_rects, max_circles)) return 0;
  return HEADER_BYTES + al256(max_circles) + al256(4 * scan_blocks_for(max_circles));
}

extern "C" int dp_overlay_shapes(uint8_t* image, int32_t W, int32_t H, const double* camera_dev, const double* rects,
                                 const int32_t* n_rects_dev, int32_t max_rects, const double* shapes, const int32_t* n_clusters_dev,
                                 int32_t max_clusters, const uint8_t* palette, double stroke, int32_t alpha, int32_t label_scale,
                                 double* records_out, double* stats_out, void* workspace, int64_t workspace_bytes,
                                 dp_stream_t stream) {
  if (!image || !camera_dev || !palette || !records_out || !stats_out || !workspace) return DP_ERR_ARG;
  if (W < 1 || H < 1 || (int64_t)W * H >= ((int64_t)1 << 31)) return DP_ERR_ARG;
  if (!caps_ok(max_rects, max_clusters)) return DP_ERR_ARG;
  if ((max_rects > 0 && !rects) || (max_clusters > 0 && !shapes)) return DP_ERR_ARG;
  if (!al(camera_dev, 8) || !al(rects, 8) || !al(shapes, 8) || !al(records_out, 8) || !al(stats_out, 8) || !al(workspace, 8)) return DP_ERR_ARG;
  if (!al(n_rects_dev, 4) || !al(n_clusters_dev, 4)) return DP_ERR_ARG;
  if (!finite_host(stroke) || !(stroke > 0.0)) return DP_ERR_ARG;
  if (alpha < 0 || alpha > 255 || label_scale < 0 || label_scale > DP_OVERLAY_MAX_LABEL_SCALE) return DP_ERR_ARG;
  if (workspace_bytes < dp_overlay_workspace_size(max_rects, max_clusters)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  Header* hd = (Header*)ws;
  uint8_t* flag = (uint8_t*)(ws + HEADER_BYTES);
  uint32_t* bc = (uint32_t*)(ws + HEADER_BYTES + al256(max_clusters));
  Palette pal;
  for (int k = 0; k < 48; ++k) pal.c[k / 3][k % 3] = palette[k];
  const double t = stroke / 2.0;
  const int dbg = g_flags;
  if (!(dbg & F_SKIP_RECORDS))
    hipLaunchKernelGGL(ov_flags_kernel, dim3(grid_for(max_clusters, MAX_BLOCKS)), dim3(256), 0, s, shapes, n_clusters_dev, max_clusters,
                       n_rects_dev, max_rects, camera_dev, flag, hd);
  if (max_rects > 0 && !(dbg & F_SKIP_RECORDS))
    hipLaunchKernelGGL(ov_rect_records_kernel, dim3(grid_for(max_rects, MAX_BLOCKS)), dim3(256), 0, s, rects, camera_dev, pal, t,
                       label_scale, W, H, records_out, hd);
  if (max_clusters > 0 && !(dbg & F_SKIP_RECORDS)) {
    const int nb = (int)scan_blocks_for(max_clusters);
    hipLaunchKernelGGL(scan_count_kernel, dim3(nb), dim3(256), 0, s, (const uint8_t*)flag, n_clusters_dev, max_clusters, bc);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(256), 0, s, bc, nb, &hd->nc);
    hipLaunchKernelGGL(ov_circle_records_kernel, dim3(nb), dim3(256), 0, s, shapes, n_clusters_dev, max_clusters, (const uint8_t*)flag,
                       (const uint32_t*)bc, camera_dev, pal, t, label_scale, W, H, records_out, hd);
  }
  const int tiles_x = (W + TX - 1) / TX, tiles_y = (H + TY - 1) / TY;
  if (!(dbg & F_SKIP_DRAW))
    hipLaunchKernelGGL(ov_draw_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(NT), 0, s, image, W, H, tiles_x, (const double*)records_out, t,
                     (uint32_t)alpha, label_scale, hd);
  hipLaunchKernelGGL(ov_stats_kernel, dim3(1), dim3(64), 0, s, (const Header*)hd, stats_out);
  DP_CHECK_LAUNCH();
  return 0;
}
