// Floor-plan polygons (additive to ABI 20): the outline of every region of a dp_grid_regions call
// (cv2.findContours, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE), its simplification (contourArea, arcLength,
// approxPolyDP, Polygon.is_valid, the rectangle snap of approximate_contour) and the mean height of the
// raster's participants -- the rest of the reference's cleaned_pointcloud_to_floorplan.py behind the regions.
// The specification (rules O1-O5, S1-S7) is in dp_mi355x.h; this file is the method:
//   outlines:  start cells and cell counts (one pass over the labels) -> one wave per region walks its
//              border and counts -> one workgroup scans the counts into offsets -> the same walk writes.
//   polygons:  one workgroup per region: anchors, Douglas-Peucker level by level, validity over all edge
//              pairs, hull + calipers of dp_points.h -> one workgroup scans the counts -> the rows are written.
// Integer geometry is exact (64-bit); fp64 with no FMA contraction everywhere else.  No kernel waits on
// another workgroup; the walk is bounded by 8 * (cells of the region), the rounds by the vertex count.
#include "dp_common.h"
#include "dp_points.h"

#pragma clang fp contract(off)

namespace {

constexpr int GRID_CAP = 4096;
constexpr int MAX_DIM = DP_FLOOR_MAX_DIM;
constexpr int ICOLS = DP_OUTLINE_INT_COLUMNS;
constexpr int RCOLS = DP_OUTLINE_REAL_COLUMNS;
constexpr int PCOLS = DP_POLYGON_COLUMNS;
constexpr uint32_t NO_CELL = ~0u;
typedef long long i64;

// direction d of rule O2 (0 = E, counter-clockwise on the screen, z down) as a step: two bits per direction
__device__ __forceinline__ int dir_dx(int d) { return (int)((0x901Au >> (2 * d)) & 3u) - 1; }
__device__ __forceinline__ int dir_dz(int d) { return (int)((0xA901u >> (2 * d)) & 3u) - 1; }

__device__ __forceinline__ bool of_region(const int32_t* __restrict__ labels, int H, int W, int x, int z, int32_t l) {
  return x >= 0 && x < W && z >= 0 && z < H && labels[(long long)z * W + x] == l;
}

// ---- outlines: start cells ------------------------------------------------------------------------
__global__ void __launch_bounds__(256) start_init_kernel(uint32_t* __restrict__ start, uint32_t* __restrict__ cells, int max_regions) {
  for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < max_regions; r += (long long)gridDim.x * 256) {
    start[r] = NO_CELL;
    cells[r] = 0;
  }
}

// Rule O1.  A region's first cell has no member to its west, north-west, north or north-east; only such
// cells take the atomicMin.  The cell count (the walk's bound) takes one atomic per wave where the wave's
// cells share a label, which is the common case.
__global__ void __launch_bounds__(256) start_kernel(const int32_t* __restrict__ labels, const int32_t* dims, int max_cells,
                                                    const int32_t* n_regions, int max_regions, uint32_t* __restrict__ start,
                                                    uint32_t* __restrict__ cells) {
  int H, W;
  grid_dims(dims, max_cells, H, W);
  const long long total = (long long)H * W;
  const int rows = table_rows(n_regions, max_regions);
  for (long long b = (long long)blockIdx.x * 256; b < total; b += (long long)gridDim.x * 256) {
    const long long c = b + threadIdx.x;
    int32_t l = 0;
    if (c < total) l = labels[c];
    const bool in = l >= 1 && l <= rows;
    if (in) {
      const int z = (int)(c / W), x = (int)(c % W);
      if (!of_region(labels, H, W, x - 1, z, l) && !of_region(labels, H, W, x - 1, z - 1, l) &&
          !of_region(labels, H, W, x, z - 1, l) && !of_region(labels, H, W, x + 1, z - 1, l))
        atomicMin(&start[l - 1], (uint32_t)c);
    }
    const u64 m = __ballot(in);
    if (m) {
      const int leader = __ffsll((long long)m) - 1;
      const int32_t ll = __shfl(l, leader);
      const u64 same = __ballot(in && l == ll);
      if (same == m) {
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&cells[ll - 1], (uint32_t)__popcll(m));
      } else if (in) {
        atomicAdd(&cells[l - 1], 1u);
      }
    }
  }
}

// ---- outlines: the walk ---------------------------------------------------------------------------
// One wave per region; every lane carries the same state, lane k < 8 looks at the k-th direction of a
// search and a ballot picks the first hit.  WRITE = false: the columns; WRITE = true: the vertices of a
// region whose range in `offsets` holds them.
__device__ __forceinline__ float edge_len(int ax, int az, int bx, int bz) {
  const float dx = (float)(bx - ax), dz = (float)(bz - az);
  const float a = dx * dx, b = dz * dz;
  return __builtin_sqrtf(a + b);
}

template <bool WRITE>
__global__ void __launch_bounds__(64) walk_kernel(const int32_t* __restrict__ labels, const int32_t* dims, int max_cells,
                                                  const int32_t* n_regions, int max_regions, const uint32_t* __restrict__ start,
                                                  const uint32_t* __restrict__ cells, int max_vertices,
                                                  const int32_t* __restrict__ offsets, int32_t* __restrict__ vertices,
                                                  i64* __restrict__ cols, double* __restrict__ real) {
  int H, W;
  grid_dims(dims, max_cells, H, W);
  const long long total = (long long)H * W;
  const int rows = table_rows(n_regions, max_regions);
  const int lane = threadIdx.x & 63;
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const int32_t l = r + 1;
    const uint32_t s = start[r];
    i64 nv = 0, nb = 0, sum = 0;
    double per = 0.0;
    long long out = -1, room = 0;                                // where the vertices go (WRITE), -1: nowhere
    if (WRITE) {
      const long long beg = offsets[r], end = offsets[r + 1];
      if (beg >= 0 && end > beg && end <= max_vertices && end - beg == cols[(size_t)r * ICOLS]) { out = beg; room = end - beg; }
      if (out < 0) continue;
    }
    if (s != NO_CELL && (long long)s < total) {
      const int sx = (int)(s % (uint32_t)W), sz = (int)(s / (uint32_t)W);
      // i1: the first member clockwise from W
      int d0 = (4 - lane) & 7;
      const u64 hit0 = __ballot(lane < 8 && of_region(labels, H, W, sx + dir_dx(d0), sz + dir_dz(d0), l));
      if (!hit0) {
        nv = nb = 1;
        if (WRITE && lane == 0) { vertices[2 * out] = sx; vertices[2 * out + 1] = sz; }
      } else {
        const int s0 = (4 - (__ffsll((long long)hit0) - 1)) & 7;
        const int i1x = sx + dir_dx(s0), i1z = sz + dir_dz(s0);
        int x = sx, z = sz, din = s0;                            // i3 and the direction from i3 to i2
        int px = sx, pz = sz;                                    // the previous vertex
        const u64 bound = 8ull * cells[r];
        for (u64 step = 0; step < bound; ++step) {
          const int d = (din + 1 + lane) & 7;
          const u64 hit = __ballot(lane < 8 && of_region(labels, H, W, x + dir_dx(d), z + dir_dz(d), l));
          const int dout = hit ? (din + 1 + (__ffsll((long long)hit) - 1)) & 7 : din;
          ++nb;
          if (dout != (din ^ 4)) {                               // rule O3
            if (nv > 0) {
              sum += (i64)px * z - (i64)x * pz;
              per += (double)edge_len(px, pz, x, z);
            }
            if (WRITE && lane == 0 && nv < room) { vertices[2 * (out + nv)] = x; vertices[2 * (out + nv) + 1] = z; }
            ++nv;
            px = x; pz = z;
          }
          const int nx = x + dir_dx(dout), nz = z + dir_dz(dout);
          if (nx == sx && nz == sz && x == i1x && z == i1z) break;
          x = nx; z = nz; din = dout ^ 4;
        }
        sum += (i64)px * sz - (i64)sx * pz;
        per += (double)edge_len(px, pz, sx, sz);
      }
    }
    if (!WRITE && lane == 0) {
      i64* c = cols + (size_t)r * ICOLS;
      c[0] = nv; c[1] = nb; c[2] = sum; c[3] = s == NO_CELL ? -1 : (i64)s;
      real[(size_t)r * RCOLS] = (double)(sum < 0 ? -sum : sum) / 2.0;
      real[(size_t)r * RCOLS + 1] = per;
    }
  }
}

// ---- offsets: one workgroup -----------------------------------------------------------------------
// Rule O5 / S7: row r is written iff the counts of rows 0..r together fit the capacity; off[r + 1] is then
// their sum, otherwise off[r + 1] = off[r].  A row that fits has every earlier row fitting, so the offsets
// are the inclusive sums cut off at the last one that fits.
__device__ __forceinline__ void fit_offsets(const i64* __restrict__ cnt, int stride, int rows, i64 cap, int32_t* __restrict__ off,
                                            u64* total_out, u64* written_out) {
  __shared__ u64 wsum[4];
  __shared__ u64 last;
  if (threadIdx.x == 0) last = 0;
  __syncthreads();
  const int per = (rows + 255) / 256;
  const long long r0 = (long long)threadIdx.x * per;
  const long long r1 = r0 + per < rows ? r0 + per : rows;
  u64 s = 0, tot = 0;
  for (long long r = r0; r < r1; ++r) { const i64 c = cnt[(size_t)r * stride]; s += (u64)(c < 0 ? 0 : c); }
  u64 run = block_excl_scan(s, wsum, &tot);
  u64 mine = 0;
  for (long long r = r0; r < r1; ++r) {
    const i64 c = cnt[(size_t)r * stride];
    run += (u64)(c < 0 ? 0 : c);
    if (run <= (u64)cap) mine = run;
  }
  atomicMax(&last, mine);
  __syncthreads();
  const u64 lim = last;
  run -= s;
  if (threadIdx.x == 0) off[0] = 0;
  for (long long r = r0; r < r1; ++r) {
    const i64 c = cnt[(size_t)r * stride];
    run += (u64)(c < 0 ? 0 : c);
    off[r + 1] = (int32_t)(run <= (u64)cap ? run : lim);
  }
  *total_out = tot;
  *written_out = lim;
}

__global__ void __launch_bounds__(256) outline_offsets_kernel(const i64* __restrict__ cols, const int32_t* dims, int max_cells,
                                                              const int32_t* n_regions, int max_regions, int max_vertices,
                                                              int32_t* __restrict__ offsets, double* st) {
  const int rows = table_rows(n_regions, max_regions);
  u64 tot, wr;
  fit_offsets(cols, ICOLS, rows, max_vertices, offsets, &tot, &wr);
  if (threadIdx.x == 0) {
    int H, W;
    grid_dims(dims, max_cells, H, W);
    st[0] = (double)*n_regions;
    st[1] = (double)rows;
    st[2] = (double)tot;
    st[3] = (double)wr;
    st[4] = tot > wr ? 1.0 : 0.0;
    st[5] = *n_regions > max_regions ? 1.0 : 0.0;
    st[6] = (double)H;
    st[7] = (double)W;
  }
}

// ---- polygons: one workgroup per region -----------------------------------------------------------
enum { DROP_NONE = 0, DROP_SMALL, DROP_FEW, DROP_INVALID, DROP_OVERFLOW };

__device__ __forceinline__ i64 orient_i(i64 ax, i64 ay, i64 bx, i64 by, i64 cx, i64 cy) {
  return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}
// c on the closed segment a b, given that a, b, c are collinear
__device__ __forceinline__ bool on_segment(i64 ax, i64 ay, i64 bx, i64 by, i64 cx, i64 cy) {
  return (ax < bx ? ax : bx) <= cx && cx <= (ax > bx ? ax : bx) && (ay < by ? ay : by) <= cy && cy <= (ay > by ? ay : by);
}
__device__ __forceinline__ bool segments_meet(i64 ax, i64 ay, i64 bx, i64 by, i64 cx, i64 cy, i64 dx, i64 dy) {
  const i64 d1 = orient_i(cx, cy, dx, dy, ax, ay), d2 = orient_i(cx, cy, dx, dy, bx, by);
  const i64 d3 = orient_i(ax, ay, bx, by, cx, cy), d4 = orient_i(ax, ay, bx, by, dx, dy);
  if (((d1 > 0 && d2 < 0) || (d1 < 0 && d2 > 0)) && ((d3 > 0 && d4 < 0) || (d3 < 0 && d4 > 0))) return true;
  return (d1 == 0 && on_segment(cx, cy, dx, dy, ax, ay)) || (d2 == 0 && on_segment(cx, cy, dx, dy, bx, by)) ||
         (d3 == 0 && on_segment(ax, ay, bx, by, cx, cy)) || (d4 == 0 && on_segment(ax, ay, bx, by, dx, dy));
}

struct PolyWs {
  int32_t *cs, *ce, *ridx;     // per outline vertex (+ one per region): chain start, chain end, the ring's vertices
  u64* key;                    // per outline vertex (+ one per region): a chain's arg-max, at its start
  i64* pcnt;                   // per region: vertices of its polygon
  double* corner;              // per region: 8, the snapped rectangle
};

__global__ void __launch_bounds__(HULL_NT) simplify_kernel(const int32_t* __restrict__ offsets, const int32_t* __restrict__ vertices,
                                                           const i64* __restrict__ cols, const double* __restrict__ real,
                                                           const int32_t* n_regions, int max_regions, int max_vertices,
                                                           double resolution, double area_floor, double alpha, PolyWs w,
                                                           double* __restrict__ pcols) {
  __shared__ HullLds s;
  __shared__ u64 smax;
  __shared__ i64 ssum;
  __shared__ int cnt[2], wsum[4];
  __shared__ double rect[6];
  const int rows = table_rows(n_regions, max_regions), tid = threadIdx.x;
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const i64 nv64 = cols[(size_t)r * ICOLS];
    const long long beg = offsets[r], end = offsets[r + 1];
    const bool have = nv64 > 0 && beg >= 0 && end <= max_vertices && end - beg == nv64;
    const int nv = have ? (int)nv64 : 0;
    const double area = real[(size_t)r * RCOLS], eps = alpha * real[(size_t)r * RCOLS + 1];
    const double eps2 = eps * eps;
    const int32_t* V = vertices + 2 * (have ? beg : 0);
    const long long wb = (have ? beg : 0) + r;                   // nv + 1 workspace entries from here
    int reason = DROP_NONE, m = 0, snapped = 0;
    double parea = 0.0;
    if (area * (resolution * resolution) < area_floor) reason = DROP_SMALL;                // S1
    else if (!have) reason = DROP_OVERFLOW;
    int A = 0;
    if (!reason) {
      // ---- S3 anchors: three moves to the farthest vertex
      int cur = 0, far = 0;
      u64 best = 0;
      for (int it = 0; it < 3; ++it) {
        cur = (cur + far) % nv;
        if (tid == 0) smax = 0;
        __syncthreads();
        const i64 cx = V[2 * cur], cy = V[2 * cur + 1];
        u64 k = 0;
        for (int j = 1 + tid; j < nv; j += HULL_NT) {
          const int i = (cur + j) % nv;
          const i64 dx = V[2 * i] - cx, dy = V[2 * i + 1] - cy;
          const u64 kk = ((u64)(dx * dx + dy * dy) << 32) | (u64)(~(uint32_t)j);
          k = kk > k ? kk : k;
        }
        if (k) atomicMax(&smax, k);
        __syncthreads();
        best = smax;
        if (best >> 32) far = (int)(~(uint32_t)best);
        __syncthreads();
      }
      A = cur;
      const int jb = far;
      if ((double)(best >> 32) <= eps2 || jb <= 0 || jb >= nv) {
        m = 1;                                                   // the early exit: one vertex
      } else {
        // ---- S3 splitting, level by level over j = 0 .. nv (ring position A + j; nv is A again)
        for (int j = tid; j <= nv; j += HULL_NT) {
          const bool kept = j == 0 || j == jb || j == nv;
          w.cs[wb + j] = kept ? -1 : (j < jb ? 0 : jb);
          w.ce[wb + j] = j < jb ? jb : nv;
          w.ridx[wb + j] = kept;                                 // the keep flag until the ring is listed
        }
        __syncthreads();
        for (int round = 0; round < nv; ++round) {
          for (int j = tid; j <= nv; j += HULL_NT) w.key[wb + j] = 0;
          __syncthreads();
          for (int j = tid; j < nv; j += HULL_NT) {
            const int a = w.cs[wb + j];
            if (a < 0) continue;
            const int ia = (A + a) % nv, ib = (A + w.ce[wb + j]) % nv, i = (A + j) % nv;
            const i64 dx = V[2 * ib] - V[2 * ia], dy = V[2 * ib + 1] - V[2 * ia + 1];
            i64 c = (i64)(V[2 * i + 1] - V[2 * ia + 1]) * dx - (i64)(V[2 * i] - V[2 * ia]) * dy;
            c = c < 0 ? -c : c;
            atomicMax(&w.key[wb + a], ((u64)c << 32) | (u64)(~(uint32_t)j));
          }
          __syncthreads();
          int any = 0;
          for (int j = tid; j < nv; j += HULL_NT) {
            const int a = w.cs[wb + j];
            if (a < 0) continue;
            const int ia = (A + a) % nv, ib = (A + w.ce[wb + j]) % nv;
            const i64 dx = V[2 * ib] - V[2 * ia], dy = V[2 * ib + 1] - V[2 * ia + 1];
            const u64 k = w.key[wb + a];
            const double c = (double)(k >> 32);
            const int at = (int)(~(uint32_t)k);
            if (!(c * c > eps2 * (double)(dx * dx + dy * dy))) { w.cs[wb + j] = -1; continue; }
            if (j == at) { w.ridx[wb + j] = 1; w.cs[wb + j] = -1; any = 1; }
            else if (j < at) w.ce[wb + j] = at;
            else w.cs[wb + j] = at;
          }
          if (!__syncthreads_or(any)) break;
        }
        // ---- the ring in order from A: a scan of the keep flags (ce is free now: it takes the list)
        int run = 0;
        for (int t0 = 0; t0 < nv; t0 += HULL_NT) {
          const int j = t0 + tid;
          const int f = j < nv ? w.ridx[wb + j] : 0;
          int tot = 0;
          const int ex = run + block_excl_scan(f, wsum, &tot);
          if (f) w.ce[wb + ex] = (A + j) % nv;
          run += tot;
        }
        m = run;
        __syncthreads();
        for (int k = tid; k < m; k += HULL_NT) w.ridx[wb + k] = w.ce[wb + k];
        __syncthreads();
      }
      if (m < 3) reason = DROP_FEW;                              // S4
    }
    if (!reason) {
      // ---- S5: exact validity over all pairs
      const int32_t* R = w.ridx + wb;
      if (tid == 0) ssum = 0;
      __syncthreads();
      i64 part = 0;
      for (int k = tid; k < m; k += HULL_NT) {
        const int a = R[k], b = R[k + 1 < m ? k + 1 : 0];
        part += (i64)V[2 * a] * V[2 * b + 1] - (i64)V[2 * b] * V[2 * a + 1];
      }
      if (part) atomicAdd((u64*)&ssum, (u64)part);
      int bad = 0;
      const u64 pairs = (u64)m * (u64)m;
      for (u64 t = tid; t < pairs; t += HULL_NT) {
        const int i = (int)(t / (u64)m), j = (int)(t % (u64)m);
        if (i >= j) continue;
        const int a0 = R[i], a1 = R[i + 1 < m ? i + 1 : 0], b0 = R[j], b1 = R[j + 1 < m ? j + 1 : 0];
        const i64 ax = V[2 * a0], ay = V[2 * a0 + 1], bx = V[2 * a1], by = V[2 * a1 + 1];
        const i64 cx = V[2 * b0], cy = V[2 * b0 + 1], dx = V[2 * b1], dy = V[2 * b1 + 1];
        if (ax == cx && ay == cy) { bad = 1; continue; }
        if (j == i + 1 || (i == 0 && j == m - 1)) {              // adjacent edges p q, q r: a spike folds back
          i64 px, py, qx, qy, rx, ry;
          if (j == i + 1) { px = ax; py = ay; qx = cx; qy = cy; rx = dx; ry = dy; }
          else { px = cx; py = cy; qx = ax; qy = ay; rx = bx; ry = by; }
          const i64 cr = (qx - px) * (ry - qy) - (qy - py) * (rx - qx);
          const i64 dt = (qx - px) * (rx - qx) + (qy - py) * (ry - qy);
          if (cr == 0 && dt < 0) bad = 1;
        } else if (segments_meet(ax, ay, bx, by, cx, cy, dx, dy)) {
          bad = 1;
        }
      }
      bad = __syncthreads_or(bad);
      const i64 sum2 = ssum;
      __syncthreads();
      if (bad || sum2 == 0) reason = DROP_INVALID;
      parea = (double)(sum2 < 0 ? -sum2 : sum2) / 2.0;
    }
    if (!reason && m >= 4 && m <= 6) {
      // ---- S6: hull and calipers of dp_points.h on the ring
      const int32_t* R = w.ridx + wb;
      for (int i = tid; i < 8; i += HULL_NT) {
        s.st[i] = i < m ? (uint32_t)i : HULL_PAD;
        s.su[i] = i < m ? (double)V[2 * R[i]] : 0.0;
        s.sv[i] = i < m ? (double)V[2 * R[i] + 1] : 0.0;
      }
      __syncthreads();
      int kl;
      const int hn = hull_sort_chain(s, m, 8, cnt, &kl);
      double hu = 0.0, hv = 0.0;
      if (tid < hn) { const int i = hull_vertex(s, kl, tid); hu = s.su[i]; hv = s.sv[i]; }
      __syncthreads();
      if (tid < hn) { s.su[tid] = hu; s.sv[tid] = hv; }
      __syncthreads();
      hull_min_rect(s, hn, rect);
      __syncthreads();
      const double ra = rect[5];
      if (__builtin_fabs(ra - parea) / parea < 0.2) {
        snapped = 1;
        if (tid == 0) {                                          // cv2.boxPoints of (centre, (width, height), angle)
          const double ang = rect[4] / HULL_DEG;
          const double b = cos(ang) * 0.5, a = sin(ang) * 0.5;
          const double cx = rect[0], cy = rect[1], ww = rect[2], hh = rect[3];
          double* c = w.corner + 8 * (size_t)r;
          c[0] = cx - a * hh - b * ww; c[1] = cy + b * hh - a * ww;
          c[2] = cx + a * hh - b * ww; c[3] = cy - b * hh - a * ww;
          c[4] = 2.0 * cx - c[0];      c[5] = 2.0 * cy - c[1];
          c[6] = 2.0 * cx - c[2];      c[7] = 2.0 * cy - c[3];
        }
        parea = ra;
      }
      __syncthreads();
    }
    if (tid == 0) {
      const int n = reason ? 0 : (snapped ? 4 : m);
      w.pcnt[r] = n;
      double* c = pcols + (size_t)r * PCOLS;
      c[0] = (double)(r + 1);
      c[1] = (double)n;
      c[2] = (double)snapped;
      c[3] = reason ? 0.0 : parea;
      c[4] = reason ? 0.0 : parea * (resolution * resolution);
      c[5] = eps;
      c[6] = (double)reason;
      c[7] = (double)nv64;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(256) poly_offsets_kernel(PolyWs w, const int32_t* n_regions, int max_regions, int max_poly_vertices,
                                                           int32_t* __restrict__ poffsets, double* __restrict__ pcols, double* st) {
  __shared__ uint32_t ctr[5];
  const int rows = table_rows(n_regions, max_regions);
  if (threadIdx.x < 5) ctr[threadIdx.x] = 0;
  u64 tot, wr;
  fit_offsets(w.pcnt, 1, rows, max_poly_vertices, poffsets, &tot, &wr);
  __syncthreads();
  for (int r = threadIdx.x; r < rows; r += 256) {
    double* c = pcols + (size_t)r * PCOLS;
    if (w.pcnt[r] > 0 && poffsets[r + 1] - poffsets[r] != w.pcnt[r]) {       // S7: the polygon does not fit
      c[1] = 0.0; c[6] = (double)DROP_OVERFLOW;
    }
    atomicAdd(&ctr[(int)c[6]], 1u);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    st[0] = (double)rows;
    st[1] = (double)ctr[DROP_NONE];
    st[2] = (double)tot;
    st[3] = (double)wr;
    st[4] = (double)ctr[DROP_OVERFLOW];
    st[5] = (double)ctr[DROP_SMALL];
    st[6] = (double)ctr[DROP_FEW];
    st[7] = (double)ctr[DROP_INVALID];
  }
}

__global__ void __launch_bounds__(64) poly_write_kernel(const int32_t* __restrict__ offsets, const int32_t* __restrict__ vertices,
                                                        PolyWs w, const int32_t* n_regions, int max_regions, int max_vertices,
                                                        int max_poly_vertices, const int32_t* __restrict__ poffsets,
                                                        const double* __restrict__ pcols, double* __restrict__ pverts) {
  const int rows = table_rows(n_regions, max_regions);
  for (int r = blockIdx.x; r < rows; r += gridDim.x) {
    const long long to = poffsets[r], n = w.pcnt[r];
    if (n <= 0 || poffsets[r + 1] - to != n || to < 0 || to + n > max_poly_vertices) continue;
    if (pcols[(size_t)r * PCOLS + 2] != 0.0) {
      if (threadIdx.x < 8) pverts[2 * to + threadIdx.x] = w.corner[8 * (size_t)r + threadIdx.x];
      continue;
    }
    const long long beg = offsets[r];
    if (beg < 0 || beg + n > max_vertices) continue;
    for (int k = threadIdx.x; k < n; k += 64) {
      const int i = w.ridx[beg + r + k];
      pverts[2 * (to + k)] = (double)vertices[2 * (beg + i)];
      pverts[2 * (to + k) + 1] = (double)vertices[2 * (beg + i) + 1];
    }
  }
}

// ---- mean height of the raster's participants -----------------------------------------------------
__global__ void mean_init_kernel(double* out) { out[0] = 0.0; out[1] = 0.0; }

__global__ void __launch_bounds__(256) mean_sum_kernel(const double* __restrict__ pts, const int32_t* n_dev, int n_max, double thr,
                                                       double* out) {
  __shared__ double red[8];
  const int n = live_n(n_dev, n_max);
  double sy = 0.0, cnt = 0.0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    if (finite3(x, y, z) && !(y < thr)) { sy += y; cnt += 1.0; }
  }
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) { sy += __shfl_xor(sy, o); cnt += __shfl_xor(cnt, o); }
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = sy; red[4 + (threadIdx.x >> 6)] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double c = ((red[4] + red[5]) + red[6]) + red[7];
    if (c > 0.0) {
      atomicAdd(&out[0], ((red[0] + red[1]) + red[2]) + red[3]);
      atomicAdd(&out[1], c);
    }
  }
}

__global__ void mean_finish_kernel(double thr, double* out) { out[0] = out[1] > 0.0 ? out[0] / out[1] : thr; }

// ---- workspace ------------------------------------------------------------------------------------
struct Ws {
  uint32_t *start, *cells;
  PolyWs p;
};
int64_t ws_bytes_for(int64_t max_regions, int64_t max_vertices) {
  const int64_t k = max_regions < 0 ? 0 : max_regions, v = (max_vertices < 0 ? 0 : max_vertices) + k + 1;
  return 2 * al256(4 * k) + 3 * al256(4 * v) + al256(8 * v) + al256(8 * k) + al256(64 * k) + 256;
}
bool ws_carve(void* ws, int64_t bytes, int64_t max_regions, int64_t max_vertices, Ws* o) {
  if (!ws || bytes < ws_bytes_for(max_regions, max_vertices) || ((uintptr_t)ws & 7)) return false;
  const int64_t k = max_regions, v = max_vertices + k + 1;
  char* p = (char*)ws;
  o->start = (uint32_t*)p;    p += al256(4 * k);
  o->cells = (uint32_t*)p;    p += al256(4 * k);
  o->p.cs = (int32_t*)p;      p += al256(4 * v);
  o->p.ce = (int32_t*)p;      p += al256(4 * v);
  o->p.ridx = (int32_t*)p;    p += al256(4 * v);
  o->p.key = (u64*)p;         p += al256(8 * v);
  o->p.pcnt = (i64*)p;        p += al256(8 * k);
  o->p.corner = (double*)p;
  return true;
}
bool pos_finite(double v) { return v > 0.0 && v < __builtin_inf(); }
int region_grid(int max_regions) { return max_regions < 1 ? 1 : (max_regions > GRID_CAP ? GRID_CAP : max_regions); }

}  // namespace

extern "C" int64_t dp_outline_workspace_size(int64_t max_cells, int64_t max_regions, int64_t max_vertices) {
  (void)max_cells;                                               // nothing is kept per cell
  return ws_bytes_for(max_regions, max_vertices);
}

extern "C" int dp_region_outlines(const int32_t* labels, const int32_t* dims, int32_t max_cells, const int32_t* n_regions_dev,
                                  int32_t max_regions, int32_t max_vertices, int32_t* offsets_out, int32_t* vertices_out,
                                  int64_t* columns_out, double* measures_out, double* stats_out, void* workspace,
                                  int64_t workspace_bytes, dp_stream_t stream) {
  if (!dims || !n_regions_dev || !offsets_out || !stats_out || (max_cells > 0 && !labels) || (max_vertices > 0 && !vertices_out) ||
      (max_regions > 0 && (!columns_out || !measures_out)))
    return DP_ERR_ARG;
  if (max_cells < 0 || max_regions < 0 || max_vertices < 0) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, max_regions, max_vertices, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int gr = region_grid(max_regions);
  i64* cols = (i64*)columns_out;
  hipLaunchKernelGGL(start_init_kernel, dim3(grid_for(max_regions, GRID_CAP)), dim3(256), 0, s, w.start, w.cells, max_regions);
  hipLaunchKernelGGL(start_kernel, dim3(grid_for(max_cells, GRID_CAP)), dim3(256), 0, s, labels, dims, max_cells, n_regions_dev,
                     max_regions, w.start, w.cells);
  hipLaunchKernelGGL(walk_kernel<false>, dim3(gr), dim3(64), 0, s, labels, dims, max_cells, n_regions_dev, max_regions, w.start,
                     w.cells, max_vertices, offsets_out, vertices_out, cols, measures_out);
  hipLaunchKernelGGL(outline_offsets_kernel, dim3(1), dim3(256), 0, s, cols, dims, max_cells, n_regions_dev, max_regions,
                     max_vertices, offsets_out, stats_out);
  hipLaunchKernelGGL(walk_kernel<true>, dim3(gr), dim3(64), 0, s, labels, dims, max_cells, n_regions_dev, max_regions, w.start,
                     w.cells, max_vertices, offsets_out, vertices_out, cols, measures_out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_simplify_outlines_with(const int32_t* offsets, const int32_t* vertices, const int64_t* columns,
                                         const double* measures, const int32_t* n_regions_dev, int32_t max_regions,
                                         int32_t max_vertices, double resolution, double area_floor, double alpha,
                                         int32_t max_polygon_vertices, int32_t* polygon_offsets_out, double* polygon_vertices_out,
                                         double* polygons_out, double* stats_out, void* workspace, int64_t workspace_bytes,
                                         dp_stream_t stream) {
  if (!offsets || !n_regions_dev || !polygon_offsets_out || !stats_out || (max_vertices > 0 && !vertices) ||
      (max_polygon_vertices > 0 && !polygon_vertices_out) || (max_regions > 0 && (!columns || !measures || !polygons_out)))
    return DP_ERR_ARG;
  if (max_regions < 0 || max_vertices < 0 || max_polygon_vertices < 0 || !pos_finite(resolution) || !(area_floor >= 0.0) ||
      !(area_floor < __builtin_inf()) || !(alpha >= 0.0) || !(alpha < __builtin_inf()))
    return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, max_regions, max_vertices, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int gr = region_grid(max_regions);
  hipLaunchKernelGGL(simplify_kernel, dim3(gr), dim3(HULL_NT), 0, s, offsets, vertices, (const i64*)columns, measures, n_regions_dev,
                     max_regions, max_vertices, resolution, area_floor, alpha, w.p, polygons_out);
  hipLaunchKernelGGL(poly_offsets_kernel, dim3(1), dim3(256), 0, s, w.p, n_regions_dev, max_regions, max_polygon_vertices,
                     polygon_offsets_out, polygons_out, stats_out);
  hipLaunchKernelGGL(poly_write_kernel, dim3(gr), dim3(64), 0, s, offsets, vertices, w.p, n_regions_dev, max_regions, max_vertices,
                     max_polygon_vertices, polygon_offsets_out, polygons_out, polygon_vertices_out);
  DP_CHECK_LAUNCH();
  return 0;
}

// the height-threshold mode's halvings (S1: min_area / 4, an exact division, so a bad min_area stays one; S2: alpha 0.01 / 2)
extern "C" int dp_simplify_outlines(const int32_t* offsets, const int32_t* vertices, const int64_t* columns, const double* measures,
                                    const int32_t* n_regions_dev, int32_t max_regions, int32_t max_vertices, double resolution,
                                    double min_area, int32_t max_polygon_vertices, int32_t* polygon_offsets_out,
                                    double* polygon_vertices_out, double* polygons_out, double* stats_out, void* workspace,
                                    int64_t workspace_bytes, dp_stream_t stream) {
  return dp_simplify_outlines_with(offsets, vertices, columns, measures, n_regions_dev, max_regions, max_vertices, resolution,
                                   min_area / 4.0, 0.005, max_polygon_vertices, polygon_offsets_out, polygon_vertices_out,
                                   polygons_out, stats_out, workspace, workspace_bytes, stream);
}

extern "C" int dp_floor_mean_height(const double* points, const int32_t* n_dev, int32_t n_max, double height_threshold,
                                    double* mean_out, dp_stream_t stream) {
  if (!mean_out || (n_max > 0 && !points)) return DP_ERR_ARG;
  if (n_max < 0 || __builtin_fabs(height_threshold) == __builtin_inf()) return DP_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(mean_init_kernel, dim3(1), dim3(1), 0, s, mean_out);
  hipLaunchKernelGGL(mean_sum_kernel, dim3(grid_for(n_max, 1024)), dim3(256), 0, s, points, n_dev, n_max, height_threshold, mean_out);
  hipLaunchKernelGGL(mean_finish_kernel, dim3(1), dim3(1), 0, s, height_threshold, mean_out);
  DP_CHECK_LAUNCH();
  return 0;
}
