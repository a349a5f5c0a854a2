// L-shape split (additive to ABI 20): the rectangle list of the shapes stage (dp_shape_rectangles) and the
// reference's detect_and_split_l_shapes on it (dp_lshape_split), in the top-down frame u = -x, v = z.
// fp64 as numpy computes it; no FMA contraction anywhere in this file, so each product, sum and
// difference is rounded on its own.  The specification (rules 1-10) is in the header; this file is the
// method:
//   prep (one workgroup: candidates, grid sizes, two scans) -> raster (points x candidates) ->
//   dilation and the empty cells -> union-find over the empty cells, their sizes, the empty mask ->
//   union-find over the occupied cells, their sizes -> flags of the components to fit, their scan ->
//   one workgroup per component: row extremes, hull, calipers (dp_points.h) -> decision, output scan, rows.
// Every rectangle's grid is a range of one cell array (a byte per cell), cell = offset + gy * gw + gx, so
// every per-cell kernel runs over all grids at once and finds its rectangle by a search in the offsets.
// No kernel waits on another workgroup; a thread's loops run over one rectangle's share of the list, one
// grid row, or one rectangle's components, never over the points or a grid.
#include "dp_common.h"
#include "dp_points.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = HULL_NT;
constexpr int GRID_CAP = 4096;
constexpr int MAX_SIDE = DP_LSHAPE_MAX_SIDE;
constexpr int TILE = 64;                        // candidates of one LDS tile of the raster
constexpr double PI = 3.141592653589793;
constexpr double CELL = 0.2;                    // the reference's grid_size
constexpr int INT_BIG = 0x7fffffff;

static_assert(2 * MAX_SIDE <= HULL_MAX, "a component's row extremes must fit one hull chunk");

// the statuses of the header
enum { ST_SPLIT = 0, ST_SMALL = 1, ST_FEW = 2, ST_THIN = 3, ST_FULL = 4, ST_RATIO = 5, ST_ONE = 6, ST_PARTS = 7,
       ST_AREA = 8, ST_CAP = 9 };

struct LHdr {
  int32_t rects, cands, cells;
  uint32_t comps;
};

// what the raster and the later stages need of one rectangle
struct Cand {
  double cu, cv, c, s, hw, hh, rad2, angle;
  int32_t gw, gh, pre, grid;                    // pre: the status rules 1 and 4 give (0: none yet); grid: cells allocated
};

struct Ws {
  LHdr* h;
  Cand* cand;
  int32_t *celloff, *list, *ocnt, *stat;
  uint32_t *inside, *emptyc, *nocc;
  uint8_t *b, *e, *occ, *flag;
  uint32_t *par1, *par2, *sz1, *sz2, *bc, *croot;
  double* sub;
};
__host__ __device__ inline int64_t comps_for(int64_t cells) { return cells / 6 + 1; }
int64_t ws_bytes_for(int64_t max_rects, int64_t max_cells) {
  const int64_t r = max_rects < 0 ? 0 : max_rects, c = max_cells < 0 ? 0 : max_cells;
  return al256(sizeof(LHdr)) + al256((int64_t)sizeof(Cand) * r) + 4 * al256(4 * (r + 1)) + 3 * al256(4 * r) + 4 * al256(c) +
         4 * al256(4 * c) + al256(4 * (scan_blocks_for(c) + 1)) + al256(4 * comps_for(c)) + al256(48 * comps_for(c)) + 256;
}
bool ws_carve(void* ws, int64_t bytes, int64_t r, int64_t c, Ws* o) {
  if (!ws || bytes < ws_bytes_for(r, c) || ((uintptr_t)ws & 7)) return false;
  char* p = (char*)ws;
  o->h = (LHdr*)p;             p += al256(sizeof(LHdr));
  o->cand = (Cand*)p;          p += al256((int64_t)sizeof(Cand) * r);
  o->celloff = (int32_t*)p;    p += al256(4 * (r + 1));
  o->list = (int32_t*)p;       p += al256(4 * (r + 1));
  o->ocnt = (int32_t*)p;       p += al256(4 * (r + 1));
  o->stat = (int32_t*)p;       p += al256(4 * (r + 1));
  o->inside = (uint32_t*)p;    p += al256(4 * r);
  o->emptyc = (uint32_t*)p;    p += al256(4 * r);
  o->nocc = (uint32_t*)p;      p += al256(4 * r);
  o->b = (uint8_t*)p;          p += al256(c);
  o->e = (uint8_t*)p;          p += al256(c);
  o->occ = (uint8_t*)p;        p += al256(c);
  o->flag = (uint8_t*)p;       p += al256(c);
  o->par1 = (uint32_t*)p;      p += al256(4 * c);
  o->par2 = (uint32_t*)p;      p += al256(4 * c);
  o->sz1 = (uint32_t*)p;       p += al256(4 * c);
  o->sz2 = (uint32_t*)p;       p += al256(4 * c);
  o->bc = (uint32_t*)p;        p += al256(4 * (scan_blocks_for(c) + 1));
  o->croot = (uint32_t*)p;     p += al256(4 * comps_for(c));
  o->sub = (double*)p;
  return true;
}

// int(q) + 1 of rule 4 for q = side / 0.2, saturated (a NaN side saturates too)
__device__ __forceinline__ int grid_side(double side) {
  const double q = side / CELL;
  return q > -2.0e9 && q < 2.0e9 ? (int)q + 1 : INT_BIG;
}

// ---- dp_shape_rectangles: one workgroup -------------------------------------------------------------
__device__ __forceinline__ int rows_of(const double* __restrict__ row) {
  if (row[0] != 1.0) return 0;
  return row[4] * row[5] > 100.0 && row[1] > 1000.0 ? 2 : 1;
}
__global__ void __launch_bounds__(NT) rectangles_kernel(const double* __restrict__ shapes, const int32_t* ncl, int max_clusters,
                                                        double* __restrict__ rects, int32_t* n_rects) {
  __shared__ int wsum[4];
  const int k = table_rows(ncl, max_clusters);
  const int per = (k + NT - 1) / NT;
  const long long c0 = (long long)threadIdx.x * per;
  const long long c1 = c0 + per < k ? c0 + per : k;
  int s = 0, tot = 0;
  for (long long c = c0; c < c1; ++c) s += rows_of(shapes + 16 * c);
  int run = block_excl_scan(s, wsum, &tot);
  for (long long c = c0; c < c1; ++c) {
    const double* row = shapes + 16 * c;
    const int m = rows_of(row);
    if (m == 0) continue;
    const double cu = row[2], cv = row[3], w = row[4], h = row[5], ang = row[6];
    double* o = rects + 8 * (size_t)run;
    if (m == 1) {
      o[0] = cu; o[1] = cv; o[2] = w; o[3] = h; o[4] = ang; o[5] = (double)c; o[6] = 0.0; o[7] = 0.0;
    } else {
      const double a = ang * PI / 180.0;
      const double ca = cos(a), sa = sin(a);
      if (w > h) {
        const double d = w / 4.0;
        o[0] = cu - d * ca; o[1] = cv - d * sa; o[2] = w / 2.0; o[3] = h;
        o[8] = cu + d * ca; o[9] = cv + d * sa; o[10] = w / 2.0; o[11] = h;
      } else {
        const double d = h / 4.0;
        o[0] = cu - d * sa; o[1] = cv + d * ca; o[2] = w; o[3] = h / 2.0;
        o[8] = cu + d * sa; o[9] = cv - d * ca; o[10] = w; o[11] = h / 2.0;
      }
      o[4] = o[12] = ang;
      o[5] = o[13] = (double)c;
      o[6] = o[14] = 1.0;
      o[7] = o[15] = 0.0;
    }
    run += m;
  }
  if (threadIdx.x == 0) *n_rects = tot;
}

// ---- prep: one workgroup ------------------------------------------------------------------------
__device__ __forceinline__ void sides_of(const double* __restrict__ row, int* pre, int* gw, int* gh, int* cells) {
  const double w = row[2], h = row[3];
  *pre = 0; *gw = 0; *gh = 0; *cells = 0;
  if (w * h < 10.0) { *pre = ST_SMALL; return; }
  *gw = grid_side(w);
  *gh = grid_side(h);
  if (*gw <= 2 || *gh <= 2) *pre = ST_THIN;
  else if (*gw > MAX_SIDE || *gh > MAX_SIDE) *pre = ST_CAP;
  else *cells = *gw * *gh;
}
__global__ void __launch_bounds__(NT) prep_kernel(const double* __restrict__ rects, const int32_t* n_rects, int max_rects,
                                                  int max_cells, Ws w) {
  __shared__ long long wsum[4];
  __shared__ int isum[4];
  __shared__ long long fit;
  const int R = table_rows(n_rects, max_rects);
  const int per = (R + NT - 1) / NT;
  const long long r0 = (long long)threadIdx.x * per;
  const long long r1 = r0 + per < R ? r0 + per : R;
  long long cs = 0, ctot = 0;
  int ls = 0, ltot = 0;
  for (long long r = r0; r < r1; ++r) {
    int pre, gw, gh, cells;
    sides_of(rects + 8 * r, &pre, &gw, &gh, &cells);
    cs += cells;
    ls += pre != ST_SMALL;
  }
  long long crun = block_excl_scan(cs, wsum, &ctot);
  int lrun = block_excl_scan(ls, isum, &ltot);
  if (threadIdx.x == 0) fit = ctot;
  __syncthreads();
  // a grid is allocated while the grids up to and including it fit in max_cells; `fit` = the cells allocated
  {
    long long run = crun;
    for (long long r = r0; r < r1; ++r) {
      int pre, gw, gh, cells;
      sides_of(rects + 8 * r, &pre, &gw, &gh, &cells);
      if (cells > 0 && run + cells > max_cells) { atomicMin((u64*)&fit, (u64)run); break; }
      run += cells;
    }
  }
  __syncthreads();
  const long long total = fit;
  for (long long r = r0; r < r1; ++r) {
    const double* row = rects + 8 * r;
    int pre, gw, gh, cells;
    sides_of(row, &pre, &gw, &gh, &cells);
    const bool over = cells > 0 && crun + cells > total;
    Cand c;
    c.cu = row[0]; c.cv = row[1];
    c.hw = row[2] / 2.0; c.hh = row[3] / 2.0;
    c.angle = row[4];
    const double a = -row[4] * PI / 180.0;
    c.c = cos(a); c.s = sin(a);
    c.rad2 = (c.hw * c.hw + c.hh * c.hh) * 1.000001;             // the raster's reject only: generous
    c.gw = gw; c.gh = gh;
    c.pre = over ? ST_CAP : pre;
    c.grid = over ? 0 : cells;
    w.cand[r] = c;
    w.celloff[r] = (int32_t)(crun < total ? crun : total);
    w.inside[r] = 0; w.emptyc[r] = 0; w.nocc[r] = 0;
    if (pre != ST_SMALL) w.list[lrun++] = (int32_t)r;
    crun += cells;
  }
  if (threadIdx.x == 0) {
    w.celloff[R] = (int32_t)total;
    w.h->rects = R; w.h->cands = ltot; w.h->cells = (int32_t)total; w.h->comps = 0;
  }
}

// ---- raster: points x candidates ------------------------------------------------------------------
__global__ void __launch_bounds__(NT) raster_kernel(const double* __restrict__ pts, const int32_t* __restrict__ labels,
                                                    const int32_t* n_dev, int n_max, Ws w) {
  __shared__ Cand tile[TILE];
  __shared__ int32_t tile_r[TILE], tile_off[TILE];
  const int n = live_n(n_dev, n_max), nc = w.h->cands, cells = w.h->cells;
  for (long long base = (long long)blockIdx.x * NT; base < n; base += (long long)gridDim.x * NT) {
    const long long i = base + threadIdx.x;
    const bool take = i < n && labels[i] >= -1;
    const double u = take ? -pts[3 * (size_t)i] : 0.0, v = take ? pts[3 * (size_t)i + 2] : 0.0;
    for (int cb = 0; cb < nc; cb += TILE) {
      __syncthreads();
      if (threadIdx.x < TILE && cb + threadIdx.x < nc) {
        const int r = w.list[cb + threadIdx.x];
        tile[threadIdx.x] = w.cand[r];
        tile_r[threadIdx.x] = r;
        tile_off[threadIdx.x] = w.celloff[r];
      }
      __syncthreads();
      const int m = nc - cb < TILE ? nc - cb : TILE;
      for (int j = 0; j < m; ++j) {
        const double du = u - tile[j].cu, dv = v - tile[j].cv;
        bool in = false;
        if (take && du * du + dv * dv <= tile[j].rad2) {
          const double c = tile[j].c, s = tile[j].s, hw = tile[j].hw, hh = tile[j].hh;
          const double xr = du * c - dv * s, yr = du * s + dv * c;
          in = -hw < xr && xr < hw && -hh < yr && yr < hh;
          if (in && tile[j].grid > 0) {
            const int gw = tile[j].gw, gh = tile[j].gh;
            const int gx = (int)((xr + hw) / CELL), gy = (int)((yr + hh) / CELL);
            if (gx >= 0 && gx < gw && gy >= 0 && gy < gh) {
              const long long cell = (long long)tile_off[j] + (long long)gy * gw + gx;
              if (cell < cells) w.b[cell] = 1;                   // every writer stores the same byte
            }
          }
        }
        wave_count(&w.inside[tile_r[j]], in);
      }
    }
  }
}

// ---- the grids: a thread per cell over all grids at once --------------------------------------------
struct CellAt { int r, gw, x, y; };
__device__ __forceinline__ CellAt cell_at(const Ws& w, int R, long long i) {
  CellAt a;
  int r = upper_bound(w.celloff, R + 1, (int)i) - 1;
  a.r = r < 0 ? 0 : (r < R ? r : R - 1);
  a.gw = w.cand[a.r].gw;
  a.gw = a.gw < 1 ? 1 : a.gw;
  const int loc = (int)i - w.celloff[a.r];
  a.y = loc / a.gw;
  a.x = loc - a.y * a.gw;
  return a;
}
#define FOR_CELLS(i) \
  const int R = w.h->rects; \
  const long long cells = w.h->cells; \
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < cells; i += (long long)gridDim.x * 256)

// rule 6 and the empty cells; every per-cell array reset
__global__ void __launch_bounds__(256) dilate_kernel(Ws w) {
  FOR_CELLS(i) {
    const CellAt a = cell_at(w, R, i);
    uint8_t d = w.b[i];
    if (a.x > 0) d |= w.b[i - 1];
    if (a.y > 0) d |= w.b[i - a.gw];
    if (a.x > 0 && a.y > 0) d |= w.b[i - a.gw - 1];
    w.e[i] = !d;
    w.par1[i] = w.par2[i] = (uint32_t)i;
    w.sz1[i] = w.sz2[i] = 0;
  }
}
// 4-connected components of a byte mask: each set cell joined to its west and north neighbours
__global__ void __launch_bounds__(256) link_kernel(Ws w, const uint8_t* __restrict__ mask, uint32_t* __restrict__ par) {
  FOR_CELLS(i) {
    if (!mask[i]) continue;
    const CellAt a = cell_at(w, R, i);
    if (a.x > 0 && mask[i - 1]) uf_unite(par, (uint32_t)i, (uint32_t)(i - 1));
    if (a.y > 0 && mask[i - a.gw]) uf_unite(par, (uint32_t)i, (uint32_t)(i - a.gw));
  }
}
// a component's size at its root; with nroots, the components per rectangle
__global__ void __launch_bounds__(256) size_kernel(Ws w, const uint8_t* __restrict__ mask, uint32_t* __restrict__ par,
                                                   uint32_t* __restrict__ sz, uint32_t* __restrict__ nroots) {
  FOR_CELLS(i) {
    if (!mask[i]) continue;
    const uint32_t root = uf_find(par, (uint32_t)i);
    atomicAdd(&sz[root], 1u);
    if (nroots && root == (uint32_t)i) atomicAdd(&nroots[cell_at(w, R, i).r], 1u);
  }
}
// rule 7's empty_mask and rule 8's occupied cells
__global__ void __launch_bounds__(256) mask_kernel(Ws w) {
  FOR_CELLS(i) {
    const bool em = w.e[i] && w.sz1[uf_find(w.par1, (uint32_t)i)] >= 6u;
    w.occ[i] = !em;
    if (em) atomicAdd(&w.emptyc[cell_at(w, R, i).r], 1u);
  }
}

// rules 1-8 for rectangle r, once the grids are done: the status that keeps it, or 0
__device__ __forceinline__ int status_before_parts(const Ws& w, int r) {
  const Cand& c = w.cand[r];
  if (c.pre == ST_SMALL) return ST_SMALL;
  if (w.inside[r] < 50u) return ST_FEW;
  if (c.pre) return c.pre;
  const uint32_t em = w.emptyc[r];
  if (em == 0) return ST_FULL;
  const double ratio = (double)em / (double)(c.gw * c.gh);
  if (ratio < 0.2 || ratio > 0.6) return ST_RATIO;
  if (w.nocc[r] < 2u) return ST_ONE;
  return 0;
}
// the components rule 9 fits: the roots of >= 6 cells in a rectangle still open
__global__ void __launch_bounds__(256) flag_kernel(Ws w) {
  FOR_CELLS(i) {
    uint8_t f = 0;
    if (w.occ[i] && ld(&w.par2[i]) == (uint32_t)i && w.sz2[i] >= 6u) f = status_before_parts(w, cell_at(w, R, i).r) == 0;
    w.flag[i] = f;
  }
}
// third step of the flags' scan: component k's root, in row-major order of the first cells
__global__ void __launch_bounds__(256) roots_kernel(Ws w, int max_cells) {
  __shared__ uint32_t wsum[4];
  const int n = live_n(&w.h->cells, max_cells);
  const long long tile = (long long)blockIdx.x * SCAN_TILE;
  uint32_t run = w.bc[blockIdx.x];
  for (int r = 0; r < SCAN_ITEMS && tile + r * 256 < n; ++r) {
    const long long t = tile + r * 256 + threadIdx.x;
    const uint32_t f = t < n ? w.flag[t] : 0u;
    uint32_t tot = 0;
    const uint32_t excl = run + block_excl_scan(f, wsum, &tot);
    if (f && excl < (uint32_t)comps_for(max_cells)) w.croot[excl] = (uint32_t)t;
    run += tot;
  }
}

// ---- rule 9: one component per workgroup ------------------------------------------------------------
// A wave takes every fourth grid row: 64 cells per step, the ballot of "in this component" gives the
// row's leftmost and rightmost cell.  Their hull is the component's.  Slot 2y and 2y + 1 of the chunk.
__global__ void __launch_bounds__(NT) part_kernel(Ws w, int max_cells) {
  __shared__ HullLds s;
  __shared__ double res[6];
  __shared__ int cnt[2], members;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int R = w.h->rects;
  const long long cells = w.h->cells;
  uint32_t nk = w.h->comps;
  const uint32_t cap = (uint32_t)comps_for(max_cells);
  nk = nk < cap ? nk : cap;
  for (uint32_t k = blockIdx.x; k < nk; k += gridDim.x) {
    const uint32_t root = w.croot[k];
    if (root >= (uint32_t)cells) continue;                       // cannot happen
    const CellAt a = cell_at(w, R, root);
    const Cand c = w.cand[a.r];
    const int gw = c.gw, gh = c.gh;
    const long long g0 = w.celloff[a.r];
    if (gw < 1 || gh < 1 || gh > MAX_SIDE || g0 + (long long)gw * gh > cells) continue;   // cannot happen
    int P = 2;
    while (P < 2 * gh) P <<= 1;
    __syncthreads();                                             // the previous component's reads are done
    for (int i = tid; i < P; i += NT) { s.st[i] = HULL_PAD; s.su[i] = 0.0; s.sv[i] = 0.0; }
    if (tid == 0) members = 0;
    __syncthreads();
    for (int y = wave; y < gh; y += NT / 64) {
      int xl = -1, xr = -1;
      for (int x0 = 0; x0 < gw; x0 += 64) {
        const int x = x0 + lane;
        bool in = false;
        if (x < gw) {
          const long long cell = g0 + (long long)y * gw + x;
          in = w.occ[cell] && uf_find(w.par2, (uint32_t)cell) == root;
        }
        const u64 bal = __ballot(in);
        if (bal) {
          if (xl < 0) xl = x0 + __ffsll((long long)bal) - 1;
          xr = x0 + 63 - __clzll((long long)bal);
        }
      }
      if (lane == 0 && xl >= 0) {
        const double v = (double)y * CELL - c.hh;
        s.st[2 * y] = (uint32_t)(2 * y); s.su[2 * y] = (double)xl * CELL - c.hw; s.sv[2 * y] = v;
        if (xr != xl) { s.st[2 * y + 1] = (uint32_t)(2 * y + 1); s.su[2 * y + 1] = (double)xr * CELL - c.hw; s.sv[2 * y + 1] = v; }
        atomicAdd(&members, xr != xl ? 2 : 1);
      }
    }
    __syncthreads();
    const int m = members;
    int kl;
    const int hn = hull_sort_chain(s, m, P, cnt, &kl);
    double hu[HULL_MAX / NT], hv[HULL_MAX / NT];
    #pragma unroll
    for (int q = 0; q < HULL_MAX / NT; ++q) {
      const int e = tid + q * NT;
      hu[q] = hv[q] = 0.0;
      if (e < hn) {
        const int i = hull_vertex(s, kl, e);
        hu[q] = s.su[i]; hv[q] = s.sv[i];
      }
    }
    __syncthreads();
    #pragma unroll
    for (int q = 0; q < HULL_MAX / NT; ++q) {
      const int e = tid + q * NT;
      if (e < hn) { s.su[e] = hu[q]; s.sv[e] = hv[q]; }
    }
    __syncthreads();
    hull_min_rect(s, hn, res);
    __syncthreads();
    if (tid == 0) {
      const double sx = res[0], sy = res[1], sw = res[2], sh = res[3];
      double* o = w.sub + 6 * (size_t)k;
      o[0] = (sx * c.c - sy * c.s) + c.cu;                       // the reference's second rotation by -angle, as written
      o[1] = (sx * c.s + sy * c.c) + c.cv;
      o[2] = sw; o[3] = sh;
      o[4] = __builtin_fmod(res[4] + c.angle, 180.0);
      o[5] = sw * sh > 1.0 ? 1.0 : 0.0;
    }
  }
}

// ---- rule 10, the output offsets and the rows: one workgroup -----------------------------------------
__device__ __forceinline__ uint32_t first_root_from(const uint32_t* __restrict__ a, uint32_t n, uint32_t v) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__global__ void __launch_bounds__(NT) decide_kernel(const double* __restrict__ rects, int max_cells, int max_out, Ws w,
                                                    double* __restrict__ out, int32_t* n_out, double* __restrict__ info) {
  __shared__ int wsum[4];
  const int R = w.h->rects;
  uint32_t nk = w.h->comps;
  const uint32_t cap = (uint32_t)comps_for(max_cells);
  nk = nk < cap ? nk : cap;
  const int per = (R + NT - 1) / NT;
  const long long r0 = (long long)threadIdx.x * per;
  const long long r1 = r0 + per < R ? r0 + per : R;
  int s = 0, tot = 0;
  for (long long r = r0; r < r1; ++r) {
    const Cand& c = w.cand[r];
    int st = status_before_parts(w, (int)r), listed = 0;
    if (st == 0) {
      const uint32_t k0 = first_root_from(w.croot, nk, (uint32_t)w.celloff[r]);
      const uint32_t k1 = first_root_from(w.croot, nk, (uint32_t)w.celloff[r + 1]);
      double area = 0.0;
      for (uint32_t k = k0; k < k1; ++k) {
        const double* q = w.sub + 6 * (size_t)k;
        if (q[5] != 0.0) { area += q[2] * q[3]; ++listed; }
      }
      const double ratio = area / (rects[8 * r + 2] * rects[8 * r + 3]);
      st = listed < 2 ? ST_PARTS : (0.4 < ratio && ratio < 1.3 ? ST_SPLIT : ST_AREA);
    }
    const bool grid = st != ST_SMALL && st != ST_FEW && st != ST_THIN && st != ST_CAP;
    double* o = info + 8 * r;
    o[0] = (double)st;
    o[1] = st == ST_SMALL ? 0.0 : (double)w.inside[r];
    o[2] = (double)c.gw; o[3] = (double)c.gh;
    o[4] = grid ? (double)w.emptyc[r] : 0.0;
    o[5] = grid && st != ST_FULL && st != ST_RATIO ? (double)w.nocc[r] : 0.0;
    o[6] = (double)listed;
    o[7] = st == ST_CAP ? 1.0 : 0.0;
    w.stat[r] = st;
    w.ocnt[r] = st == ST_SPLIT ? listed : 1;
    s += w.ocnt[r];
  }
  int run = block_excl_scan(s, wsum, &tot);
  for (long long r = r0; r < r1; ++r) {
    const double* in = rects + 8 * r;
    if (w.stat[r] != ST_SPLIT) {
      if (run < max_out)
        for (int a = 0; a < 8; ++a) out[8 * (size_t)run + a] = in[a];
      ++run;
      continue;
    }
    const uint32_t k0 = first_root_from(w.croot, nk, (uint32_t)w.celloff[r]);
    const uint32_t k1 = first_root_from(w.croot, nk, (uint32_t)w.celloff[r + 1]);
    for (uint32_t k = k0; k < k1; ++k) {
      const double* q = w.sub + 6 * (size_t)k;
      if (q[5] == 0.0) continue;
      if (run < max_out) {
        double* o = out + 8 * (size_t)run;
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3]; o[4] = q[4];
        o[5] = in[5]; o[6] = in[6] + 2.0; o[7] = 0.0;
      }
      ++run;
    }
  }
  if (threadIdx.x == 0) {
    n_out[0] = tot < max_out ? tot : max_out;
    n_out[1] = tot > max_out ? 1 : 0;
  }
}

}  // namespace

extern "C" int dp_shape_rectangles(const double* shapes, const int32_t* n_clusters_dev, int32_t max_clusters,
                                   double* rects_out, int32_t* n_rects_dev, dp_stream_t stream) {
  if (!n_clusters_dev || !n_rects_dev || (max_clusters > 0 && (!shapes || !rects_out))) return DP_ERR_ARG;
  if (max_clusters < 0 || max_clusters > (1 << 30)) return DP_ERR_SHAPE;
  hipLaunchKernelGGL(rectangles_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, shapes, n_clusters_dev, max_clusters,
                     rects_out, n_rects_dev);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t dp_lshape_workspace_size(int64_t max_rects, int64_t max_cells) { return ws_bytes_for(max_rects, max_cells); }

extern "C" int dp_lshape_split(const double* points, const int32_t* labels, const int32_t* n_dev, int32_t n_max,
                               const double* rects, const int32_t* n_rects_dev, int32_t max_rects, int32_t max_out,
                               int32_t max_cells, double* rects_out, int32_t* n_out_dev, double* info_out, void* workspace,
                               int64_t workspace_bytes, dp_stream_t stream) {
  if (!n_rects_dev || !n_out_dev || (n_max > 0 && (!points || !labels)) || (max_rects > 0 && (!rects || !info_out)) ||
      (max_out > 0 && !rects_out))
    return DP_ERR_ARG;
  if (n_max < 0 || max_rects < 0 || max_out < 0 || max_cells < 0) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, max_rects, max_cells, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int gc = grid_for(max_cells, GRID_CAP), nb = (int)scan_blocks_for(max_cells);
  hipLaunchKernelGGL(prep_kernel, dim3(1), dim3(NT), 0, s, rects, n_rects_dev, max_rects, max_cells, w);
  if (max_cells > 0) {
    hipError_t e = hipMemsetAsync(w.b, 0, (size_t)max_cells, s);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(raster_kernel, dim3(grid_for(n_max, GRID_CAP)), dim3(NT), 0, s, points, labels, n_dev, n_max, w);
  if (max_cells > 0) {
    hipLaunchKernelGGL(dilate_kernel, dim3(gc), dim3(256), 0, s, w);
    hipLaunchKernelGGL(link_kernel, dim3(gc), dim3(256), 0, s, w, w.e, w.par1);
    hipLaunchKernelGGL(size_kernel, dim3(gc), dim3(256), 0, s, w, w.e, w.par1, w.sz1, (uint32_t*)nullptr);
    hipLaunchKernelGGL(mask_kernel, dim3(gc), dim3(256), 0, s, w);
    hipLaunchKernelGGL(link_kernel, dim3(gc), dim3(256), 0, s, w, w.occ, w.par2);
    hipLaunchKernelGGL(size_kernel, dim3(gc), dim3(256), 0, s, w, w.occ, w.par2, w.sz2, w.nocc);
    hipLaunchKernelGGL(flag_kernel, dim3(gc), dim3(256), 0, s, w);
    hipLaunchKernelGGL(scan_count_kernel, dim3(nb), dim3(256), 0, s, w.flag, &w.h->cells, max_cells, w.bc);
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(256), 0, s, w.bc, nb, &w.h->comps);
    hipLaunchKernelGGL(roots_kernel, dim3(nb), dim3(256), 0, s, w, max_cells);
    hipLaunchKernelGGL(part_kernel, dim3(grid_for(256 * comps_for(max_cells), 1024)), dim3(NT), 0, s, w, max_cells);
  }
  hipLaunchKernelGGL(decide_kernel, dim3(1), dim3(NT), 0, s, rects, max_cells, max_out, w, rects_out, n_out_dev, info_out);
  DP_CHECK_LAUNCH();
  return 0;
}
