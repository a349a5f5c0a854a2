// Cluster shapes (ABI 18): per cluster of a dp_cluster_table call the convex hull, the minimum-area
// rectangle, the least-squares circle and the reference's circle-or-rectangle decision, in the
// top-down frame u = -x, v = z.  fp64 as numpy computes it; no FMA contraction anywhere in this file,
// so each product, sum and difference is rounded on its own.  The specification (rules 1-6) is in
// the header; this file is the method:
//   gather (u, v) into cluster order -> rounds of [plan (one workgroup: two scans) -> hull chunks]
//   -> circle + decision (one workgroup per cluster) -> hull offsets (scan) -> hull rows.
// A hull chunk is at most CHUNK members of one cluster in LDS: bitonic sort by (u, v, position),
// monotone chain (lower hull on one wave, upper hull on another), survivors written back.  The hull
// of a union is the hull of the hulls, so a cluster shrinks round by round until it is one chunk;
// that chunk's hull is the cluster's, and its workgroup goes on to the area and the calipers.
// No kernel waits on another workgroup; the only serial loops are the two chains over one chunk.
#include "dp_common.h"
#include "dp_points.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = HULL_NT;
constexpr int CHUNK = HULL_MAX;                 // members of one hull chunk; also the cap on hull vertices
constexpr int ROUNDS = 6;                       // hull rounds when one chunk cannot hold every cluster
constexpr int LM_EVALS = 50;                    // the circle iteration's cap on trial centres
constexpr uint32_t PAD = HULL_PAD;
constexpr double PI = 3.141592653589793;

struct SHdr {
  int32_t nb[2];                                // hull chunks of the round, by parity
};

// A cluster's range of the cluster-ordered index, kept inside [0, n) whatever `offsets` holds.
__device__ __forceinline__ int off_at(const int32_t* __restrict__ offsets, int c, int n) {
  const int o = offsets[c];
  return o < 0 ? 0 : (o < n ? o : n);
}
__device__ __forceinline__ int count_at(const int32_t* __restrict__ offsets, int c, int n) {
  const int m = off_at(offsets, c + 1, n) - off_at(offsets, c, n);
  return m < 0 ? 0 : m;
}

// sum over the workgroup, the same value in every thread (red: 4 shared doubles)
__device__ __forceinline__ double block_sum(double v, double* red) {
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}

// ---- gather and row reset -----------------------------------------------------------------------
__global__ void __launch_bounds__(NT) init_kernel(const double* __restrict__ pts, const uint32_t* __restrict__ order,
                                                  const int32_t* __restrict__ offsets, const int32_t* n_dev, int n_max,
                                                  const int32_t* ncl, int max_clusters, double2* __restrict__ guv,
                                                  double* __restrict__ shapes, int32_t* __restrict__ hcnt,
                                                  int32_t* __restrict__ done) {
  const int n = live_n(n_dev, n_max), k = table_rows(ncl, max_clusters);
  const int tot = off_at(offsets, k, n);
  for (long long t = (long long)blockIdx.x * NT + threadIdx.x; t < tot; t += (long long)gridDim.x * NT) {
    uint32_t row = order[t];
    row = row < (uint32_t)n ? row : (uint32_t)(n - 1);
    guv[t] = make_double2(-pts[3 * (size_t)row], pts[3 * (size_t)row + 2]);
  }
  for (long long c = (long long)blockIdx.x * NT + threadIdx.x; c < k; c += (long long)gridDim.x * NT) {
    double* row = shapes + 16 * c;
    for (int a = 0; a < 16; ++a) row[a] = 0.0;
    row[1] = (double)count_at(offsets, (int)c, n);
    hcnt[c] = 0;
    done[c] = 0;
  }
}

// ---- the round's plan: one workgroup ------------------------------------------------------------
// Round 0 takes the clusters' ranges from `offsets`.  A later round first scans the previous round's
// survivor counts (ppos: where each previous chunk's survivors start in the round's own numbering),
// takes each cluster's range from that, and then, as round 0, cuts every range into chunks and scans
// the chunk counts (cstart: the first chunk of each cluster).
__global__ void __launch_bounds__(NT) plan_kernel(int round, const int32_t* __restrict__ offsets, const int32_t* n_dev,
                                                  int n_max, const int32_t* ncl, int max_clusters, SHdr* h,
                                                  const int32_t* __restrict__ cstart_prev, const int32_t* __restrict__ ocnt_prev,
                                                  int32_t* __restrict__ ppos, int32_t* __restrict__ lbeg,
                                                  int32_t* __restrict__ lcnt, int32_t* __restrict__ cstart) {
  __shared__ int wsum[4];
  const int n = live_n(n_dev, n_max), k = table_rows(ncl, max_clusters);
  const int cur = round & 1;
  if (round > 0) {
    const int nbp = h->nb[cur ^ 1];
    const int per = (nbp + NT - 1) / NT;
    const long long b0 = (long long)threadIdx.x * per;
    const long long b1 = b0 + per < nbp ? b0 + per : nbp;
    int s = 0, tot = 0;
    for (long long b = b0; b < b1; ++b) s += ocnt_prev[b];
    int run = block_excl_scan(s, wsum, &tot);
    for (long long b = b0; b < b1; ++b) {
      ppos[b] = run;
      run += ocnt_prev[b];
    }
    if (threadIdx.x == 0) ppos[nbp] = tot;
    __syncthreads();
  }
  const int per = (k + NT - 1) / NT;
  const long long c0 = (long long)threadIdx.x * per;
  const long long c1 = c0 + per < k ? c0 + per : k;
  int s = 0, tot = 0;
  for (long long c = c0; c < c1; ++c) {
    int beg, m;
    if (round == 0) {
      beg = off_at(offsets, (int)c, n);
      m = count_at(offsets, (int)c, n);
      if (m < 5) m = 0;                                          // rule 1: skipped
    } else {
      beg = ppos[cstart_prev[c]];
      m = ppos[cstart_prev[c + 1]] - beg;                        // 0 once the cluster is finished
    }
    lbeg[c] = beg;
    lcnt[c] = m;
    s += (m + CHUNK - 1) / CHUNK;
  }
  int run = block_excl_scan(s, wsum, &tot);
  for (long long c = c0; c < c1; ++c) {
    cstart[c] = run;
    run += (lcnt[c] + CHUNK - 1) / CHUNK;
  }
  if (threadIdx.x == 0) {
    cstart[k] = tot;
    h->nb[cur] = tot;
  }
}

// ---- one hull chunk per workgroup ---------------------------------------------------------------
// (the chunk's LDS, its sort, chain and calipers: dp_points.h)
__global__ void __launch_bounds__(NT) hull_kernel(int round, const double2* __restrict__ guv, const uint32_t* __restrict__ order,
                                                  const int32_t* __restrict__ offsets, const int32_t* n_dev, int n_max,
                                                  const int32_t* ncl, int max_clusters, const SHdr* h,
                                                  const int32_t* __restrict__ cstart, const int32_t* __restrict__ lbeg,
                                                  const int32_t* __restrict__ lcnt, const int32_t* __restrict__ ppos,
                                                  const int32_t* __restrict__ pstart_prev, const uint32_t* __restrict__ buf_prev,
                                                  uint32_t* __restrict__ buf, int32_t* __restrict__ pstart,
                                                  int32_t* __restrict__ ocnt, uint32_t* __restrict__ hstage,
                                                  int32_t* __restrict__ hcnt, int32_t* __restrict__ done,
                                                  double* __restrict__ shapes) {
  __shared__ HullLds s;
  __shared__ double red[4];
  __shared__ int cnt[2];
  const int cur = round & 1, tid = threadIdx.x;
  const int b = blockIdx.x;
  if (b >= h->nb[cur]) return;
  const int n = live_n(n_dev, n_max), k = table_rows(ncl, max_clusters);
  const int c = upper_bound(cstart, k + 1, b) - 1;
  if (c < 0 || c >= k) return;
  const int j = b - cstart[c];
  const bool last = cstart[c + 1] - cstart[c] == 1;             // the whole cluster: this hull is final
  const int in_lo = lbeg[c] + j * CHUNK;
  int m = lcnt[c] - j * CHUNK;
  m = m < CHUNK ? m : CHUNK;
  if (m <= 0 || in_lo < 0 || in_lo > n - m) return;             // cannot happen; keeps every access inside n
  int P = 1;
  while (P < m) P <<= 1;

  // load: position in cluster order (through the previous round's chunks), its (u, v)
  const int nbp = round > 0 ? h->nb[cur ^ 1] : 0;
  for (int i = tid; i < P; i += NT) {
    uint32_t t = PAD;
    double2 p = make_double2(0.0, 0.0);
    if (i < m) {
      const int q = in_lo + i;
      if (round == 0) {
        t = (uint32_t)q;
      } else {
        int bp = upper_bound(ppos, nbp + 1, q) - 1;
        bp = bp < 0 ? 0 : (bp < nbp ? bp : nbp - 1);
        long long ph = (long long)pstart_prev[bp] + (q - ppos[bp]);
        ph = ph < 0 ? 0 : (ph < n ? ph : n - 1);
        t = buf_prev[ph];
        t = t < (uint32_t)n ? t : (uint32_t)(n - 1);
      }
      p = guv[t];
    }
    s.st[i] = t;
    s.su[i] = p.x;
    s.sv[i] = p.y;
  }
  __syncthreads();

  // sort by (u, v, position): a position is a row rank inside the cluster, so coincident members come
  // smallest row first; then the chain
  int kl;
  const int hn = hull_sort_chain(s, m, P, cnt, &kl);            // counter-clockwise from the smallest (u, v)

  // the hull's members into registers (CHUNK / NT = 8 per thread)
  double hu[CHUNK / NT], hv[CHUNK / NT];
  uint32_t ht[CHUNK / NT];
  #pragma unroll
  for (int r = 0; r < CHUNK / NT; ++r) {
    const int e = tid + r * NT;
    hu[r] = hv[r] = 0.0;
    ht[r] = 0;
    if (e < hn) {
      const int i = hull_vertex(s, kl, e);
      hu[r] = s.su[i]; hv[r] = s.sv[i]; ht[r] = s.st[i];
    }
  }
  if (!last) {
    #pragma unroll
    for (int r = 0; r < CHUNK / NT; ++r) {
      const int e = tid + r * NT;
      if (e < hn) buf[in_lo + e] = ht[r];
    }
    if (tid == 0) { pstart[b] = in_lo; ocnt[b] = hn; }
    return;
  }
  if (tid == 0) { pstart[b] = in_lo; ocnt[b] = 0; }

  // ---- the cluster's hull: rows out, vertices to the front of LDS, area, calipers ----
  const int obeg = off_at(offsets, c, n);
  __syncthreads();
  #pragma unroll
  for (int r = 0; r < CHUNK / NT; ++r) {
    const int e = tid + r * NT;
    if (e < hn) {
      s.su[e] = hu[r]; s.sv[e] = hv[r];
      if (obeg + e < n) hstage[obeg + e] = order[ht[r]];
    }
  }
  __syncthreads();
  double* row = shapes + 16 * (size_t)c;
  // rule 2: half the sum of o(p0, p_i, p_i+1), every term of a strict hull positive
  double part = 0.0;
  for (int i = 1 + tid; i < hn - 1; i += NT) part += orient(s.su[0], s.sv[0], s.su[i], s.sv[i], s.su[i + 1], s.sv[i + 1]);
  const double area2 = block_sum(part, red);

  if (tid == 0) {
    hcnt[c] = hn;
    done[c] = 1;
    row[12] = area2 / 2.0;
    row[13] = (double)hn;
  }
  hull_min_rect(s, hn, row + 2);                                 // rule 3: centre, width, height, angle, area
}

// ---- circle and decision: one workgroup per cluster -----------------------------------------------
// the nine sums of one trial centre, the same values in every thread
struct Eval { double sR, sa, sb, saa, sab, sbb, saR, sbR, sRR; };
__device__ __forceinline__ Eval eval_at(const double2* __restrict__ g, int m, double x, double y, double* red9) {
  double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < m; i += NT) {
    const double2 p = g[i];
    const double du = p.x - x, dv = p.y - y;
    const double R = __builtin_sqrt(du * du + dv * dv);
    const double a = R == 0.0 ? 0.0 : du / R, bb = R == 0.0 ? 0.0 : dv / R;
    v[0] += R; v[1] += a; v[2] += bb; v[3] += a * a; v[4] += a * bb; v[5] += bb * bb; v[6] += a * R; v[7] += bb * R;
    v[8] += R * R;
  }
  #pragma unroll
  for (int a = 0; a < 9; ++a) {
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[a] += __shfl_xor(v[a], o);
    if ((threadIdx.x & 63) == 0) red9[(threadIdx.x >> 6) * 9 + a] = v[a];
  }
  __syncthreads();
  #pragma unroll
  for (int a = 0; a < 9; ++a) v[a] = ((red9[a] + red9[9 + a]) + red9[18 + a]) + red9[27 + a];
  __syncthreads();
  Eval e;
  e.sR = v[0]; e.sa = v[1]; e.sb = v[2]; e.saa = v[3]; e.sab = v[4]; e.sbb = v[5]; e.saR = v[6]; e.sbR = v[7]; e.sRR = v[8];
  return e;
}

__global__ void __launch_bounds__(NT) circle_kernel(const double2* __restrict__ guv, const int32_t* __restrict__ offsets,
                                                    const int32_t* n_dev, int n_max, const int32_t* ncl, int max_clusters,
                                                    double thr, int32_t* __restrict__ hcnt, const int32_t* __restrict__ done,
                                                    double* __restrict__ shapes) {
  __shared__ double red[4], red9[36];
  const int n = live_n(n_dev, n_max), k = table_rows(ncl, max_clusters);
  const int c = blockIdx.x;
  if (c >= k) return;
  const int m = count_at(offsets, c, n);
  if (m < 5) return;                                             // rule 1: the row stays kind 0
  double* row = shapes + 16 * (size_t)c;
  if (!done[c]) {                                                // the hull did not get down to H_MAX
    if (threadIdx.x == 0) { row[15] = 1.0; hcnt[c] = 0; }
    return;
  }
  const double2* g = guv + off_at(offsets, c, n);
  const double N = (double)m;
  double su = 0.0, sv = 0.0;
  for (int i = threadIdx.x; i < m; i += NT) { su += g[i].x; sv += g[i].y; }
  double x = block_sum(su, red) / N, y = block_sum(sv, red) / N;
  Eval e = eval_at(g, m, x, y, red9);
  double lam = 1e-3;
  for (int it = 0; it < LM_EVALS; ++it) {
    const double Rm = e.sR / N;
    const double A11 = e.saa - e.sa * e.sa / N, A12 = e.sab - e.sa * e.sb / N, A22 = e.sbb - e.sb * e.sb / N;
    const double g1 = e.saR - e.sa * Rm, g2 = e.sbR - e.sb * Rm;
    const double cost = e.sRR - e.sR * Rm;
    const double M11 = A11 * (1.0 + lam), M22 = A22 * (1.0 + lam);
    const double det = M11 * M22 - A12 * A12;
    if (!(det > 0.0)) break;
    const double dx = (M22 * g1 - A12 * g2) / det, dy = (M11 * g2 - A12 * g1) / det;
    const Eval t = eval_at(g, m, x + dx, y + dy, red9);
    const double cost_t = t.sRR - t.sR * (t.sR / N);
    if (cost_t <= cost) {
      x = x + dx; y = y + dy; e = t;
      lam = lam / 10.0;
      if (__builtin_sqrt(dx * dx + dy * dy) <= 1e-13 * (t.sR / N)) break;
    } else {
      lam = lam * 10.0;
      if (lam > 1e10) break;
    }
  }
  const double r = e.sR / N;
  double part = 0.0;
  for (int i = threadIdx.x; i < m; i += NT) {
    const double du = g[i].x - x, dv = g[i].y - y;
    const double d = __builtin_sqrt(du * du + dv * dv) - r;
    part += d * d;
  }
  const double err = block_sum(part, red) / N / (r * r);
  if (threadIdx.x == 0) {
    const double harea = row[12], ra = row[7], ca = PI * (r * r);
    double circ = 0.0;
    bool circle = false;
    if (row[13] >= 3.0 && harea > 0.0) {                         // rule 5
      circ = harea / ca;
      const double inv = 1.0 / circ;
      circ = inv < circ ? inv : circ;
      const double big = ra > ca ? ra : ca;
      circle = circ > thr && err < 0.15 && __builtin_fabs(ca - ra) / big < 0.3;
    }
    row[0] = circle ? 2.0 : 1.0;
    row[8] = x; row[9] = y; row[10] = r; row[11] = err;
    row[14] = circ;
  }
}

// ---- hull ranges: one scan, then the rows ---------------------------------------------------------
__global__ void __launch_bounds__(NT) hoff_kernel(const int32_t* ncl, int max_clusters, const int32_t* __restrict__ hcnt,
                                                  int32_t* __restrict__ hoff) {
  __shared__ int wsum[4];
  const int k = table_rows(ncl, max_clusters);
  const int per = (k + NT - 1) / NT;
  const long long c0 = (long long)threadIdx.x * per;
  const long long c1 = c0 + per < k ? c0 + per : k;
  int s = 0, tot = 0;
  for (long long c = c0; c < c1; ++c) s += hcnt[c];
  int run = block_excl_scan(s, wsum, &tot);
  for (long long c = c0; c < c1; ++c) {
    hoff[c] = run;
    run += hcnt[c];
  }
  if (threadIdx.x == 0) hoff[k] = tot;
}

__global__ void __launch_bounds__(NT) hrows_kernel(const int32_t* __restrict__ offsets, const int32_t* n_dev, int n_max,
                                                   const int32_t* ncl, int max_clusters, const int32_t* __restrict__ hcnt,
                                                   const int32_t* __restrict__ hoff, const uint32_t* __restrict__ hstage,
                                                   int32_t* __restrict__ hull_rows) {
  const int n = live_n(n_dev, n_max), k = table_rows(ncl, max_clusters);
  for (int c = blockIdx.x; c < k; c += gridDim.x) {
    const int beg = off_at(offsets, c, n), to = hoff[c], hn = hcnt[c];
    for (int i = threadIdx.x; i < hn; i += NT)
      if (beg + i < n && to + i < n) hull_rows[to + i] = (int32_t)hstage[beg + i];
  }
}

// hull chunks of one round at the most: every cluster with a chunk has >= 5 members
int64_t max_chunks(int64_t n, int64_t k) {
  const int64_t by5 = n / 5;
  return n / CHUNK + (k < by5 ? k : by5) + 1;
}

struct Ws {
  SHdr* h;
  double2* guv;
  uint32_t *buf[2], *hstage;
  int32_t *lbeg, *lcnt, *cstart[2], *hcnt, *done, *pstart[2], *ocnt[2], *ppos;
};
int64_t ws_bytes_for(int64_t n_max, int64_t max_clusters) {
  const int64_t n = n_max < 0 ? 0 : n_max, k = max_clusters < 0 ? 0 : max_clusters, b = max_chunks(n, k);
  return al256(sizeof(SHdr)) + al256(16 * n) + 3 * al256(4 * n) + 6 * al256(4 * (k + 1)) + 4 * al256(4 * b) +
         al256(4 * (b + 1)) + 256;
}
bool ws_carve(void* ws, int64_t bytes, int64_t n, int64_t k, Ws* o) {
  if (!ws || bytes < ws_bytes_for(n, k) || ((uintptr_t)ws & 7)) return false;
  const int64_t b = max_chunks(n, k);
  char* p = (char*)ws;
  o->h = (SHdr*)p;             p += al256(sizeof(SHdr));
  o->guv = (double2*)p;        p += al256(16 * n);
  o->buf[0] = (uint32_t*)p;    p += al256(4 * n);
  o->buf[1] = (uint32_t*)p;    p += al256(4 * n);
  o->hstage = (uint32_t*)p;    p += al256(4 * n);
  o->lbeg = (int32_t*)p;       p += al256(4 * (k + 1));
  o->lcnt = (int32_t*)p;       p += al256(4 * (k + 1));
  o->cstart[0] = (int32_t*)p;  p += al256(4 * (k + 1));
  o->cstart[1] = (int32_t*)p;  p += al256(4 * (k + 1));
  o->hcnt = (int32_t*)p;       p += al256(4 * (k + 1));
  o->done = (int32_t*)p;       p += al256(4 * (k + 1));
  o->pstart[0] = (int32_t*)p;  p += al256(4 * b);
  o->pstart[1] = (int32_t*)p;  p += al256(4 * b);
  o->ocnt[0] = (int32_t*)p;    p += al256(4 * b);
  o->ocnt[1] = (int32_t*)p;    p += al256(4 * b);
  o->ppos = (int32_t*)p;
  return true;
}
}  // namespace

extern "C" int64_t dp_shapes_workspace_size(int64_t n_max, int64_t max_clusters) { return ws_bytes_for(n_max, max_clusters); }

extern "C" int dp_cluster_shapes(const double* points, const int32_t* n_dev, int32_t n_max, const uint32_t* order,
                                 const int32_t* offsets, const int32_t* n_clusters_dev, int32_t max_clusters,
                                 double circularity_threshold, double* shapes_out, int32_t* hull_rows_out,
                                 int32_t* hull_offsets_out, void* workspace, int64_t workspace_bytes, dp_stream_t stream) {
  if (!n_clusters_dev || !offsets || !hull_offsets_out || (max_clusters > 0 && !shapes_out) ||
      (n_max > 0 && (!points || !order || !hull_rows_out)))
    return DP_ERR_ARG;
  if (n_max < 0 || max_clusters < 0 || circularity_threshold != circularity_threshold) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, n_max, max_clusters, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int g = grid_for(n_max > max_clusters ? n_max : max_clusters, 4096);
  const int gb = (int)max_chunks(n_max, max_clusters), gc = max_clusters < 1 ? 1 : max_clusters;
  hipLaunchKernelGGL(init_kernel, dim3(g), dim3(NT), 0, s, points, order, offsets, n_dev, n_max, n_clusters_dev, max_clusters,
                     w.guv, shapes_out, w.hcnt, w.done);
  const int rounds = n_max <= CHUNK ? 1 : ROUNDS;               // one chunk holds any cluster of <= CHUNK rows
  for (int r = 0; r < rounds; ++r) {
    const int cur = r & 1, prv = cur ^ 1;
    hipLaunchKernelGGL(plan_kernel, dim3(1), dim3(NT), 0, s, r, offsets, n_dev, n_max, n_clusters_dev, max_clusters, w.h,
                       w.cstart[prv], w.ocnt[prv], w.ppos, w.lbeg, w.lcnt, w.cstart[cur]);
    hipLaunchKernelGGL(hull_kernel, dim3(gb), dim3(NT), 0, s, r, w.guv, order, offsets, n_dev, n_max, n_clusters_dev,
                       max_clusters, w.h, w.cstart[cur], w.lbeg, w.lcnt, w.ppos, w.pstart[prv], w.buf[prv], w.buf[cur],
                       w.pstart[cur], w.ocnt[cur], w.hstage, w.hcnt, w.done, shapes_out);
  }
  hipLaunchKernelGGL(circle_kernel, dim3(gc), dim3(NT), 0, s, w.guv, offsets, n_dev, n_max, n_clusters_dev, max_clusters,
                     circularity_threshold, w.hcnt, w.done, shapes_out);
  hipLaunchKernelGGL(hoff_kernel, dim3(1), dim3(NT), 0, s, n_clusters_dev, max_clusters, w.hcnt, hull_offsets_out);
  hipLaunchKernelGGL(hrows_kernel, dim3(gc < 4096 ? gc : 4096), dim3(NT), 0, s, offsets, n_dev, n_max, n_clusters_dev,
                     max_clusters, w.hcnt, hull_offsets_out, w.hstage, hull_rows_out);
  DP_CHECK_LAUNCH();
  return 0;
}
