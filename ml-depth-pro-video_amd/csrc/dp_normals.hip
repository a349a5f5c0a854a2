// Oriented mesh points (ABI 19): voxel-grid down-sampling, the hybrid (radius + max_nn) neighbour search
// and PCA normals oriented towards a camera -- the three Open3D calls every meshing method of the
// reference starts with (pointcloud_to_mesh.py:313-395).  The specification is in dp_mi355x.h.  fp64, no
// FMA contraction anywhere in this file.  The grid (cell keys, cell rows by binary search, the top-k merge)
// is dp_grid3.h's; the sort is dp_clean.hip's, called through its exported entry point dp_sort_pairs.
#include "dp_common.h"
#include "dp_grid3.h"

#pragma clang fp contract(off)

namespace {

constexpr int GRID_CAP = 4096;                  // workgroups of a per-point kernel at the most
constexpr int MAX_NN = 64;                      // one kept neighbour per lane

struct Hdr {
  Grid3 g;
  uint32_t ctr[2];
};
enum { C_FEW = 0, C_TRUNC = 1 };

__global__ void hdr_init_kernel(Hdr* h) {
  grid3_reset(&h->g);
  h->ctr[C_FEW] = h->ctr[C_TRUNC] = 0;
}

// ---- voxel grid -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) vox_flag_kernel(const u64* __restrict__ keys, const int32_t* n_dev, int n_max,
                                                       uint8_t* __restrict__ flag) {
  const int n = live_n(n_dev, n_max);
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256) {
    const u64 k = keys[t];
    flag[t] = k != NO_KEY && (t == 0 || keys[t - 1] != k);
  }
}

// Third step of the head flags' scan (dp_points.h): the voxel of every sorted position, voxel_of for its
// row, the run's head position, and the end of the last run.  head has n_max + 1 entries.
__global__ void __launch_bounds__(256) vox_rank_kernel(const u64* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                       const uint8_t* __restrict__ flag, const int32_t* n_dev, int n_max,
                                                       const uint32_t* __restrict__ bc, int32_t* __restrict__ voxel_of,
                                                       uint32_t* __restrict__ head) {
  __shared__ uint32_t wsum[4];
  const int n = live_n(n_dev, n_max);
  const long long tile = (long long)blockIdx.x * SCAN_TILE;
  uint32_t run = bc[blockIdx.x];
  for (int r = 0; r < SCAN_ITEMS && tile + r * 256 < n; ++r) {
    const long long t = tile + r * 256 + threadIdx.x;
    const bool in = t < n;
    const uint32_t f = in ? flag[t] : 0u;
    uint32_t tot = 0;
    const uint32_t excl = run + block_excl_scan(f, wsum, &tot);
    if (in) {
      const uint32_t row = vals[t];
      const bool valid = keys[t] != NO_KEY;
      const uint32_t v = excl + f - 1u;                 // heads at positions <= t, minus one (valid rows only)
      if (row < (uint32_t)n) voxel_of[row] = valid ? (int32_t)v : -1;
      if (valid && v < (uint32_t)n) {
        if (f) head[v] = (uint32_t)t;
        if (t == n - 1 || keys[t + 1] == NO_KEY) head[v + 1] = (uint32_t)(t + 1);
      }
    }
    run += tot;
  }
}

// One wave per voxel: lanes stride the run, butterfly sums.  Members are in row order (the sort is stable).
__global__ void __launch_bounds__(256) vox_reduce_kernel(const double* __restrict__ pts, const uint8_t* __restrict__ cols,
                                                         const uint32_t* __restrict__ vals, const uint32_t* __restrict__ head,
                                                         const int32_t* n_dev, int n_max, const int32_t* n_out_dev,
                                                         double* __restrict__ pts_out, uint8_t* __restrict__ cols_out,
                                                         int32_t* __restrict__ count_out) {
  const int n = live_n(n_dev, n_max), lane = threadIdx.x & 63;
  const int n_out = live_n(n_out_dev, n);
  for (long long v = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); v < n_out; v += (long long)gridDim.x * 4) {
    uint32_t a = head[v], b = head[v + 1];
    b = b < (uint32_t)n ? b : (uint32_t)n;
    a = a < b ? a : b;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    u64 sr = 0, sg = 0, sb = 0;
    for (uint32_t c = a + lane; c < b; c += 64) {
      const size_t i = row_of(vals[c], n);
      sx += pts[3 * i]; sy += pts[3 * i + 1]; sz += pts[3 * i + 2];
      if (cols) { sr += cols[3 * i]; sg += cols[3 * i + 1]; sb += cols[3 * i + 2]; }
    }
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sx += __shfl_xor(sx, o); sy += __shfl_xor(sy, o); sz += __shfl_xor(sz, o);
      sr += __shfl_xor(sr, o); sg += __shfl_xor(sg, o); sb += __shfl_xor(sb, o);
    }
    if (lane == 0) {
      const u64 m = b - a;
      const double dm = (double)m;
      pts_out[3 * v] = sx / dm; pts_out[3 * v + 1] = sy / dm; pts_out[3 * v + 2] = sz / dm;
      count_out[v] = (int32_t)m;
      if (cols && m) {                                  // rounds half up
        cols_out[3 * v] = (uint8_t)((2 * sr + m) / (2 * m));
        cols_out[3 * v + 1] = (uint8_t)((2 * sg + m) / (2 * m));
        cols_out[3 * v + 2] = (uint8_t)((2 * sb + m) / (2 * m));
      }
    }
  }
}

__global__ void vox_final_kernel(const Hdr* h, const int32_t* n_out_dev, double* st) {
  st[0] = (double)h->g.finite;
  st[1] = (double)h->g.nonfinite;
  st[2] = (double)*n_out_dev;
  st[3] = st[4] = 0.0;
  st[5] = (double)h->g.err;
  st[6] = st[7] = 0.0;
}

// ---- hybrid search --------------------------------------------------------------------------------
// One wave per query, in sorted (cell) order.  Cell edge radius * EDGE_SLACK: the 3 x 3 x 3 cells around a
// point hold every true neighbour (the argument stands at EDGE_SLACK, dp_grid3.h); a (x, y) cell row's
// three z-adjacent cells are one key range.  Lanes stride a range's candidates in batches of 64, and each
// batch goes to wave_top64_merge with the running best, held one per lane in ascending (d2, row) order.
__global__ void __launch_bounds__(256) knn_kernel(const u64* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                  const double* __restrict__ sp, const int32_t* n_dev, int n_max,
                                                  double r2, int max_nn, Hdr* h, int32_t* __restrict__ nbr,
                                                  int32_t* __restrict__ nbr_count) {
  const int n = live_n(n_dev, n_max), lane = threadIdx.x & 63;
  uint32_t few = 0, trunc = 0;                            // this wave's counters (lane-uniform)
  for (long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); q < n; q += (long long)gridDim.x * 4) {
    const u64 key = keys[q];
    const uint32_t row = idx[q];
    if (row >= (uint32_t)n) continue;                     // never, for a consistent sort
    u64 bk = NO_KEY;
    uint32_t br = ~0u;
    uint32_t total = 0;
    if (key != NO_KEY) {
      int cx, cy, cz;
      unpack_cell(key, cx, cy, cz);
      const double x = sp[3 * q], y = sp[3 * q + 1], z = sp[3 * q + 2];
      for (int rr = 0; rr < 9; ++rr) {
        const int rx = cx + rr / 3 - 1, ry = cy + rr % 3 - 1;
        if (rx < 0 || ry < 0 || rx > CELL_MAX + 1 || ry > CELL_MAX + 1) continue;
        int a, b;
        cell_row_range(keys, n, rx, ry, cz > 0 ? cz - 1 : 0, cz + 1, a, b);
        for (int base = a; base < b; base += 64) {
          const int c = base + lane;
          bool hit = false;
          u64 ck = NO_KEY;
          uint32_t cr = ~0u;
          if (c < b) {
            const double dx = sp[3 * (size_t)c] - x, dy = sp[3 * (size_t)c + 1] - y, dz = sp[3 * (size_t)c + 2] - z;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            hit = d2 < r2;
            if (hit) { ck = (u64)__double_as_longlong(d2); cr = idx[c]; }
          }
          total += (uint32_t)__popcll(__ballot(hit));
          wave_top64_merge(hit, ck, cr, max_nn, lane, bk, br);      // q, rr and base are the wave's: uniform here
        }
      }
      few += total < 3u;
      trunc += total > (uint32_t)max_nn;
    }
    const uint32_t cnt = total < (uint32_t)max_nn ? total : (uint32_t)max_nn;
    if (lane < max_nn) nbr[(size_t)row * max_nn + lane] = (uint32_t)lane < cnt && br < (uint32_t)n ? (int32_t)br : -1;
    if (lane == 0) nbr_count[row] = (int32_t)cnt;
  }
  if (lane == 0) {
    if (few) atomicAdd(&h->ctr[C_FEW], few);
    if (trunc) atomicAdd(&h->ctr[C_TRUNC], trunc);
  }
}

__global__ void knn_final_kernel(const Hdr* h, double* st) {
  const bool err = h->g.err != 0;
  st[0] = (double)h->g.finite;
  st[1] = (double)h->g.nonfinite;
  st[2] = err ? (double)h->g.finite : (double)h->ctr[C_FEW];          // no neighbourhood at all under the flag
  st[3] = (double)h->ctr[C_TRUNC];
  st[4] = 0.0;
  st[5] = (double)h->g.err;
  st[6] = st[7] = 0.0;
}

// ---- normals --------------------------------------------------------------------------------------
// One Jacobi rotation of the symmetric 3 x 3 in the (p, q) plane; r is the third index.  v*p / v*q are
// the eigenvector matrix's columns p and q.
__device__ __forceinline__ void jacobi_rot(double& app, double& aqq, double& apq, double& apr, double& aqr,
                                           double& v0p, double& v1p, double& v2p, double& v0q, double& v1q, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta < 0.0 ? -1.0 : 1.0) / (__builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0));
  const double c = 1.0 / __builtin_sqrt(t * t + 1.0), s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0;
  const double pr = apr, qr = aqr;
  apr = c * pr - s * qr;
  aqr = s * pr + c * qr;
  const double a0 = v0p, a1 = v1p, a2 = v2p;
  v0p = c * a0 - s * v0q; v0q = s * a0 + c * v0q;
  v1p = c * a1 - s * v1q; v1q = s * a1 + c * v1q;
  v2p = c * a2 - s * v2q; v2q = s * a2 + c * v2q;
}

// One thread per row; stats_out is zeroed before the launch, takes the counts as 64-bit integers and is
// turned into fp64 in place by normals_final_kernel.
__global__ void __launch_bounds__(256) normals_kernel(const double* __restrict__ pts, const int32_t* n_dev, int n_max,
                                                      const int32_t* __restrict__ nbr, const int32_t* __restrict__ nbr_count,
                                                      int max_nn, double camx, double camy, double camz, int orient,
                                                      double* __restrict__ normals, double* st) {
  const int n = live_n(n_dev, n_max);
  uint32_t c_fin = 0, c_bad = 0, c_few = 0, c_flip = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const double px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    if (!finite3(px, py, pz)) {
      ++c_bad;
      normals[3 * i] = 0.0; normals[3 * i + 1] = 0.0; normals[3 * i + 2] = 0.0;
      continue;
    }
    ++c_fin;
    int m = nbr_count[i];
    m = m < 0 ? 0 : (m > max_nn ? max_nn : m);
    const int32_t* list = nbr + (size_t)i * max_nn;
    double nx = 0.0, ny = 0.0, nz = 1.0;
    // an entry outside [0, n) is no row: the list ends there
    int mm = 0;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int k = 0; k < m; ++k) {
      const int32_t j = list[k];
      if ((uint32_t)j >= (uint32_t)n) break;
      sx += pts[3 * (size_t)j]; sy += pts[3 * (size_t)j + 1]; sz += pts[3 * (size_t)j + 2];
      ++mm;
    }
    if (mm < 3) {
      ++c_few;
    } else {
      const double dm = (double)mm, mx = sx / dm, my = sy / dm, mz = sz / dm;
      double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
      for (int k = 0; k < mm; ++k) {
        const size_t j = (size_t)list[k];
        const double dx = pts[3 * j] - mx, dy = pts[3 * j + 1] - my, dz = pts[3 * j + 2] - mz;
        a00 += dx * dx; a01 += dx * dy; a02 += dx * dz; a11 += dy * dy; a12 += dy * dz; a22 += dz * dz;
      }
      a00 /= dm; a01 /= dm; a02 /= dm; a11 /= dm; a12 /= dm; a22 /= dm;
      // cyclic Jacobi: (0,1), (0,2), (1,2) per sweep; converged when the off-diagonal part no longer counts
      double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
      // (below 2^-53 of the diagonal; a rotation zeroes its element exactly, so the sum reaches that or 0)
      for (int sweep = 0; sweep < 24; ++sweep) {
        const double off = (__builtin_fabs(a01) + __builtin_fabs(a02)) + __builtin_fabs(a12);
        const double dia = (__builtin_fabs(a00) + __builtin_fabs(a11)) + __builtin_fabs(a22);
        if (!(off > 0.0) || dia + off == dia) break;
        jacobi_rot(a00, a11, a01, a02, a12, v00, v10, v20, v01, v11, v21);
        jacobi_rot(a00, a22, a02, a01, a12, v00, v10, v20, v02, v12, v22);
        jacobi_rot(a11, a22, a12, a01, a02, v01, v11, v21, v02, v12, v22);
      }
      // the smallest eigenvalue's column (the lowest index on a tie)
      const bool s1 = a11 < a00;
      const double e1 = s1 ? a11 : a00;
      const bool s2 = a22 < e1;
      const double ex = s2 ? v02 : (s1 ? v01 : v00), ey = s2 ? v12 : (s1 ? v11 : v10), ez = s2 ? v22 : (s1 ? v21 : v20);
      const double len = __builtin_sqrt((ex * ex + ey * ey) + ez * ez);
      if (len > 0.0 && len < __builtin_inf()) { nx = ex / len; ny = ey / len; nz = ez / len; }
    }
    if (orient) {
      const double d = (nx * (camx - px) + ny * (camy - py)) + nz * (camz - pz);
      if (d < 0.0) { nx = -nx; ny = -ny; nz = -nz; ++c_flip; }
    }
    normals[3 * i] = nx; normals[3 * i + 1] = ny; normals[3 * i + 2] = nz;
  }
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    c_fin += __shfl_xor(c_fin, o); c_bad += __shfl_xor(c_bad, o);
    c_few += __shfl_xor(c_few, o); c_flip += __shfl_xor(c_flip, o);
  }
  if ((threadIdx.x & 63) == 0) {
    u64* ctr = (u64*)st;
    if (c_fin) atomicAdd(&ctr[0], (u64)c_fin);
    if (c_bad) atomicAdd(&ctr[1], (u64)c_bad);
    if (c_few) atomicAdd(&ctr[2], (u64)c_few);
    if (c_flip) atomicAdd(&ctr[4], (u64)c_flip);
  }
}

__global__ void normals_final_kernel(double* st) {
  for (int a = 0; a < 8; ++a) st[a] = (double)((const u64*)st)[a];
}

// ---- workspace ------------------------------------------------------------------------------------
struct Ws {
  Hdr* h;
  u64* keys;
  uint32_t *vals, *head, *bc;
  uint8_t* flag;
  double* sp;
  void* sort;
  int64_t sort_bytes;
};
int64_t ws_bytes_for(int64_t n_max) {
  const int64_t n = n_max < 0 ? 0 : n_max;
  return al256(sizeof(Hdr)) + al256(8 * n) + al256(4 * n) + al256(4 * (n + 1)) + al256(4 * (scan_blocks_for(n) + 1)) + al256(n) +
         al256(24 * n) + al256(dp_clean_workspace_size(n)) + 256;
}
bool ws_carve(void* ws, int64_t bytes, int n_max, Ws* o) {
  if (!ws || bytes < ws_bytes_for(n_max) || ((uintptr_t)ws & 7)) return false;
  const int64_t n = n_max;
  char* p = (char*)ws;
  o->h = (Hdr*)p;          p += al256(sizeof(Hdr));
  o->keys = (u64*)p;       p += al256(8 * n);
  o->vals = (uint32_t*)p;  p += al256(4 * n);
  o->head = (uint32_t*)p;  p += al256(4 * (n + 1));
  o->bc = (uint32_t*)p;    p += al256(4 * (scan_blocks_for(n) + 1));
  o->flag = (uint8_t*)p;   p += al256(n);
  o->sp = (double*)p;      p += al256(24 * n);
  o->sort = p;
  o->sort_bytes = dp_clean_workspace_size(n);
  return true;
}

// minimum / maximum, cell keys of edge `edge` from origin min - shift, sorted by (cell, row)
int sorted_cells(hipStream_t s, const Ws& w, const double* points, const int32_t* n_dev, int n_max, double edge, double shift) {
  hipLaunchKernelGGL(hdr_init_kernel, dim3(1), dim3(1), 0, s, w.h);
  grid3_keys(s, &w.h->g, grid_for(n_max, GRID_CAP), points, n_dev, n_max, edge, shift, w.keys, w.vals);
  return dp_sort_pairs((uint64_t*)w.keys, w.vals, n_dev, n_max, 0, 64, w.sort, w.sort_bytes, (dp_stream_t)s);
}

}  // namespace

extern "C" int64_t dp_normals_workspace_size(int64_t n_max) { return ws_bytes_for(n_max); }

extern "C" int dp_voxel_downsample(const double* points, const uint8_t* colors, const int32_t* n_dev, int32_t n_max,
                                   double voxel_size, double* points_out, uint8_t* colors_out, int32_t* count_out,
                                   int32_t* voxel_of_out, int32_t* n_out_dev, double* stats_out, void* workspace,
                                   int64_t workspace_bytes, dp_stream_t stream) {
  if (!stats_out || !n_out_dev ||
      (n_max > 0 && (!points || !points_out || !count_out || !voxel_of_out || (colors && !colors_out))))
    return DP_ERR_ARG;
  if (n_max < 0 || !(voxel_size > 0.0) || !(voxel_size < __builtin_inf())) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, n_max, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int g = grid_for(n_max, GRID_CAP);
  const int rc = sorted_cells(s, w, points, n_dev, n_max, voxel_size, voxel_size / 2.0);
  if (rc) return rc;
  const int nb = (int)scan_blocks_for(n_max);
  hipLaunchKernelGGL(vox_flag_kernel, dim3(g), dim3(256), 0, s, w.keys, n_dev, n_max, w.flag);
  if (nb) hipLaunchKernelGGL(scan_count_kernel, dim3(nb), dim3(256), 0, s, w.flag, n_dev, n_max, w.bc);
  hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(256), 0, s, w.bc, nb, (uint32_t*)n_out_dev);   // the same bits
  if (nb) {
    hipLaunchKernelGGL(vox_rank_kernel, dim3(nb), dim3(256), 0, s, w.keys, w.vals, w.flag, n_dev, n_max, w.bc, voxel_of_out,
                       w.head);
    hipLaunchKernelGGL(vox_reduce_kernel, dim3(grid_for(64 * (int64_t)n_max, GRID_CAP)), dim3(256), 0, s, points, colors, w.vals,
                       w.head, n_dev, n_max, n_out_dev, points_out, colors_out, count_out);
  }
  hipLaunchKernelGGL(vox_final_kernel, dim3(1), dim3(1), 0, s, w.h, n_out_dev, stats_out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_knn_search(const double* points, const int32_t* n_dev, int32_t n_max, double radius, int32_t max_nn,
                             int32_t* nbr_out, int32_t* nbr_count_out, double* stats_out, void* workspace,
                             int64_t workspace_bytes, dp_stream_t stream) {
  if (!stats_out || (n_max > 0 && (!points || !nbr_out || !nbr_count_out))) return DP_ERR_ARG;
  if (n_max < 0 || max_nn < 1 || max_nn > MAX_NN || !(radius > 0.0) || !(radius < __builtin_inf())) return DP_ERR_SHAPE;
  Ws w;
  if (!ws_carve(workspace, workspace_bytes, n_max, &w)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int rc = sorted_cells(s, w, points, n_dev, n_max, radius * EDGE_SLACK, 0.0);
  if (rc) return rc;
  hipLaunchKernelGGL(gather_points_kernel, dim3(grid_for(n_max, GRID_CAP)), dim3(256), 0, s, points, w.vals, n_dev, n_max, w.sp);
  hipLaunchKernelGGL(knn_kernel, dim3(grid_for(64 * (int64_t)n_max, GRID_CAP)), dim3(256), 0, s, w.keys, w.vals, w.sp, n_dev,
                     n_max, radius * radius, max_nn, w.h, nbr_out, nbr_count_out);
  hipLaunchKernelGGL(knn_final_kernel, dim3(1), dim3(1), 0, s, w.h, stats_out);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_estimate_normals(const double* points, const int32_t* n_dev, int32_t n_max, const int32_t* nbr,
                                   const int32_t* nbr_count, int32_t max_nn, const double* camera, int32_t orient,
                                   double* normals_out, double* stats_out, dp_stream_t stream) {
  if (!stats_out || !camera || (n_max > 0 && (!points || !nbr || !nbr_count || !normals_out))) return DP_ERR_ARG;
  if (n_max < 0 || max_nn < 1 || max_nn > MAX_NN) return DP_ERR_SHAPE;
  for (int a = 0; a < 3; ++a)
    if (!(__builtin_fabs(camera[a]) < __builtin_inf())) return DP_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  (void)hipMemsetAsync(stats_out, 0, 8 * sizeof(double), s);
  hipLaunchKernelGGL(normals_kernel, dim3(grid_for(n_max, GRID_CAP)), dim3(256), 0, s, points, n_dev, n_max, nbr, nbr_count,
                     max_nn, camera[0], camera[1], camera[2], orient, normals_out, stats_out);
  hipLaunchKernelGGL(normals_final_kernel, dim3(1), dim3(1), 0, s, stats_out);
  DP_CHECK_LAUNCH();
  return 0;
}
