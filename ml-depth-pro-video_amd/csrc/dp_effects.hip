// Depth-warped views: the parallax frames and the red-cyan anaglyph of the reference's
// OLD_SCRIPTS/depth_video_effect.py (3D_EFFECTS_README.md), on the GPU.  The rules are in
// include/dp_mi355x.h ("Depth-warped views") and restated in tests/effects_numpy.py.
//
// The sampler is OpenCV 4.x's published fixed-point rule for cv2.remap(INTER_LINEAR) on 8-bit pixels
// with float32 maps (coordinates rounded half-even to 1/32, 15-bit weights).  As for dp_resize_u8_cv
// no cv2 binary was available to run against, so parity with a cv2 binary is unpinned: the restatement
// is the specification.
//
// Layout: the image is walked as one flat list of H * W pixels, 4 consecutive pixels per thread, so that
// a thread's 12 output bytes of a view are 3 dwords; rows need not be aligned.  A view whose first byte
// (v * H * W * 3) is not dword-aligned, and the last group of an image whose pixel count is no multiple
// of 4, are stored bytewise.  The depth is read once per pixel, whatever the number of views.  The
// source taps of a pixel are two runs of 6 bytes (two neighbouring pixels on each of two rows), fetched
// as one 4-byte and one 2-byte load each; they lie within the amplitude of the pixel itself and are
// left to L2 and the infinity cache.
#include "dp_common.h"

#pragma clang fp contract(off)      // x + dx * (1 - dn): a fused multiply-add changes the bytes

namespace {

constexpr int MAX_DIM = 16384;
constexpr int64_t WS_BYTES = 256;   // min / max keys of the finite depths

struct Views {
  int32_t n;
  int32_t kind[DP_WARP_MAX_VIEWS];
  double a[DP_WARP_MAX_VIEWS];
  double b[DP_WARP_MAX_VIEWS];
};

__device__ __forceinline__ uint32_t order_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) {   // inverse of order_key; 0xffffffff / 0 -> NaN
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool finite_d(double v) {
  return ((uint32_t)(__double_as_longlong(v) >> 32) & 0x7ff00000u) != 0x7ff00000u;
}

__global__ void fx_init_kernel(uint32_t* __restrict__ mm, unsigned long long* __restrict__ bad, int n_bad) {
  if (threadIdx.x < 2) mm[threadIdx.x] = threadIdx.x == 0 ? 0xffffffffu : 0u;
  if ((int)threadIdx.x < n_bad) bad[threadIdx.x] = 0ull;
}

// min and max over the finite depths (dp_depth_to_image's scheme; there NaN alone is skipped)
__global__ void __launch_bounds__(256) fx_minmax_kernel(const float* __restrict__ d, long long n, uint32_t* __restrict__ mm) {
  __shared__ uint32_t red[2][4];
  uint32_t kmin = 0xffffffffu, kmax = 0u;
  const long long stride = (long long)gridDim.x * 256 * 4;
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += stride) {
    float v[4];
    if (i + 3 < n && ((uintptr_t)(d + i) & 15) == 0) {
      const float4 q = *(const float4*)(d + i);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      #pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = i + r < n ? d[i + r] : __builtin_nanf("");
    }
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (finite_f(v[r])) {
        const uint32_t k = order_key(v[r]);
        kmin = k < kmin ? k : kmin;
        kmax = k > kmax ? k : kmax;
      }
    }
  }
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t a = __shfl_xor(kmin, o), b = __shfl_xor(kmax, o);
    kmin = a < kmin ? a : kmin;
    kmax = b > kmax ? b : kmax;
  }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = kmin; red[1][threadIdx.x >> 6] = kmax; }
  __syncthreads();
  if (threadIdx.x == 0) {
    #pragma unroll
    for (int w = 1; w < 4; ++w) {
      kmin = red[0][w] < kmin ? red[0][w] : kmin;
      kmax = red[1][w] > kmax ? red[1][w] : kmax;
    }
    atomicMin(mm, kmin);
    atomicMax(mm + 1, kmax);
  }
}

// np.clip(m, 0, hi).astype(float32) * 32, rounded half-even: the 1/32 fixed-point coordinate (m finite)
__device__ __forceinline__ int fixed_coord(double m, double hi) {
  m = m < 0.0 ? 0.0 : m;
  m = m > hi ? hi : m;
  return (int)__builtin_rintf((float)m * 32.f);
}

// One source row's two taps at flat pixel `idx` (and the pixel after it), blended with fx / 32: per
// channel (32 - fx) * p0 + fx * p1.  The last pixel of the image has no pixel after it; fx is 0 there.
__device__ __forceinline__ void row_taps(const uint8_t* __restrict__ src, long long idx, long long n_px, int fx,
                                         int& r, int& g, int& b) {
  const uint8_t* p = src + 3 * idx;
  uint32_t lo;
  uint32_t hi = 0;
  if (idx + 1 < n_px) {
    uint16_t h;
    __builtin_memcpy(&lo, p, 4);
    __builtin_memcpy(&h, p + 4, 2);
    hi = h;
  } else {
    lo = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
  }
  const int w0 = 32 - fx;
  r = w0 * (int)(lo & 0xff) + fx * (int)(lo >> 24);
  g = w0 * (int)((lo >> 8) & 0xff) + fx * (int)(hi & 0xff);
  b = w0 * (int)((lo >> 16) & 0xff) + fx * (int)(hi >> 8);
}

// cv2.remap(INTER_LINEAR) of one pixel at the fixed-point coordinates (sx, sy): (sum + 512) >> 10 per channel
__device__ __forceinline__ uint32_t sample_px(const uint8_t* __restrict__ src, int H, int W, long long n_px, int sx, int sy) {
  const int ix = sx >> 5, fx = sx & 31, iy = sy >> 5, fy = sy & 31;
  int r0, g0, b0, r1 = 0, g1 = 0, b1 = 0;
  row_taps(src, (long long)iy * W + ix, n_px, fx, r0, g0, b0);
  if (fy) row_taps(src, (long long)(iy + 1 < H ? iy + 1 : iy) * W + ix, n_px, fx, r1, g1, b1);
  const int w0 = 32 - fy;
  const uint32_t r = (uint32_t)(w0 * r0 + fy * r1 + 512) >> 10;
  const uint32_t g = (uint32_t)(w0 * g0 + fy * g1 + 512) >> 10;
  const uint32_t b = (uint32_t)(w0 * b0 + fy * b1 + 512) >> 10;
  return r | (g << 8) | (b << 16);
}

// 4 pixels (r | g << 8 | b << 16 each) -> 12 bytes at o, pixels beyond `live` left alone
__device__ __forceinline__ void store_group(uint8_t* __restrict__ o, const uint32_t px[4], int live) {
  if (live == 4 && ((uintptr_t)o & 3) == 0) {
    uint32_t* q = (uint32_t*)o;
    q[0] = px[0] | (px[1] << 24);
    q[1] = (px[1] >> 8) | (px[2] << 16);
    q[2] = (px[2] >> 16) | (px[3] << 8);
  } else {
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < live) {
        o[3 * j] = (uint8_t)px[j];
        o[3 * j + 1] = (uint8_t)(px[j] >> 8);
        o[3 * j + 2] = (uint8_t)(px[j] >> 16);
      }
    }
  }
}

// the wave's sum of `cnt` added to *dst by one lane (bad pixels are rare: most waves skip this)
__device__ __forceinline__ void count_bad(unsigned long long* dst, int cnt) {
  if (__ballot(cnt != 0) == 0ull) return;
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((threadIdx.x & 63) == 0) atomicAdd(dst, (unsigned long long)cnt);
}

// 1f - dn of a thread's 4 pixels (float32 throughout, correctly rounded division); a pixel past the image gets 0
__device__ __forceinline__ void load_om(const float* __restrict__ depth, long long p0, int live, const uint32_t* __restrict__ mm,
                                        float om[4]) {
  const float mn = key_float(mm[0]), mx = key_float(mm[1]);
  const float range = mx - mn;
  float d[4];
  if (live == 4 && ((uintptr_t)(depth + p0) & 15) == 0) {
    const float4 q = *(const float4*)(depth + p0);
    d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
  } else {
    #pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = j < live ? depth[p0 + j] : mn;
  }
  #pragma unroll
  for (int j = 0; j < 4; ++j) om[j] = 1.f - __fdiv_rn(d[j] - mn, range);
}

template <bool USE_DEPTH>
__global__ void __launch_bounds__(256) warp_views_kernel(const uint8_t* __restrict__ src, const float* __restrict__ depth,
                                                         int H, int W, const Views vw, const uint32_t* __restrict__ mm,
                                                         uint8_t* __restrict__ out, unsigned long long* __restrict__ bad) {
  const long long n_px = (long long)H * W;
  const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  // no early return: count_bad is a wave operation
  const int live = p0 >= n_px ? 0 : (n_px - p0 < 4 ? (int)(n_px - p0) : 4);
  int xs[4], ys[4];
  {
    int y = (int)((p0 < n_px ? p0 : 0) / W), x = (int)((p0 < n_px ? p0 : 0) - (long long)y * W);
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      xs[j] = x; ys[j] = y;
      if (++x == W) { x = 0; ++y; }
    }
  }
  float om[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (USE_DEPTH) {
    if (live) load_om(depth, p0, live, mm, om);
  }
  const double xmax = (double)(W - 1), ymax = (double)(H - 1), cx = (double)W * 0.5, cy = (double)H * 0.5;
  for (int v = 0; v < vw.n; ++v) {
    const int kind = vw.kind[v];
    const double a = vw.a[v], b = vw.b[v];
    const float af = (float)a;
    uint32_t px[4];
    int cnt = 0;
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double x = (double)xs[j], y = (double)ys[j];
      double mx_, my_;
      if (kind == DP_WARP_ZOOM) {
        mx_ = x + a * (x - cx);
        my_ = y + a * (y - cy);
      } else if (kind == DP_WARP_SHIFT) {
        const double o = (double)om[j];
        mx_ = x + a * o;
        my_ = y + b * o;
      } else {                                   // DP_WARP_SHIFT_F32: the product in float32, no vertical shift
        mx_ = x + (double)(af * om[j]);
        my_ = y;
      }
      px[j] = 0u;
      if (j < live) {
        if (finite_d(mx_) && finite_d(my_)) px[j] = sample_px(src, H, W, n_px, fixed_coord(mx_, xmax), fixed_coord(my_, ymax));
        else ++cnt;
      }
    }
    if (live) store_group(out + ((long long)v * n_px + p0) * 3, px, live);
    count_bad(bad + v, cnt);
  }
}

__global__ void __launch_bounds__(256) anaglyph_kernel(const uint8_t* __restrict__ src, const float* __restrict__ depth, int H,
                                                       int W, float dx, const uint32_t* __restrict__ mm,
                                                       uint8_t* __restrict__ out, unsigned long long* __restrict__ bad) {
  const long long n_px = (long long)H * W;
  const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  const int live = p0 >= n_px ? 0 : (n_px - p0 < 4 ? (int)(n_px - p0) : 4);
  float om[4] = {0.f, 0.f, 0.f, 0.f};
  if (live) load_om(depth, p0, live, mm, om);
  const double xmax = (double)(W - 1);
  int y = (int)((p0 < n_px ? p0 : 0) / W), x = (int)((p0 < n_px ? p0 : 0) - (long long)y * W);
  uint32_t px[4];
  int cnt = 0;
  #pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double s = (double)(dx * om[j]);
    const double ml = (double)x + s, mr = (double)x - s;     // left view shifted right, right view shifted left
    px[j] = 0u;
    if (j < live) {
      if (finite_d(ml) && finite_d(mr)) {
        // map_y = y: one source row per view; channel 0 from the left view, 1 and 2 from the right
        const long long row = (long long)y * W;
        const int sl = fixed_coord(ml, xmax), sr = fixed_coord(mr, xmax);
        int r, g, b, t0, t1;
        row_taps(src, row + (sl >> 5), n_px, sl & 31, r, t0, t1);
        row_taps(src, row + (sr >> 5), n_px, sr & 31, t0, g, b);
        px[j] = ((uint32_t)(32 * r + 512) >> 10) | (((uint32_t)(32 * g + 512) >> 10) << 8) |
                (((uint32_t)(32 * b + 512) >> 10) << 16);
      } else {
        ++cnt;
      }
    }
    if (++x == W) { x = 0; ++y; }
  }
  if (live) store_group(out + p0 * 3, px, live);
  count_bad(bad, cnt);
}

inline bool dims_ok(int32_t H, int32_t W) { return H > 0 && W > 0 && H <= MAX_DIM && W <= MAX_DIM; }

inline void launch_minmax(const float* depth, long long n, uint32_t* mm, unsigned long long* bad, int n_bad, hipStream_t s) {
  hipLaunchKernelGGL(fx_init_kernel, dim3(1), dim3(64), 0, s, mm, bad, n_bad);
  if (n == 0) return;
  const int g = (int)(n / 1024 + 1 < 1024 ? n / 1024 + 1 : 1024);
  hipLaunchKernelGGL(fx_minmax_kernel, dim3(g), dim3(256), 0, s, depth, n, mm);
}
}  // namespace

extern "C" int64_t dp_effects_workspace_size(void) { return WS_BYTES; }

extern "C" int dp_warp_views(const uint8_t* image, const float* depth, int32_t H, int32_t W, const double* views,
                             int32_t n_views, uint8_t* out, int64_t* bad_out, void* workspace, int64_t workspace_bytes,
                             dp_stream_t stream) {
  if (!image || !depth || !views || !out || !bad_out || !workspace) return DP_ERR_ARG;
  if (!dims_ok(H, W) || n_views < 1 || n_views > DP_WARP_MAX_VIEWS) return DP_ERR_SHAPE;
  Views vw;
  vw.n = n_views;
  bool use_depth = false;
  for (int v = 0; v < DP_WARP_MAX_VIEWS; ++v) {
    const bool in = v < n_views;
    const double k = in ? views[3 * v] : (double)DP_WARP_ZOOM;
    if (!(k == DP_WARP_SHIFT || k == DP_WARP_SHIFT_F32 || k == DP_WARP_ZOOM)) return DP_ERR_ARG;
    vw.kind[v] = (int32_t)k;
    vw.a[v] = in ? views[3 * v + 1] : 0.0;
    vw.b[v] = in ? views[3 * v + 2] : 0.0;
    use_depth = use_depth || vw.kind[v] != DP_WARP_ZOOM;
  }
  if (workspace_bytes < WS_BYTES || ((uintptr_t)workspace & 3) || ((uintptr_t)bad_out & 7)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const long long n = (long long)H * W;
  uint32_t* mm = (uint32_t*)workspace;
  unsigned long long* bad = (unsigned long long*)bad_out;
  launch_minmax(depth, use_depth ? n : 0, mm, bad, n_views, s);
  const unsigned blocks = (unsigned)((n + 1023) / 1024);
  if (use_depth)
    hipLaunchKernelGGL(warp_views_kernel<true>, dim3(blocks), dim3(256), 0, s, image, depth, H, W, vw, mm, out, bad);
  else                                          // zoom alone never reads the depth
    hipLaunchKernelGGL(warp_views_kernel<false>, dim3(blocks), dim3(256), 0, s, image, depth, H, W, vw, mm, out, bad);
  DP_CHECK_LAUNCH();
  return 0;
}

extern "C" int dp_anaglyph(const uint8_t* image, const float* depth, int32_t H, int32_t W, double dx, uint8_t* out,
                           int64_t* bad_out, void* workspace, int64_t workspace_bytes, dp_stream_t stream) {
  if (!image || !depth || !out || !bad_out || !workspace) return DP_ERR_ARG;
  if (!dims_ok(H, W)) return DP_ERR_SHAPE;
  if (workspace_bytes < WS_BYTES || ((uintptr_t)workspace & 3) || ((uintptr_t)bad_out & 7)) return DP_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const long long n = (long long)H * W;
  uint32_t* mm = (uint32_t*)workspace;
  unsigned long long* bad = (unsigned long long*)bad_out;
  launch_minmax(depth, n, mm, bad, 1, s);
  hipLaunchKernelGGL(anaglyph_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, s, image, depth, H, W, (float)dx, mm,
                     out, bad);
  DP_CHECK_LAUNCH();
  return 0;
}
