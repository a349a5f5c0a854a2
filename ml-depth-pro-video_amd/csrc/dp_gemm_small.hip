// dp_gemm_small.hip: the register-staged small-tile engines and the 2-workgroup-per-CU 256 x 128 engine.
//
// "small" (BM x BN x 64, 256 threads, register-staged, 2 workgroups/CU): N <= 64 outputs
// (depth-head tail, FOV head) and the fused 1x1 head.  The same swizzled LDS rows and MFMA operand
// order as the big engines (dp_gemm_dev.h).  launch_dual runs the big engine's kernel
// (dp_gemm_big.h) with 4 waves per workgroup.
#include "dp_gemm_big.h"

namespace {

// ---------------------------------------------------------------- epilogue
// v[0..3] = accumulators of output (m, n..n+3).  Order: bias, act, gamma, pos,
// R1, R2, (+C), store; with head_w the values are folded into hsum instead.
template <typename K_>
__device__ __forceinline__ void epilogue4(const GemmP& p, int m, int n, float (&v)[4], float& hsum) {
  if (p.bias) {
    float4 b = *(const float4*)(p.bias + n);
    v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
  }
  if (p.act == DP_ACT_RELU) {
    #pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
  } else if (p.act == DP_ACT_GELU) {
    #pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = gelu_erf(v[r]);
  }
  if (p.gamma) {
    float4 g = *(const float4*)(p.gamma + n);
    v[0] *= g.x; v[1] *= g.y; v[2] *= g.z; v[3] *= g.w;
  }
  if (p.pos) {
    const float* pp = p.pos + (long long)(m % p.pos_group + p.pos_off) * p.ldpos + n;
    float4 q = *(const float4*)pp;
    v[0] += q.x; v[1] += q.y; v[2] += q.z; v[3] += q.w;
  }
  if (p.R1) {
    uint2 r = *(const uint2*)(p.R1 + (long long)m * p.ldr1 + n);
    v[0] += K_::to_f(r.x & 0xffff); v[1] += K_::to_f(r.x >> 16);
    v[2] += K_::to_f(r.y & 0xffff); v[3] += K_::to_f(r.y >> 16);
  }
  if (p.R2) {
    uint2 r = *(const uint2*)(p.R2 + (long long)m * p.ldr2 + n);
    v[0] += K_::to_f(r.x & 0xffff); v[1] += K_::to_f(r.x >> 16);
    v[2] += K_::to_f(r.y & 0xffff); v[3] += K_::to_f(r.y >> 16);
  }
  if (p.head_w) {
    float4 w = *(const float4*)(p.head_w + n);
    hsum += v[0] * w.x + v[1] * w.y + v[2] * w.z + v[3] * w.w;
    return;
  }
  long long off;
  if (p.store_mode == DP_STORE_DECONV2X2) {
    const int hw = p.dc_h * p.dc_w;
    const int b = m / hw, rr = m - b * hw;
    const int y = rr / p.dc_w, x = rr - y * p.dc_w;
    const int q = n / p.dc_cout, co = n - q * p.dc_cout;
    const long long pix = ((long long)b * 2 * p.dc_h + 2 * y + (q >> 1)) * (2 * p.dc_w) + 2 * x + (q & 1);
    off = pix * p.ldc + co;
  } else {
    long long row = m;
    if (p.row_group) row = (long long)(m / p.row_group) * p.row_group_out + p.row_off + m % p.row_group;
    off = row * p.ldc + n;
  }
  if (p.c_dtype == DP_F32) {
    float* c = (float*)p.C + off;
    if (p.accumulate) {
      float4 o = *(const float4*)c;
      v[0] += o.x; v[1] += o.y; v[2] += o.z; v[3] += o.w;
    }
    *(float4*)c = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    uint2 o;
    o.x = (uint32_t)K_::from_f(v[0]) | ((uint32_t)K_::from_f(v[1]) << 16);
    o.y = (uint32_t)K_::from_f(v[2]) | ((uint32_t)K_::from_f(v[3]) << 16);
    *(uint2*)((u16*)p.C + off) = o;
  }
}

// ========================================================== small-tile engine
constexpr int NT = 256;

template <typename K_, int BM, int BN, int WM, int WN, bool CONV>
__global__ void __launch_bounds__(NT, 2) gemm_kernel(const GemmP p) {
  constexpr int TM = BM / WM, TN = BN / WN;
  constexpr int FM = TM / 16, FN = TN / 16;
  constexpr int CA = BM * 8 / NT;  // 16-B chunks per thread per A tile
  constexpr int CB = BN * 8 / NT;
  static_assert(CA >= 1 && CB >= 1 && WM * WN == 4, "tile config");
  __shared__ __attribute__((aligned(16))) u16 smem[2][(BM + BN) * BK];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int tile_n = blockIdx.x % p.tiles_n;
  const int tile_m = blockIdx.x / p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int kc = tid & 7;      // 16-B chunk within a 64-wide K row
  const int rbase = tid >> 3;  // first row of this thread's chunks (step 32)

  const u16* a_ptr[CA];
  ConvRow a_cr[CA];
  #pragma unroll
  for (int i = 0; i < CA; ++i) {
    const int m = m0 + rbase + 32 * i;
    if constexpr (!CONV) a_ptr[i] = p.A + (long long)(m < p.M ? m : p.M - 1) * p.lda + kc * 8;
    else a_cr[i] = conv_row(p, m);
  }
  const u16* b_ptr[CB];
  #pragma unroll
  for (int i = 0; i < CB; ++i) {
    int n = n0 + rbase + 32 * i;
    n = n < p.N ? n : p.N - 1;
    b_ptr[i] = p.B + (long long)n * p.ldb + kc * 8;
  }

  uint4 ra[CA], rb[CB];

  auto load_tile = [&](int k0) {
    if constexpr (!CONV) {
      #pragma unroll
      for (int i = 0; i < CA; ++i) ra[i] = *(const uint4*)(a_ptr[i] + k0);
    } else {
      int t_ky, t_kx, t_ci;
      conv_tap(p, k0, t_ky, t_kx, t_ci);
      #pragma unroll
      for (int i = 0; i < CA; ++i) {
        bool inb;
        const u16* s = conv_src(p, a_cr[i], t_ky, t_kx, t_ci + kc * 8, inb);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (inb) v = *(const uint4*)s;
        ra[i] = v;
      }
    }
    #pragma unroll
    for (int i = 0; i < CB; ++i) rb[i] = *(const uint4*)(b_ptr[i] + k0);
  };
  auto store_tile = [&](int buf) {
    u16* sa = smem[buf];
    u16* sb = smem[buf] + BM * BK;
    #pragma unroll
    for (int i = 0; i < CA; ++i) {
      uint4 v = ra[i];
      if (p.relu_a) v = relu_pk16(v);
      *(uint4*)(sa + lds_off(rbase + 32 * i, kc)) = v;
    }
    #pragma unroll
    for (int i = 0; i < CB; ++i) *(uint4*)(sb + lds_off(rbase + 32 * i, kc)) = rb[i];
  };

  f32x4_t acc[FM][FN];
  #pragma unroll
  for (int i = 0; i < FM; ++i)
    #pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int KT = p.K / BK;
  load_tile(0);
  store_tile(0);
  __syncthreads();

  const int frow = lane & 15;
  const int fchunk = lane >> 4;
  for (int kt = 0; kt < KT; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < KT) load_tile((kt + 1) * BK);
    const u16* sa = smem[cur];
    const u16* sb = smem[cur] + BM * BK;
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      uint4 af[FM], bf[FN];
      #pragma unroll
      for (int i = 0; i < FM; ++i)
        af[i] = *(const uint4*)(sa + lds_off(wm * TM + i * 16 + frow, ks * 4 + fchunk));
      #pragma unroll
      for (int j = 0; j < FN; ++j)
        bf[j] = *(const uint4*)(sb + lds_off(wn * TN + j * 16 + frow, ks * 4 + fchunk));
      #pragma unroll
      for (int i = 0; i < FM; ++i)
        #pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = K_::mfma16(bf[j], af[i], acc[i][j]);
    }
    if (kt + 1 < KT) store_tile(cur ^ 1);
    __syncthreads();
  }

  // epilogue: lane holds rows m = .. + (lane & 15), cols n = .. + 4*(lane >> 4) + r
  const int em = lane & 15;
  const int en = 4 * (lane >> 4);
  float hsum[FM];
  #pragma unroll
  for (int i = 0; i < FM; ++i) hsum[i] = 0.f;
  #pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int m = m0 + wm * TM + i * 16 + em;
    #pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n = n0 + wn * TN + j * 16 + en;
      if (m >= p.M || n >= p.N) continue;
      float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
      epilogue4<K_>(p, m, n, v, hsum[i]);
    }
  }
  if (p.head_w) {
    // a row's channels live in lanes (lane&15) + 16*{0..3} of the wave (WN == 1)
    #pragma unroll
    for (int i = 0; i < FM; ++i) {
      float s = hsum[i];
      s += __shfl_xor(s, 16);
      s += __shfl_xor(s, 32);
      const int m = m0 + wm * TM + i * 16 + em;
      if ((lane >> 4) == 0 && m < p.M) ((float*)p.C)[m] = fmaxf(s + p.head_b, 0.f);
    }
  }
}

template <typename K_, int BM, int BN, int WM, int WN>
int launch_small(const GemmP& p0, bool conv, hipStream_t s) {
  GemmP p = p0;
  p.tiles_n = (p.N + BN - 1) / BN;
  const int tiles_m = (p.M + BM - 1) / BM;
  dim3 grid(p.tiles_n * tiles_m);
  if (conv)
    hipLaunchKernelGGL((gemm_kernel<K_, BM, BN, WM, WN, true>), grid, dim3(NT), 0, s, p);
  else
    hipLaunchKernelGGL((gemm_kernel<K_, BM, BN, WM, WN, false>), grid, dim3(NT), 0, s, p);
  DP_CHECK_LAUNCH();
  return 0;
}

// two 4-wave workgroups per CU (tile 256 x 128, BK 32, 3-stage ring)
template <typename K_>
int launch_dual(const GemmP& p0, bool conv, hipStream_t s) {
  GemmP p = p0;
  p.tiles_n = (p.N + 127) / 128;
  p.tiles_m = (p.M + 255) / 256;
  dim3 grid(p.tiles_n * p.tiles_m);
  if (conv && p.relu_a)
    hipLaunchKernelGGL((gemm_big_kernel<K_, 256, 128, 32, 3, false, true, true, 4>), grid, dim3(256), 0, s, p);
  else if (conv)
    hipLaunchKernelGGL((gemm_big_kernel<K_, 256, 128, 32, 3, false, true, false, 4>), grid, dim3(256), 0, s, p);
  else {
    int ea = fast_epi_act(p);
    if (ea >= EPI_ACC && p.N % 128 != 0) ea = -1;   // (epilogue_acc32: whole column tiles only)
    if (p.relu_a)
      hipLaunchKernelGGL((gemm_big_kernel<K_, 256, 128, 32, 3, false, false, true, 4>), grid, dim3(256), 0, s, p);
    else if (ea == DP_ACT_NONE)
      hipLaunchKernelGGL((gemm_big_kernel<K_, 256, 128, 32, 3, false, false, false, 4, DP_ACT_NONE>), grid, dim3(256), 0, s, p);
    else if (ea == DP_ACT_GELU)
      hipLaunchKernelGGL((gemm_big_kernel<K_, 256, 128, 32, 3, false, false, false, 4, DP_ACT_GELU>), grid, dim3(256), 0, s, p);
    else if (ea == EPI_ACC)
      hipLaunchKernelGGL((gemm_big_kernel<K_, 256, 128, 32, 3, false, false, false, 4, EPI_ACC>), grid, dim3(256), 0, s, p);
    else
      hipLaunchKernelGGL((gemm_big_kernel<K_, 256, 128, 32, 3, false, false, false, 4>), grid, dim3(256), 0, s, p);
  }
  DP_CHECK_LAUNCH();
  return 0;
}

}  // namespace

namespace dpg {
int launch_part_small(const GemmP& p, int tile, bool conv, bool bf16, hipStream_t s) {
  switch (tile) {
    case DP_TILE_256x64: return (bf16 ? launch_small<KBF16, 256, 64, 4, 1>(p, conv, s) : launch_small<KF16, 256, 64, 4, 1>(p, conv, s));
    case DP_TILE_256x32: return (bf16 ? launch_small<KBF16, 256, 32, 4, 1>(p, conv, s) : launch_small<KF16, 256, 32, 4, 1>(p, conv, s));
    case DP_TILE_DUAL_256x128: return (bf16 ? launch_dual<KBF16>(p, conv, s) : launch_dual<KF16>(p, conv, s));
    default: return (bf16 ? launch_small<KBF16, 128, 128, 2, 2>(p, conv, s) : launch_small<KF16, 128, 128, 2, 2>(p, conv, s));
  }
}
}  // namespace dpg
