// dp_gemm_splitk.hip: split-K for small grids (the 256 x 256 big engine over K ranges + a reduce launch).
//
// Launch 1: the 256 x 256 big engine over tiles x ksplit workgroups, each a K-step range of one
// tile, raw fp32 partials into the workspace ([ksplit][M][N]); launch 2 (this kernel): every
// thread sums the ksplit partials of 2 rows x 8 columns in split order (deterministic) and runs
// the same row epilogue the engines use (bias, activation, gamma, pos, residuals, store mode).
// No workgroup ever waits for another (unlike the stream-K hand-off), so a split-K launch can
// run beside any other launch.
#include "dp_gemm_big.h"

namespace {

template <typename K_>
__global__ void __launch_bounds__(256) splitk_reduce_kernel(const GemmP p) {
  const int cpr = p.N / 8;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long pairs = (p.M + 1) / 2;
  if (idx >= pairs * cpr) return;
  const int rp = (int)(idx / cpr), n = (int)(idx - (long long)rp * cpr) * 8;
  int ms[2] = {2 * rp, 2 * rp + 1};
  float v[2][8];
  #pragma unroll
  for (int it = 0; it < 2; ++it)
    #pragma unroll
    for (int r = 0; r < 8; ++r) v[it][r] = 0.f;
  const long long slab = (long long)p.M * p.N;
  const bool two = ms[1] < p.M;
  const float* base = p.kpart + (long long)ms[0] * p.N + n;
  #pragma unroll 4
  for (int sp = 0; sp < p.ksplit; ++sp) {
    const float* q = base + sp * slab;
    const float4 a0 = *(const float4*)q, a1 = *(const float4*)(q + 4);
    float4 b0 = make_float4(0.f, 0.f, 0.f, 0.f), b1 = b0;
    if (two) { b0 = *(const float4*)(q + p.N); b1 = *(const float4*)(q + p.N + 4); }
    v[0][0] += a0.x; v[0][1] += a0.y; v[0][2] += a0.z; v[0][3] += a0.w;
    v[0][4] += a1.x; v[0][5] += a1.y; v[0][6] += a1.z; v[0][7] += a1.w;
    v[1][0] += b0.x; v[1][1] += b0.y; v[1][2] += b0.z; v[1][3] += b0.w;
    v[1][4] += b1.x; v[1][5] += b1.y; v[1][6] += b1.z; v[1][7] += b1.w;
  }
  ColConst cc;
  load_colconst(p, n, cc);
  epilogue_rows<K_, 2>(p, cc, ms, n, v);
}

template <typename K_>
int launch_splitk(const GemmP& p0, bool conv, hipStream_t s) {
  GemmP p = p0;
  p.tiles_n = p.N / 256;
  p.tiles_m = (p.M + 255) / 256;
  if (p.ksplit < 2 || !p.kpart || p.N % 256 != 0) return DP_ERR_ARG;
  dim3 g1(p.tiles_n * p.tiles_m * p.ksplit);
#define DP_SPK(C_, R_) hipLaunchKernelGGL((gemm_big_kernel<K_, 256, 256, 64, 2, false, C_, R_, 8, -1, false, true>), g1, dim3(NT_BIG), 0, s, p)
  if (conv && p.relu_a) DP_SPK(true, true);
  else if (conv) DP_SPK(true, false);
  else if (p.relu_a) DP_SPK(false, true);
  else DP_SPK(false, false);
#undef DP_SPK
  DP_CHECK_LAUNCH();
  const long long threads = (long long)((p.M + 1) / 2) * (p.N / 8);
  hipLaunchKernelGGL(splitk_reduce_kernel<K_>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, p);
  DP_CHECK_LAUNCH();
  return 0;
}

}  // namespace

namespace dpg {
int launch_part_splitk(const GemmP& p, bool conv, bool bf16, hipStream_t s) {
  return (bf16 ? launch_splitk<KBF16>(p, conv, s) : launch_splitk<KF16>(p, conv, s));
}
}  // namespace dpg
