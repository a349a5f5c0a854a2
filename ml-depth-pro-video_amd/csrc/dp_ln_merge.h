#pragma once
// dp_ln_merge.h -- folded LayerNorm: a row's statistics from its chunk statistics, shared by the
// consumer's pre-pass (ln_merge_kernel, dp_gemm.hip) and the split producer's last workgroup
// (ln_merge_last, dp_gemm_8ph320.hip) so that both compute the same bits.

#include "dp_common.h"

namespace {

// (rstd, -rstd * mean) of a row from its 8 chunk statistics (K = 1024; Chan's merge, as
// epilogue_mfma_lnc): ln_merge_kernel and ln_merge_last, the same arithmetic
__device__ __forceinline__ float2 ln_merge_row(const f32x4_t (&c)[4], float eps) {
  const float mean = (((c[0][0] + c[0][2]) + (c[1][0] + c[1][2])) + ((c[2][0] + c[2][2]) + (c[3][0] + c[3][2]))) *
                     (1.f / 8);
  float m2 = 0.f;
  #pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float d0 = c[i][0] - mean, d1 = c[i][2] - mean;
    m2 += (c[i][1] + 128.f * d0 * d0) + (c[i][3] + 128.f * d1 * d1);
  }
  const float rs = rsqrtf(m2 * (1.f / 1024) + eps);
  return make_float2(rs, -rs * mean);
}

}  // namespace
