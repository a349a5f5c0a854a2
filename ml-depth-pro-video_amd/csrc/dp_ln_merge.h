#pragma once
// dp_ln_merge.h -- folded LayerNorm: a row's statistics from its chunk statistics, shared by the
// consumer's pre-pass (ln_merge_kernel, dp_gemm.hip) and the split producer's last workgroup
// (ln_merge_last, dp_gemm_8ph320.hip) so that both compute the same bits; the grouped 128 x 128
// launches' folded-LN epilogues (dp_gemm_big.h) use it too, and ln_chunk_merge for their producer.

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

// (mean, M2) of a 128-column chunk from the 4 waves' entries (shift, mean - shift, M2 over 32 columns
// each; epilogue_acc32_ln, the grouped 128 x 128 producer): Chan's merge of four equal counts on the
// means taken relative to the first entry's shift -- differences of nearby values, so a large common
// offset costs no digits -- and the offset added back at the end.
__device__ __forceinline__ float2 ln_chunk_merge(const f32x4_t (&e)[4]) {
  #pragma clang fp contract(off)
  float mu[4];
  #pragma unroll
  for (int w = 0; w < 4; ++w) mu[w] = (e[w][0] - e[0][0]) + e[w][1];
  const float mr = ((mu[0] + mu[1]) + (mu[2] + mu[3])) * 0.25f;
  float m2 = 0.f;
  #pragma unroll
  for (int w = 0; w < 4; ++w) {
    const float dl = mu[w] - mr;
    m2 += e[w][2] + 32.f * dl * dl;
  }
  return make_float2(e[0][0] + mr, m2);
}

}  // namespace
