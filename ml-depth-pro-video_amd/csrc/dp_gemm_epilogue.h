#pragma once
// dp_gemm_epilogue.h -- the dp_gemm epilogues that more than one engine uses.  Order of the
// operands everywhere: bias, activation, gamma, pos, R1, R2, (+C), store.
//   epilogue_rows   the general one (runtime operand set), 8 columns x NIT rows per lane: the
//                   big, 8-phase and stream-K engines and the split-K reduce
//   epilogue_mfma   load-free, in the MFMA register layout (16-bit C, no per-row operand): the
//                   big, 8-phase and 8-phase 320 x 256 engines
//   epilogue_acc32  fp32 C accumulated into, MFMA layout: the big engine
//   epilogue_acc32_ln  ... + the folded-LayerNorm producer outputs (grouped 128 x 128 launches)
//   head_ps_rows    the composed depth-head tail (DP_STORE_HEAD_PS): the big engine
// An engine's private epilogue lives beside its kernel.

#include "dp_gemm_impl.h"

namespace {

__device__ __forceinline__ void add8_f32(float (&v)[8], const float* p) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w;
  v[4] += b.x; v[5] += b.y; v[6] += b.z; v[7] += b.w;
}

// Row-staged epilogue for the big engines.  Per-column operands (bias, LayerScale
// gamma) are loaded once per lane -- a lane keeps the same 8 columns for the whole
// tile -- and each batch of NIT rows issues ALL of its row-dependent loads
// (residuals, the fp32 C being accumulated into) before any arithmetic or store, so
// their latencies overlap instead of serialising behind the stores.
struct ColConst {
  float b[8], g[8];
};
__device__ __forceinline__ void load_colconst(const GemmP& p, int n, ColConst& c) {
  const bool ok = n < p.N;
  if (p.bias && ok) {
    const float4 x = *(const float4*)(p.bias + n), y = *(const float4*)(p.bias + n + 4);
    c.b[0] = x.x; c.b[1] = x.y; c.b[2] = x.z; c.b[3] = x.w; c.b[4] = y.x; c.b[5] = y.y; c.b[6] = y.z; c.b[7] = y.w;
  } else {
    #pragma unroll
    for (int r = 0; r < 8; ++r) c.b[r] = 0.f;
  }
  if (p.gamma && ok) {
    const float4 x = *(const float4*)(p.gamma + n), y = *(const float4*)(p.gamma + n + 4);
    c.g[0] = x.x; c.g[1] = x.y; c.g[2] = x.z; c.g[3] = x.w; c.g[4] = y.x; c.g[5] = y.y; c.g[6] = y.z; c.g[7] = y.w;
  } else {
    #pragma unroll
    for (int r = 0; r < 8; ++r) c.g[r] = 1.f;
  }
}
__device__ __forceinline__ long long out_offset(const GemmP& p, int m, int n) {
  if (p.store_mode == DP_STORE_DECONV2X2) {
    const int hw = p.dc_h * p.dc_w;
    const int b = m / hw, rr = m - b * hw;
    const int y = rr / p.dc_w, x = rr - y * p.dc_w;
    const int q = n / p.dc_cout, co = n - q * p.dc_cout;
    const long long pix = ((long long)b * 2 * p.dc_h + 2 * y + (q >> 1)) * (2 * p.dc_w) + 2 * x + (q & 1);
    return pix * p.ldc + co;
  }
  long long row = m;
  if (p.row_group) row = (long long)(m / p.row_group) * p.row_group_out + p.row_off + m % p.row_group;
  return row * p.ldc + n;
}
template <typename K_>
__device__ __forceinline__ void add8_u4(float (&v)[8], uint4 r) {
  const uint32_t w[4] = {r.x, r.y, r.z, r.w};
  #pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[2 * k] += K_::to_f(w[k] & 0xffff);
    v[2 * k + 1] += K_::to_f(w[k] >> 16);
  }
}
// Composed 3x3-after-1x1 conv (DP_STORE_ROWS with head_corr, engine.compose_head0): the 1x1's
// bias rides in the composed bias for all 9 taps; at the image border the taps that fall in
// the 3x3's zero padding must not contribute it: subtract corr[(ky*3+kx)*N + n] for each.
__device__ __forceinline__ void border_correct(const GemmP& p, int m, int nc, float (&z)[8]) {
  const int hw = p.out_h * p.out_w;
  const int rr = m % hw;
  const int yy = rr / p.out_w, xx = rr - yy * p.out_w;
  const bool top = yy == 0, bot = yy == p.out_h - 1, lft = xx == 0, rgt = xx == p.out_w - 1;
  if (!(top || bot || lft || rgt)) return;
  // a rolled loop with two 16-B loads per tap: few live registers in an epilogue that is
  // already at the 256-VGPR limit (the unrolled 9 x 8 form cost 71 spills)
  #pragma unroll 1
  for (int t = 0; t < 9; ++t) {
    const int a = t / 3, c = t - 3 * (t / 3);
    const bool oob = (a == 0 && top) || (a == 2 && bot) || (c == 0 && lft) || (c == 2 && rgt);
    if (oob) {
      const float4 lo = *(const float4*)(p.head_corr + t * p.N + nc);
      const float4 hi = *(const float4*)(p.head_corr + t * p.N + nc + 4);
      z[0] -= lo.x; z[1] -= lo.y; z[2] -= lo.z; z[3] -= lo.w;
      z[4] -= hi.x; z[5] -= hi.y; z[6] -= hi.z; z[7] -= hi.w;
    }
  }
}
// v[it][0..7] = accumulators of row ms[it], columns n..n+7.  Loads go to clamped
// (always valid) rows with no predicate, so the compiler issues the whole batch
// back to back instead of sinking each load into its own branch; only the
// stores are predicated.
// BC: this instantiation applies the composed-conv border correction (only the 512 x 128 conv
// engine has it: compiled into every engine's epilogue it costs the 320 x 256 one ~170 spills)
template <typename K_, int NIT, bool BC = false>
__device__ __forceinline__ void epilogue_rows(const GemmP& p, const ColConst& cc, const int (&ms)[NIT], int n,
                                              float (&v)[NIT][8]) {
  const int nc = n < p.N ? n : p.N - 8;
  int mc[NIT];
  long long off[NIT];
  #pragma unroll
  for (int it = 0; it < NIT; ++it) {
    mc[it] = ms[it] < p.M ? ms[it] : p.M - 1;
    off[it] = out_offset(p, mc[it], nc);
  }
  uint4 r1[NIT], r2[NIT];
  float4 c0[NIT], c1[NIT];
  if (p.R1) {
    #pragma unroll
    for (int it = 0; it < NIT; ++it) r1[it] = *(const uint4*)(p.R1 + (long long)mc[it] * p.ldr1 + nc);
  }
  if (p.R2) {
    #pragma unroll
    for (int it = 0; it < NIT; ++it) r2[it] = *(const uint4*)(p.R2 + (long long)mc[it] * p.ldr2 + nc);
  }
  const bool acc32 = p.accumulate && p.c_dtype == DP_F32;
  if (acc32) {
    #pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const float* c = (const float*)p.C + off[it];
      c0[it] = *(const float4*)c;
      c1[it] = *(const float4*)(c + 4);
    }
  }
  #pragma unroll
  for (int it = 0; it < NIT; ++it) {
    float (&x)[8] = v[it];
    #pragma unroll
    for (int r = 0; r < 8; ++r) x[r] += cc.b[r];
    if constexpr (BC) {
      if (p.head_corr) border_correct(p, mc[it], nc, x);
    }
    if (p.act == DP_ACT_RELU) {
      #pragma unroll
      for (int r = 0; r < 8; ++r) x[r] = fmaxf(x[r], 0.f);
    } else if (p.act == DP_ACT_GELU) {
      #pragma unroll
      for (int r = 0; r < 8; ++r) x[r] = gelu_erf(x[r]);
    }
    if (p.gamma) {
      #pragma unroll
      for (int r = 0; r < 8; ++r) x[r] *= cc.g[r];
    }
    if (p.pos) add8_f32(x, p.pos + (long long)(mc[it] % p.pos_group + p.pos_off) * p.ldpos + nc);
    if (p.R1) add8_u4<K_>(x, r1[it]);
    if (p.R2) add8_u4<K_>(x, r2[it]);
    if (acc32) {
      x[0] += c0[it].x; x[1] += c0[it].y; x[2] += c0[it].z; x[3] += c0[it].w;
      x[4] += c1[it].x; x[5] += c1[it].y; x[6] += c1[it].z; x[7] += c1[it].w;
    }
  }
  const bool nok = n < p.N;
  #pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const float (&x)[8] = v[it];
    if (!(nok && ms[it] < p.M)) continue;
    if (p.c_dtype == DP_F32) {
      float* c = (float*)p.C + off[it];
      *(float4*)c = make_float4(x[0], x[1], x[2], x[3]);
      *(float4*)(c + 4) = make_float4(x[4], x[5], x[6], x[7]);
    } else {
      uint4 o;
      o.x = (uint32_t)K_::from_f(x[0]) | ((uint32_t)K_::from_f(x[1]) << 16);
      o.y = (uint32_t)K_::from_f(x[2]) | ((uint32_t)K_::from_f(x[3]) << 16);
      o.z = (uint32_t)K_::from_f(x[4]) | ((uint32_t)K_::from_f(x[5]) << 16);
      o.w = (uint32_t)K_::from_f(x[6]) | ((uint32_t)K_::from_f(x[7]) << 16);
      *(uint4*)((u16*)p.C + off[it]) = o;
    }
  }
}

// Load-free epilogue in the MFMA register layout (no per-row operands, 16-bit C): lane
// (t = lane & 15, g = lane >> 4) of accumulator fragment (fm, fn) holds token row fm * 16 + t,
// channels fn * 16 + 4 g .. + 3.  bias / ACT / gamma are applied right there, on all FM x FN x 4
// values of the lane at once (no per-row batches: the compiler interleaves 128 independent GELU
// chains), packed to 16 bits and staged through the wave's LDS slab as [rows][TN] 16-bit rows
// (16-B chunks XOR-swizzled by row), which are read back row-major and stored as whole row
// segments (TN * 2 bytes per row, 16 B per lane).  PF fragment rows per pass (slab: PF * 16 *
// TN * 2 bytes per wave).  LDS operations of one wave complete in order, so the write -> read
// -> next pass's write sequence needs no barrier (the slab is the wave's own).
// LNC: the consumer of a folded LayerNorm (grouped 128 x 128 launches, dp_gemm_args.ln_part_in): per
// value rstd * acc - rstd * mean * colsum[n] + bias[n], then ACT (no gamma) -- the arithmetic of the
// 8-phase 320 x 256 engine's epilogue_mfma_lnc; `rsm` = (rstd, -rstd * mean) of the wave's rows in
// LDS, merged once per workgroup by the kernel.
template <typename K_, int ACT, int FM, int FN, int TN, int PF, bool LNC = false>
__device__ __forceinline__ void epilogue_mfma(const GemmP& p, f32x4_t (&acc)[FM][FN], char* slab, int lane,
                                              int m_base, int n_base, const float2* rsm = nullptr) {
  constexpr int CH = TN / 8;            // 16-B chunks per staged row
  constexpr int RPI = 64 / CH;          // rows per read-back instruction
  static_assert(FM % PF == 0 && (CH == 16 || CH == 8 || CH == 4), "tile");
  const int t = lane & 15, g = lane >> 4;
  float bias[FN][4], gam[FN][4];        // (LNC: gam = the column sums of B)
  #pragma unroll
  for (int fn = 0; fn < FN; ++fn) {
    const int n = n_base + fn * 16 + 4 * g;
    const bool ok = n < p.N;
    const float4 b = (p.bias && ok) ? *(const float4*)(p.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 q;
    if constexpr (LNC) q = ok ? *(const float4*)(p.ln_colsum + n) : make_float4(0.f, 0.f, 0.f, 0.f);
    else q = (p.gamma && ok) ? *(const float4*)(p.gamma + n) : make_float4(1.f, 1.f, 1.f, 1.f);
    bias[fn][0] = b.x; bias[fn][1] = b.y; bias[fn][2] = b.z; bias[fn][3] = b.w;
    gam[fn][0] = q.x; gam[fn][1] = q.y; gam[fn][2] = q.z; gam[fn][3] = q.w;
  }
  #pragma unroll
  for (int f0 = 0; f0 < FM; f0 += PF) {
    #pragma unroll
    for (int fm = 0; fm < PF; ++fm)
      #pragma unroll
      for (int fn = 0; fn < FN; ++fn) {
        // packed-f32 arithmetic on the lane's 4 columns (gelu_erf4): same values as per element
        f32x4_t x;
        if constexpr (LNC) {
          const float2 rs = rsm[(f0 + fm) * 16 + t];
          x = __builtin_elementwise_fma(
              acc[f0 + fm][fn], (f32x4_t)(rs.x),
              __builtin_elementwise_fma(f32x4_t{gam[fn][0], gam[fn][1], gam[fn][2], gam[fn][3]}, (f32x4_t)(rs.y),
                                        f32x4_t{bias[fn][0], bias[fn][1], bias[fn][2], bias[fn][3]}));
        } else {
          x = acc[f0 + fm][fn] + f32x4_t{bias[fn][0], bias[fn][1], bias[fn][2], bias[fn][3]};
        }
        if constexpr (ACT == DP_ACT_RELU) {
          #pragma unroll
          for (int r = 0; r < 4; ++r) x[r] = fmaxf(x[r], 0.f);
        } else if constexpr (ACT == DP_ACT_GELU) {
          x = gelu_erf4(x);
        }
        if constexpr (!LNC) x = x * f32x4_t{gam[fn][0], gam[fn][1], gam[fn][2], gam[fn][3]};
        const int row = fm * 16 + t;
        const int chunk = fn * 2 + (g >> 1);
        uint2 w;
        w.x = K_::pack2(x[0], x[1]);
        w.y = K_::pack2(x[2], x[3]);
        *(uint2*)(slab + row * (TN * 2) + ((chunk ^ (row & (CH - 1))) << 4) + (g & 1) * 8) = w;
      }
    #pragma unroll
    for (int k = 0; k < PF * 16 / RPI; ++k) {
      const int row = k * RPI + lane / CH, chunk = lane % CH;
      const uint4 d = *(const uint4*)(slab + row * (TN * 2) + ((chunk ^ (row & (CH - 1))) << 4));
      const int m = m_base + f0 * 16 + row, n = n_base + chunk * 8;
      if (m < p.M && n < p.N) *(uint4*)((u16*)p.C + (long long)m * p.ldc + n) = d;
    }
  }
}

// Residual-accumulate epilogue in the MFMA register layout (fp32 C += (acc + bias) act * gamma,
// no other per-row operand: the ViT proj / fc2 with LayerScale, timm Block's x + ls(...)).  Each
// lane reads and writes its 4 consecutive fp32 columns of one row (16 B; a fragment pair covers a
// whole 128-B line of 16 rows), no LDS round trip, and the C loads of fragment row fm + 1 are in
// flight while row fm is computed and stored (straight-line code: the compiler counts the waits
// instead of draining every earlier store).  Same arithmetic, in the same order, as
// epilogue_rows -- no contraction of the gamma product into the residual add, which the general
// path's separate (runtime-conditional) steps do not get either: bit-identical results.
template <int ACT, int FM, int FN>
__device__ __forceinline__ void epilogue_acc32(const GemmP& p, f32x4_t (&acc)[FM][FN], int lane, int m_base,
                                               int n_base) {
  #pragma clang fp contract(off)
  const int t = lane & 15, g = lane >> 4;
  float bias[FN][4], gam[FN][4];
  #pragma unroll
  for (int fn = 0; fn < FN; ++fn) {
    const int n = n_base + fn * 16 + 4 * g;
    const bool ok = n < p.N;
    const float4 b = (p.bias && ok) ? *(const float4*)(p.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 q = (p.gamma && ok) ? *(const float4*)(p.gamma + n) : make_float4(1.f, 1.f, 1.f, 1.f);
    bias[fn][0] = b.x; bias[fn][1] = b.y; bias[fn][2] = b.z; bias[fn][3] = b.w;
    gam[fn][0] = q.x; gam[fn][1] = q.y; gam[fn][2] = q.z; gam[fn][3] = q.w;
  }
  float* const C = (float*)p.C;
  f32x4_t cur[FN], nxt[FN];
  auto load_row = [&](int fm, f32x4_t (&c)[FN]) __attribute__((always_inline)) {
    const int m = min(m_base + fm * 16 + t, p.M - 1);
    #pragma unroll
    for (int fn = 0; fn < FN; ++fn) c[fn] = *(const f32x4_t*)(C + (long long)m * p.ldc + n_base + fn * 16 + 4 * g);
  };
  load_row(0, cur);
  #pragma unroll
  for (int fm = 0; fm < FM; ++fm) {
    if (fm + 1 < FM) load_row(fm + 1, nxt);
    const int m = m_base + fm * 16 + t;
    #pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
      f32x4_t x;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[fm][fn][r] + bias[fn][r];
        if constexpr (ACT == DP_ACT_RELU) v = fmaxf(v, 0.f);
        else if constexpr (ACT == DP_ACT_GELU) v = gelu_erf(v);
        x[r] = v * gam[fn][r] + cur[fn][r];
      }
      if (m < p.M) *(f32x4_t*)(C + (long long)m * p.ldc + n_base + fn * 16 + 4 * g) = x;
    }
    #pragma unroll
    for (int fn = 0; fn < FN; ++fn) cur[fn] = nxt[fn];
  }
}

// epilogue_acc32 (ACT none) + the producer side of a folded LayerNorm, for the grouped 128 x 128
// launches (the side encoders' proj / fc2): besides C (fp32, accumulated, bit-identical to
// epilogue_acc32) every new row goes out in 16 bits (p.ln_xb_out, 8 B per lane) and leaves the
// statistics of the wave's TN = 32 columns in LDS, shifted as in the 320 x 256 producer (shift = the
// row's first value in the wave, so a large common offset cancels exactly) but in two passes over
// the lane's 8 registers: (shift, mean - shift, M2) at st[4 * wave row] (`st` = the wave's column of
// the workgroup's [tile row][wn] table).  The
// tile is one 128-column chunk wide, so the kernel merges a row's WN entries into its (mean, M2)
// after a barrier (ln_chunk_merge): no hand-off between workgroups.  Whole column tiles only.
template <typename K_, int FM, int FN>
__device__ __forceinline__ void epilogue_acc32_ln(const GemmP& p, f32x4_t (&acc)[FM][FN], f32x4_t* st, int lane,
                                                  int m_base, int n_base) {
  #pragma clang fp contract(off)
  const int t = lane & 15, g = lane >> 4;
  float bias[FN][4], gam[FN][4];
  #pragma unroll
  for (int fn = 0; fn < FN; ++fn) {
    const int n = n_base + fn * 16 + 4 * g;
    const float4 b = p.bias ? *(const float4*)(p.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 q = p.gamma ? *(const float4*)(p.gamma + n) : make_float4(1.f, 1.f, 1.f, 1.f);
    bias[fn][0] = b.x; bias[fn][1] = b.y; bias[fn][2] = b.z; bias[fn][3] = b.w;
    gam[fn][0] = q.x; gam[fn][1] = q.y; gam[fn][2] = q.z; gam[fn][3] = q.w;
  }
  float* const C = (float*)p.C;
  f32x4_t cur[FN], nxt[FN];
  auto load_row = [&](int fm, f32x4_t (&c)[FN]) __attribute__((always_inline)) {
    const int m = min(m_base + fm * 16 + t, p.M - 1);
    #pragma unroll
    for (int fn = 0; fn < FN; ++fn) c[fn] = *(const f32x4_t*)(C + (long long)m * p.ldc + n_base + fn * 16 + 4 * g);
  };
  load_row(0, cur);
  #pragma unroll
  for (int fm = 0; fm < FM; ++fm) {
    if (fm + 1 < FM) load_row(fm + 1, nxt);
    const int m = m_base + fm * 16 + t;
    f32x4_t x[FN];
    #pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = acc[fm][fn][r] + bias[fn][r];
        x[fn][r] = v * gam[fn][r] + cur[fn][r];
      }
      if (m < p.M) {
        *(f32x4_t*)(C + (long long)m * p.ldc + n_base + fn * 16 + 4 * g) = x[fn];
        uint2 w;
        w.x = K_::pack2(x[fn][0], x[fn][1]);
        w.y = K_::pack2(x[fn][2], x[fn][3]);
        *(uint2*)(p.ln_xb_out + (long long)m * p.ldc + n_base + fn * 16 + 4 * g) = w;
      }
    }
    const float sh = __shfl(x[0][0], t);    // the row's value at column n_base (lane t, g = 0)
    float d[FN][4], s1 = 0.f;
    #pragma unroll
    for (int fn = 0; fn < FN; ++fn)
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        d[fn][r] = x[fn][r] - sh;
        s1 += d[fn][r];
      }
    // the row's TN columns: 4 lanes (g)
    s1 += __shfl_xor(s1, 16);
    s1 += __shfl_xor(s1, 32);
    const float dm = s1 * (1.f / 32);
    float s2 = 0.f;
    #pragma unroll
    for (int fn = 0; fn < FN; ++fn)
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = d[fn][r] - dm;
        s2 += e * e;
      }
    s2 += __shfl_xor(s2, 16);
    s2 += __shfl_xor(s2, 32);
    if (g == 0) st[(fm * 16 + t) * 4] = f32x4_t{sh, dm, s2, 0.f};
    #pragma unroll
    for (int fn = 0; fn < FN; ++fn) cur[fn] = nxt[fn];
  }
}

// DP_STORE_HEAD_PS epilogue (depth head tail, depth_pro.py:182-207, composed at
// pack time): the GEMM ran the 3x3 conv of head.2 over the 2x-upsampled map as a
// 3x3 conv of the pre-upsampling map h0 whose N = 128 columns are (parity q =
// 2*dy + dx, channel o < 32).  Per output pixel (2y+dy, 2x+dx): z = acc + bias,
// minus the deconv-bias share of the taps that fall in head.2's zero padding
// (image border only), ReLU, dot with head.4's 32 weights, + bias, ReLU -> fp32.
// The 8 columns of a lane lie in one parity group; the 4 lanes of a row finish
// the 32-channel dot with two xor-shuffles.  Requires TN == 32 (one parity per wave).
template <int NIT>
__device__ __forceinline__ void head_ps_rows(const GemmP& p, const ColConst& cc, const int (&ms)[NIT], int n,
                                             float (&v)[NIT][8], int lane) {
  const int q = n >> 5, o0 = n & 31, dy = q >> 1, dx = q & 1;
  const int hw = p.out_h * p.out_w;
  float hw8[8];
  #pragma unroll
  for (int r = 0; r < 8; ++r) hw8[r] = p.head_w[o0 + r];
  #pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int m = ms[it] < p.M ? ms[it] : p.M - 1;
    const int b = m / hw, rr = m - b * hw;
    const int y = rr / p.out_w, x = rr - y * p.out_w;
    float z[8];
    #pragma unroll
    for (int r = 0; r < 8; ++r) z[r] = v[it][r] + cc.b[r];
    const bool top = y == 0 && dy == 0, bot = y == p.out_h - 1 && dy == 1;
    const bool lft = x == 0 && dx == 0, rgt = x == p.out_w - 1 && dx == 1;
    if (top || bot || lft || rgt) {
      #pragma unroll
      for (int a = 0; a < 3; ++a)
        #pragma unroll
        for (int c = 0; c < 3; ++c) {
          const bool oob = (a == 0 && top) || (a == 2 && bot) || (c == 0 && lft) || (c == 2 && rgt);
          if (oob) {
            #pragma unroll
            for (int r = 0; r < 8; ++r) z[r] -= p.head_corr[(a * 3 + c) * 32 + o0 + r];
          }
        }
    }
    float hs = 0.f;
    #pragma unroll
    for (int r = 0; r < 8; ++r) hs += fmaxf(z[r], 0.f) * hw8[r];
    hs += __shfl_xor(hs, 1);
    hs += __shfl_xor(hs, 2);
    if ((lane & 3) == 0 && ms[it] < p.M) {
      const long long W2 = 2LL * p.out_w;
      ((float*)p.C)[((long long)b * 2 * p.out_h + 2 * y + dy) * W2 + 2 * x + dx] = fmaxf(hs + p.head_b, 0.f);
    }
  }
}

}  // namespace
