// dp_gemm_8ph320.hip: the 8-phase 320 x 256 engine.
//
// The 8-phase schedule (gemm_8ph_kernel) on the 320 x 256 tile that gives the ViT's M = 20195
// exactly 64 row tiles (proj / fc2: ONE round of 256 workgroups; qkv: 3).  8 waves as 4 (M) x
// 2 (N), wave tile 80 x 128 (acc 5 x 8 fragments = 160 VGPRs).  A K step (BK 64) is 4 phases,
// one per 32-column quarter of the wave's 128 columns: {ds_reads, LDS-DMA pieces, counted
// vmcnt, s_barrier, 20 MFMAs at raised priority, s_barrier}; phase 0 also reads the wave's 10
// A fragments (kept for the step).  The two wave groups (waves 0-3 / 4-7: one of each per
// SIMD) run staggered by one barrier, so one wave of a SIMD issues MFMAs while the other reads.
// LDS: 2 K-tile buffers of A (320 x 128 B) + B (256 x 128 B) = 144 KiB.
// Streaming, per step s (9 pieces of 1 KiB per wave): B quarter q of step s+1 in phase q (its
// buffer's quarter was last read 4 phases earlier), A of step s+2 in phases 2 / 3 (3 + 2
// pieces; the buffer's A was read in phase 0, two barriers back).  Every phase waits (counted)
// for what the NEXT phase reads -- B quarter q+1 of this step, or A and B quarter 0 of step
// s+1 in phase 3 -- so each piece has 4+ phases to land and the count is 8 in steady state.
// Dense A only; epilogues: the load-free MFMA-layout one (EACT = DP_ACT_*; 16-bit C) or the
// fp32 residual-accumulate one (EACT = EPI_ACC + act).
// (Measured and rejected, round 5: the K loop's first steps also streaming the wave's epilogue rows
// of the residual into a dummy LDS slot, so the epilogue's reads would hit the caches: proj 71.1 ->
// 76.9 us cold, fc2 155.9 -> 162.5, in-frame -0.8 fps, profiles/r05av_residual_touch/.)
#include "dp_gemm_dev.h"
#include "dp_gemm_epilogue.h"
#include "dp_ln_merge.h"

namespace {

// epilogue_acc32_wide + the producer side of a folded LayerNorm: besides C (fp32, accumulated),
// the new rows go out in 16 bits (p.ln_xb_out, staged through the wave's LDS region so each row
// leaves as one 256-B segment) and, per row, (mean, M2) of the wave's 128 columns
// (p.ln_part_out[m][n_base / 128]) -- shifted single-pass sums (shift = the row's first value,
// so no cancellation) reduced over the row's 4 lanes.  C is bit-identical to epilogue_acc32_wide.
// `slab`: the wave's LDS region, >= 5 KiB.
template <typename K_, int FM, int FN>
__device__ __forceinline__ void epilogue_acc32_wide_ln(const GemmP& p, f32x4_t (&acc)[FM][FN], char* slab, int lane,
                                                       int m_base, int n_base) {
  #pragma clang fp contract(off)
  static_assert(FN == 8, "wide epilogue");
  constexpr int H = FN / 2;
  const int t = lane & 15, g = lane >> 4;
  {
    const int c = 4 * (lane & 31), n = n_base + c;
    f32x4_t v;
    if (lane < 32) v = (p.bias && n < p.N) ? *(const f32x4_t*)(p.bias + n) : f32x4_t{0.f, 0.f, 0.f, 0.f};
    else v = (p.gamma && n < p.N) ? *(const f32x4_t*)(p.gamma + n) : f32x4_t{1.f, 1.f, 1.f, 1.f};
    *(f32x4_t*)(slab + (lane < 32 ? 0 : 512) + c * 4) = v;
  }
  char* const xst = slab + 1024;          // 16 rows x 128 columns x 16 bit, chunk ^ row swizzle
  float* const C = (float*)p.C;
  const int nch = p.N / 128;
  f32x4_t cur[H], nxt[H];
  auto load = [&](int ch, f32x4_t (&c)[H]) __attribute__((always_inline)) {
    const int fm = ch >> 1, h = ch & 1;
    const int m = min(m_base + fm * 16 + t, p.M - 1);
    #pragma unroll
    for (int f = 0; f < H; ++f)
      c[f] = *(const f32x4_t*)(C + (long long)m * p.ldc + n_base + (h * H + f) * 16 + 4 * g);
  };
  load(0, cur);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  float sh = 0.f, s1 = 0.f, s2 = 0.f;
  #pragma unroll
  for (int ch = 0; ch < 2 * FM; ++ch) {
    if (ch + 1 < 2 * FM) load(ch + 1, nxt);
    const int fm = ch >> 1, h = ch & 1;
    const int m = m_base + fm * 16 + t;
    #pragma unroll
    for (int f = 0; f < H; ++f) {
      const int fn = h * H + f;
      const f32x4_t b = *(const f32x4_t*)(slab + (fn * 16 + 4 * g) * 4);
      const f32x4_t q = *(const f32x4_t*)(slab + 512 + (fn * 16 + 4 * g) * 4);
      f32x4_t x;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[fm][fn][r] + b[r];
        x[r] = v * q[r] + cur[f][r];
      }
      if (m < p.M) *(f32x4_t*)(C + (long long)m * p.ldc + n_base + fn * 16 + 4 * g) = x;
      if (h == 0 && f == 0) {
        sh = __shfl(x[0], t);             // the row's value at column n_base (lane t, g = 0)
        s1 = 0.f;
        s2 = 0.f;
      }
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d = x[r] - sh;
        s1 += d;
        s2 += d * d;
      }
      uint2 w;
      w.x = K_::pack2(x[0], x[1]);
      w.y = K_::pack2(x[2], x[3]);
      *(uint2*)(xst + t * 256 + (((fn * 2 + (g >> 1)) ^ t) << 4) + (g & 1) * 8) = w;
    }
    #pragma unroll
    for (int f = 0; f < H; ++f) cur[f] = nxt[f];
    if (h == 1) {
      // the row's 128 columns: 4 lanes (g) of 32 values each
      s1 += __shfl_xor(s1, 16);
      s2 += __shfl_xor(s2, 16);
      s1 += __shfl_xor(s1, 32);
      s2 += __shfl_xor(s2, 32);
      if (g == 0 && m < p.M) {
        const float mc = sh + s1 * (1.f / 128);
        const float m2 = s2 - s1 * (s1 * (1.f / 128));
        *(float2*)(p.ln_part_out + ((long long)m * nch + n_base / 128) * 2) = make_float2(mc, m2);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's staging writes
      #pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int row = k * 4 + (lane >> 4), chunk = lane & 15;
        const uint4 d = *(const uint4*)(xst + row * 256 + ((chunk ^ row) << 4));
        const int mm = m_base + fm * 16 + row;
        if (mm < p.M) *(uint4*)(p.ln_xb_out + (long long)mm * p.ldc + n_base + chunk * 8) = d;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // read back before the next row's writes
    }
  }
}

// epilogue_mfma for the consumer of a folded LayerNorm (the ViT qkv / fc1 over un-normalised
// 16-bit rows, dp_gemm_args.ln_part_in): per value v = rstd * acc - rstd * mean * colsum[n] +
// bias[n], then ACT, packed to 16 bits and stored as epilogue_mfma does (PF = 1).  The wave's
// bias / colsum live in its LDS region (first KiB; staging after it), and each fragment row's
// 8 chunk statistics are loaded one row ahead and merged (Chan) -- no per-column or per-row
// register arrays beside the 160 accumulators.  `slab` >= 1 KiB + 16 * TN * 2 bytes.
template <typename K_, int ACT, int FM, int FN, int TN>
__device__ __forceinline__ void epilogue_mfma_lnc(const GemmP& p, f32x4_t (&acc)[FM][FN], char* slab, int lane,
                                                  int m_base, int n_base) {
  constexpr int CH = TN / 8, RPI = 64 / CH;
  static_assert(TN == 128 && FN == 8, "wide consumer epilogue");
  const int t = lane & 15, g = lane >> 4;
  {
    // lanes 0-31: bias of columns 4 lane .. +3; lanes 32-63: colsum
    const int c = 4 * (lane & 31), n = n_base + c;
    f32x4_t v;
    if (lane < 32) v = (p.bias && n < p.N) ? *(const f32x4_t*)(p.bias + n) : f32x4_t{0.f, 0.f, 0.f, 0.f};
    else v = n < p.N ? *(const f32x4_t*)(p.ln_colsum + n) : f32x4_t{0.f, 0.f, 0.f, 0.f};
    *(f32x4_t*)(slab + (lane < 32 ? 0 : 512) + c * 4) = v;
  }
  char* const stg = slab + 1024;
  f32x4_t cur[4], nxt[4];
  auto load = [&](int fm, f32x4_t (&c)[4]) __attribute__((always_inline)) {
    const int m = min(m_base + fm * 16 + t, p.M - 1);
    const f32x4_t* pp = (const f32x4_t*)(p.ln_part_in + (long long)m * 16);
    #pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = pp[i];
  };
  load(0, cur);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the constants, before any read of them
  #pragma unroll
  for (int fm = 0; fm < FM; ++fm) {
    if (fm + 1 < FM) load(fm + 1, nxt);
    // the row's mean / rstd from its 8 chunks of 128 columns
    const float mean = (((cur[0][0] + cur[0][2]) + (cur[1][0] + cur[1][2])) +
                        ((cur[2][0] + cur[2][2]) + (cur[3][0] + cur[3][2]))) * (1.f / 8);
    float m2 = 0.f;
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float d0 = cur[i][0] - mean, d1 = cur[i][2] - mean;
      m2 += (cur[i][1] + 128.f * d0 * d0) + (cur[i][3] + 128.f * d1 * d1);
    }
    const float rs = rsqrtf(m2 * (1.f / 1024) + p.ln_eps), nm = -rs * mean;
    #pragma unroll
    for (int fn = 0; fn < FN; ++fn) {
      const f32x4_t b = *(const f32x4_t*)(slab + (fn * 16 + 4 * g) * 4);
      const f32x4_t q = *(const f32x4_t*)(slab + 512 + (fn * 16 + 4 * g) * 4);
      f32x4_t x = __builtin_elementwise_fma(acc[fm][fn], (f32x4_t)(rs), __builtin_elementwise_fma(q, (f32x4_t)(nm), b));
      if constexpr (ACT == DP_ACT_RELU) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) x[r] = fmaxf(x[r], 0.f);
      } else if constexpr (ACT == DP_ACT_GELU) {
        x = gelu_erf4(x);
      }
      const int row = t;
      const int chunk = fn * 2 + (g >> 1);
      uint2 w;
      w.x = K_::pack2(x[0], x[1]);
      w.y = K_::pack2(x[2], x[3]);
      *(uint2*)(stg + row * (TN * 2) + ((chunk ^ (row & (CH - 1))) << 4) + (g & 1) * 8) = w;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    #pragma unroll
    for (int k = 0; k < 16 / RPI; ++k) {
      const int row = k * RPI + lane / CH, chunk = lane % CH;
      const uint4 d = *(const uint4*)(stg + row * (TN * 2) + ((chunk ^ (row & (CH - 1))) << 4));
      const int m = m_base + fm * 16 + row, n = n_base + chunk * 8;
      if (m < p.M && n < p.N) *(uint4*)((u16*)p.C + (long long)m * p.ldc + n) = d;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    #pragma unroll
    for (int i = 0; i < 4; ++i) cur[i] = nxt[i];
  }
}

// epilogue_acc32 for wide wave tiles (FN = 8: the 8-phase 320 x 256 engine), where 8 columns'
// bias / gamma and two rows of C in flight would not fit beside the 160 accumulators: the
// wave's bias / gamma go through its LDS slab (ds_read per half row), and C is read and
// written in half rows (4 fragments = 64 columns), the next half row's loads in flight while
// one is computed.  Same arithmetic in the same order as epilogue_acc32: bit-identical.
template <int ACT, int FM, int FN>
__device__ __forceinline__ void epilogue_acc32_wide(const GemmP& p, f32x4_t (&acc)[FM][FN], char* slab, int lane,
                                                    int m_base, int n_base) {
  #pragma clang fp contract(off)
  static_assert(FN == 8, "wide epilogue");
  constexpr int H = FN / 2;
  const int t = lane & 15, g = lane >> 4;
  {
    // lanes 0-31: bias of columns 4 lane .. +3; lanes 32-63: gamma (1 and 0 when absent)
    const int c = 4 * (lane & 31), n = n_base + c;
    f32x4_t v;
    if (lane < 32) v = (p.bias && n < p.N) ? *(const f32x4_t*)(p.bias + n) : f32x4_t{0.f, 0.f, 0.f, 0.f};
    else v = (p.gamma && n < p.N) ? *(const f32x4_t*)(p.gamma + n) : f32x4_t{1.f, 1.f, 1.f, 1.f};
    *(f32x4_t*)(slab + (lane < 32 ? 0 : 512) + c * 4) = v;
  }
  float* const C = (float*)p.C;
  f32x4_t cur[H], nxt[H];
  auto load = [&](int ch, f32x4_t (&c)[H]) __attribute__((always_inline)) {
    const int fm = ch >> 1, h = ch & 1;
    const int m = min(m_base + fm * 16 + t, p.M - 1);
    #pragma unroll
    for (int f = 0; f < H; ++f)
      c[f] = *(const f32x4_t*)(C + (long long)m * p.ldc + n_base + (h * H + f) * 16 + 4 * g);
  };
  load(0, cur);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the slab writes, before any read of them
  #pragma unroll
  for (int ch = 0; ch < 2 * FM; ++ch) {
    if (ch + 1 < 2 * FM) load(ch + 1, nxt);
    const int fm = ch >> 1, h = ch & 1;
    const int m = m_base + fm * 16 + t;
    #pragma unroll
    for (int f = 0; f < H; ++f) {
      const int fn = h * H + f;
      const f32x4_t b = *(const f32x4_t*)(slab + (fn * 16 + 4 * g) * 4);
      const f32x4_t q = *(const f32x4_t*)(slab + 512 + (fn * 16 + 4 * g) * 4);
      f32x4_t x;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[fm][fn][r] + b[r];
        if constexpr (ACT == DP_ACT_RELU) v = fmaxf(v, 0.f);
        else if constexpr (ACT == DP_ACT_GELU) v = gelu_erf(v);
        x[r] = v * q[r] + cur[f][r];
      }
      if (m < p.M) *(f32x4_t*)(C + (long long)m * p.ldc + n_base + fn * 16 + 4 * g) = x;
    }
    #pragma unroll
    for (int f = 0; f < H; ++f) cur[f] = nxt[f];
  }
}

// Folded-LN producer on a SPLIT residual stream (dp_gemm_args.ln_xl, LNM = 3 of the 8-phase
// 320 x 256 engine): the ViT residual x is held as hi (16 bits, = ln_xb_out, the next GEMM's A
// operand anyway) and an 8-bit low part (ln_xl: x - hi in steps of ulp(hi) / 256, lo8_encode):
// about 16 significant bits against fp32's 24 -- the patch encoder's rel-L1 vs the fp32 reference
// 2.3809e-3 against 2.3788e-3 with an fp32 stream (a 16-bit low part 2.3789e-3, bf16 hi alone
// 1.06e-2; tools/hilo_emul.py).  Per element: x' = (acc + b) * gamma + (hi + lo) (the fp32
// epilogue's operation order), hi' = r16(x'), lo' = lo8(x', hi'); (mean, M2) of each row's 128
// columns as epilogue_acc32_wide_ln (when ln_part_out); C (fp32) = x' when given (never read).
// 6 B of HBM per element instead of 10 (fp32 read + write, 16-bit hi write): the epilogue of a
// one-round launch (proj / fc2) is HBM-bound (10 -> 8 B with a 16-bit low part: proj 85 -> 75,
// fc2 172 -> 161 us, profiles/r05a_split_residual).
// The wave's 80 x 128 outputs go in NI = 10 chunks of 16 rows x 64 columns (fragment row fm,
// column half h), whose hi rows (2 KiB) and lo rows (1 KiB) arrive by LDS-DMA AHEAD chunks ahead
// into a 4-deep per-wave ring (the 16-B chunks XOR-swizzled by row on the source address: the
// MFMA-layout reads are conflict-free), are read in the MFMA layout, updated in place, read back as
// rows and leave as 128-B (hi) / 64-B (lo) row segments.  Every store is a buffer store whose masked
// lanes (rows past M, an absent output) carry an out-of-range offset, so each chunk issues a fixed
// number of VMEM instructions and the counted wait for a chunk's DMA is a compile-time constant.
// AHEAD = 3 and 1 measured the same in the frame (profiles/r05b_epilogue_dma_depth; 1 = debug 1 << 27).
// `slab`: the wave's LDS region, >= 13 KiB.
template <typename K_, int FM, int FN, int AHEAD = 3>
__device__ __forceinline__ void epilogue_hilo_ln(const GemmP& p, f32x4_t (&acc)[FM][FN], char* slab, int lane,
                                                 int m_base, int n_base) {
  #pragma clang fp contract(off)
  static_assert(FN == 8 && AHEAD >= 1 && AHEAD <= 3, "128 columns per wave, <= 4 ring slots");
  constexpr int NI = 2 * FM, CB = 3072, LO = 2048;   // chunks, ring slot bytes (hi | lo), lo offset
  constexpr int PCS = 3;                              // DMA pieces per chunk: hi 2, lo 1
  // the counted wait for chunk i's DMA: younger are the DMAs of chunks i+1 .. i+AHEAD and the
  // stores of the chunks processed since chunk i's DMA was issued (C 4, part (second half), hi 2, lo 1)
  constexpr auto younger = [](int i) constexpr {
    int n = PCS * ((i + AHEAD < NI - 1 ? i + AHEAD : NI - 1) - i);
    for (int j = (i - AHEAD > 0 ? i - AHEAD : 0); j < i; ++j) n += 4 + (j & 1) + 3;
    return n;
  };
  const int t = lane & 15, g = lane >> 4;
  {
    const int c = 4 * (lane & 31), n = n_base + c;
    f32x4_t v;
    if (lane < 32) v = (p.bias && n < p.N) ? *(const f32x4_t*)(p.bias + n) : f32x4_t{0.f, 0.f, 0.f, 0.f};
    else v = (p.gamma && n < p.N) ? *(const f32x4_t*)(p.gamma + n) : f32x4_t{1.f, 1.f, 1.f, 1.f};
    *(f32x4_t*)(slab + (lane < 32 ? 0 : 512) + c * 4) = v;
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // the constants, before any DMA is counted
  constexpr unsigned OOB = 0xFFFFFFF0u;   // a masked store's offset: past every extent (host: < 0xFFFFFF00)
  const u16* const hi_in = p.ln_xb_out;
  const unsigned char* const lo_in = (const unsigned char*)p.ln_xl;
  const unsigned row_b = (unsigned)(p.M * p.ldc * 2);              // bytes of hi (lo: half)
  const __amdgpu_buffer_rsrc_t rs_hi = __builtin_amdgcn_make_buffer_rsrc((void*)p.ln_xb_out, (short)0, (int)row_b, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_lo = __builtin_amdgcn_make_buffer_rsrc((void*)p.ln_xl, (short)0, (int)(row_b / 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_c = __builtin_amdgcn_make_buffer_rsrc(p.C ? p.C : (void*)p.ln_xl, (short)0,
                                                                        p.C ? (int)(2 * row_b) : 0, 0x00020000);
  const int nch = p.N / 128;
  const __amdgpu_buffer_rsrc_t rs_pt = __builtin_amdgcn_make_buffer_rsrc(
      p.ln_part_out ? (void*)p.ln_part_out : (void*)p.ln_xl, (short)0, p.ln_part_out ? (int)(p.M * nch * 8) : 0,
      0x00020000);
  const uint32_t slab_lds = __builtin_amdgcn_readfirstlane(lds_addr(slab)) + 1024;
  // chunk i = (fm, h): rows fm * 16 .. + 15, columns h * 64 .. + 63 of the wave's range; ring slot
  // i & 3.  hi: [16][128 B], piece pc = rows pc * 8 + lane / 8, 8 lanes x 16 B per row, physical 16-B
  // chunk lane & 7 = logical (lane & 7) ^ ((row >> 1) & 7).  lo: [16][64 B], one piece, 4 lanes x
  // 16 B per row (row lane / 4), physical chunk lane & 3 = logical (lane & 3) ^ ((row >> 2) & 3).
  auto dma = [&](int i) __attribute__((always_inline)) {
    const int fm = i >> 1, h = i & 1;
    #pragma unroll
    for (int pc = 0; pc < 2; ++pc) {
      const int r = pc * 8 + (lane >> 3);
      const int m = min(m_base + fm * 16 + r, p.M - 1);
      const long long o = (long long)m * p.ldc + n_base + h * 64 + (((lane & 7) ^ ((r >> 1) & 7)) << 3);
      glds16(hi_in + o, slab_lds + (i & 3) * CB + pc * 1024);
    }
    const int r = lane >> 2;
    const int m = min(m_base + fm * 16 + r, p.M - 1);
    glds16(lo_in + (long long)m * p.ldc + n_base + h * 64 + (((lane & 3) ^ ((r >> 2) & 3)) << 4),
           slab_lds + (i & 3) * CB + LO);
  };
  #pragma unroll
  for (int i = 0; i < AHEAD && i < NI; ++i) dma(i);
  float sh = 0.f, s1 = 0.f, s2 = 0.f;
  #pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int fm = i >> 1, h = i & 1;
    char* const buf = slab + 1024 + (i & 3) * CB;
    if (i + AHEAD < NI) dma(i + AHEAD);
    wait_vmcnt_le<48>(younger(i));   // a constant once the loop is unrolled
    const int m = m_base + fm * 16 + t;
    const bool mok = m < p.M;
    #pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int fn = h * 4 + f;
      const int off = t * 128 + (((f * 2 + (g >> 1)) ^ ((t >> 1) & 7)) << 4) + (g & 1) * 8;
      const int loff = LO + t * 64 + ((f ^ ((t >> 2) & 3)) << 4) + g * 4;
      const uint2 hv = *(const uint2*)(buf + off);
      const uint32_t lv = *(const uint32_t*)(buf + loff);
      const float hf[4] = {K_::to_f(hv.x & 0xffff), K_::to_f(hv.x >> 16), K_::to_f(hv.y & 0xffff), K_::to_f(hv.y >> 16)};
      const f32x4_t b = *(const f32x4_t*)(slab + (fn * 16 + 4 * g) * 4);
      const f32x4_t q = *(const f32x4_t*)(slab + 512 + (fn * 16 + 4 * g) * 4);
      f32x4_t x;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = acc[fm][fn][r] + b[r];
        x[r] = v * q[r] + lo8_decode<K_>(hf[r], unpack_i8(lv, r));
      }
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, x), rs_c,
                                             mok ? (unsigned)(((long long)m * p.ldc + n_base + fn * 16 + 4 * g) * 4)
                                                 : OOB, 0, 0);
      if (fn == 0) {
        sh = __shfl(x[0], t);             // the row's value at column n_base (lane t, g = 0)
        s1 = 0.f;
        s2 = 0.f;
      }
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d = x[r] - sh;
        s1 += d;
        s2 += d * d;
      }
      uint2 wh;
      wh.x = K_::pack2(x[0], x[1]);
      wh.y = K_::pack2(x[2], x[3]);
      const uint32_t wl = pack_i8x4(lo8_encode<K_>(x[0], K_::to_f(wh.x & 0xffff)), lo8_encode<K_>(x[1], K_::to_f(wh.x >> 16)),
                                    lo8_encode<K_>(x[2], K_::to_f(wh.y & 0xffff)), lo8_encode<K_>(x[3], K_::to_f(wh.y >> 16)));
      *(uint2*)(buf + off) = wh;
      *(uint32_t*)(buf + loff) = wl;
    }
    if (h == 1) {
      // the row's 128 columns: 4 lanes (g) of 32 values each
      s1 += __shfl_xor(s1, 16);
      s2 += __shfl_xor(s2, 16);
      s1 += __shfl_xor(s1, 32);
      s2 += __shfl_xor(s2, 32);
      const float mc = sh + s1 * (1.f / 128);
      const float m2 = s2 - s1 * (s1 * (1.f / 128));
      const unsigned po = (g == 0 && mok) ? (unsigned)(((long long)m * nch + n_base / 128) * 8) : OOB;
      // sc1 (write-through): another workgroup of the row tile may merge it (ln_merge_last)
      __builtin_amdgcn_raw_buffer_store_b64(u32x2_t{__float_as_uint(mc), __float_as_uint(m2)}, rs_pt, po, 0, 16);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's staging writes
    #pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int row = k * 8 + (lane >> 3), chunk = lane & 7;
      const int o = row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
      const uint4 dh = *(const uint4*)(buf + o);
      const int mm = m_base + fm * 16 + row;
      const unsigned bo = mm < p.M ? (unsigned)(((long long)mm * p.ldc + n_base + h * 64 + chunk * 8) * 2) : OOB;
      __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{dh.x, dh.y, dh.z, dh.w}, rs_hi, bo, 0, 0);
    }
    {
      const int row = lane >> 2, chunk = lane & 3;
      const uint4 dl = *(const uint4*)(buf + LO + row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4));
      const int mm = m_base + fm * 16 + row;
      const unsigned bo = mm < p.M ? (unsigned)((long long)mm * p.ldc + n_base + h * 64 + chunk * 16) : OOB;
      __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{dl.x, dl.y, dl.z, dl.w}, rs_lo, bo, 0, 0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // read back before this slot's next DMA
  }
}

// The split producer's row merge (ABI 13, p.ln_rs_out): after its epilogue every workgroup of a
// row tile adds one to the tile's counter; the last of the tiles_n arrivals merges the tile's rows
// from ln_part_out (stored write-through, sc1, and drained before the add; read back with sc1
// loads) into ln_rs_out and resets the counter for the next launch.  Replaces the persistent
// consumer's pre-pass launch (ln_merge_kernel).  Guideline 16's sc1 hand-off, no fences: the
// measured-valid form of MI355X_MICROARCH.md's hand-off table, row 1 (every byte stored sc1 and
// drained by each storing wave before the barrier, ONE lane's agent-scope add to one counter, the
// last adder's workgroup loading only with sc1 buffer loads after a barrier) -- an agent-scope
// acq_rel add would also write back the XCD L2's dirty lines of the whole epilogue (~2-6 us per
// workgroup at the end of every proj / fc2).  The signal fences keep the compiler from moving the
// loads above the add (the barrier orders them too).
__device__ __forceinline__ void ln_merge_last(const GemmP& p, int tile_m, int rows, char* smem, int tid) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's part stores (sc1) have landed
  __syncthreads();
  int* last = (int*)smem;
  if (tid == 0) {
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    const unsigned old = __hip_atomic_fetch_add(p.ln_cnt + tile_m, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    *last = old == (unsigned)(p.tiles_n - 1);
  }
  __syncthreads();
  if (!*last) return;
  if (tid == 0) __hip_atomic_store(p.ln_cnt + tile_m, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const __amdgpu_buffer_rsrc_t rs_pt = __builtin_amdgcn_make_buffer_rsrc((void*)p.ln_part_out, (short)0,
                                                                         (int)(p.M * 64), 0x00020000);
  for (int r = tid; r < rows; r += blockDim.x) {
    const int m = tile_m * rows + r;
    if (m >= p.M) break;
    f32x4_t c[4];
    #pragma unroll
    for (int i = 0; i < 4; ++i)
      c[i] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rs_pt, (unsigned)(m * 64 + i * 16), 0, 16));
    *(float2*)(p.ln_rs_out + 2LL * m) = ln_merge_row(c, p.ln_eps);
  }
}

template <typename K_, int EACT, int LNM = 0>   // LNM: 1 folded-LN producer, 2 consumer, 3 (4) producer on hi + lo
__global__ void __launch_bounds__(512, 1) gemm_8ph320_kernel(const GemmP p) {
  constexpr int BM = 320;
  constexpr int A_BYTES = BM * 128, B_BYTES = 256 * 128, BUF = A_BYTES + B_BYTES;
  constexpr int FM = 5, FN = 8, TM = 80, TN = 128;
  constexpr int RING = 2 * BUF;                                   // 144 KiB
  constexpr int PF = 1, SLAB = PF * 16 * TN * 2;                  // epilogue_mfma slab per wave
  constexpr int SMEM = RING > 8 * SLAB ? RING : 8 * SLAB;
  __shared__ __attribute__((aligned(1024))) char smem[SMEM];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int wm = wave & 3, wn = wave >> 2;
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  int tile_m, tile_n;
  tile_coords(p, wgid, tile_m, tile_n);
  const int m0 = tile_m * BM, n0 = tile_n * 256;

  // LDS-DMA pieces: 8 rows x 128 B per wave, the 16-B chunk swizzled on the source address
  const int pchunk = (lane & 7) ^ ((lane >> 3) & 7);
  // byte offsets of this lane's rows from the step's scalar base (saddr DMA; the planner's off32:
  // M * lda, N * ldb < 2^31 elements)
  uint32_t aoff[5];
  #pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int m = m0 + j * 64 + wave * 8 + (lane >> 3);
    aoff[j] = 2u * (uint32_t)((m < p.M ? m : p.M - 1) * (int)p.lda + pchunk * 8);
  }
  // B quarter q = output columns {q*32 .. +31} u {128 + q*32 .. +31}: waves 0-3 / 4-7 take 8 rows each
  const int brow0 = wave_u < 4 ? wave_u * 8 : 128 + (wave_u - 4) * 8;   // + q * 32
  const uint32_t boff = 2u * (uint32_t)((n0 + brow0 + (lane >> 3)) * (int)p.ldb + pchunk * 8);
  const uint32_t lds0 = __builtin_amdgcn_readfirstlane(lds_addr(smem));
  auto issueA = [&](int j, int t) {
    glds16s(aoff[j], p.A + t * 64, lds0 + (t & 1) * BUF + j * 8192 + wave_u * 1024);
  };
  auto issueB = [&](int q, int t) {
    glds16s(boff, p.B + (q * 32 * (int)p.ldb + t * 64), lds0 + (t & 1) * BUF + A_BYTES + (brow0 + q * 32) * 128);
  };

  f32x4_t acc[FM][FN];
  #pragma unroll
  for (int i = 0; i < FM; ++i)
    #pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int frow = lane & 15, fchunk = lane >> 4;
  uint4 af[2][FM], bf[2][2];
  // fragment addresses: per-lane bases (buffer 0) per ks + ds_read immediates -- fragment row r =
  // 16 f + frow (+ 80 wm / 32 q) has r & 7 = frow & 7, so its swizzled chunk is lane-fixed.  Buffer 1
  // sits BUF (72 KiB) above, past the 16-bit immediate: one add on a laundered base (the compiler
  // would otherwise keep all four bases live across the loop)
  typedef __attribute__((address_space(3))) const char lds_c;
  typedef __attribute__((address_space(3))) const u32x4_t lds_u4;
  uint32_t abase[2], bbase[2];
  #pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const uint32_t sw = (uint32_t)(((ks * 4 + fchunk) ^ (frow & 7)) << 4);
    abase[ks] = lds0 + (wm * TM + frow) * 128 + sw;
    bbase[ks] = lds0 + A_BYTES + (wn * TN + frow) * 128 + sw;
  }
  auto pick = [](const uint32_t (&b)[2], auto buf, int ks) __attribute__((always_inline)) -> uint32_t {
    uint32_t x = b[ks];
    if constexpr (std::is_integral_v<decltype(buf)>) return x + (buf ? (uint32_t)BUF : 0u);
    else if constexpr (decltype(buf)::value == 0) return x;
    else {
      asm volatile("" : "+v"(x));
      return x + (uint32_t)BUF;
    }
  };
  auto readA = [&](auto buf) __attribute__((always_inline)) {
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      lds_c* base = (lds_c*)(uintptr_t)pick(abase, buf, ks);
      #pragma unroll
      for (int fm = 0; fm < FM; ++fm) af[ks][fm] = __builtin_bit_cast(uint4, *(lds_u4*)(base + fm * 16 * 128));
    }
  };
  auto readB = [&](int q, auto buf) __attribute__((always_inline)) {
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      lds_c* base = (lds_c*)(uintptr_t)pick(bbase, buf, ks);
      #pragma unroll
      for (int f = 0; f < 2; ++f) bf[ks][f] = __builtin_bit_cast(uint4, *(lds_u4*)(base + (q * 32 + f * 16) * 128));
    }
  };
  auto mma = [&](int q) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      #pragma unroll
      for (int fm = 0; fm < FM; ++fm)
        #pragma unroll
        for (int f = 0; f < 2; ++f) acc[fm][2 * q + f] = K_::mfma16(bf[ks][f], af[ks][fm], acc[fm][2 * q + f]);
    __builtin_amdgcn_s_setprio(0);
  };
  auto bar = [&]() { asm volatile("s_barrier" ::: "memory"); };

  const int KT = p.K / 64;
  // prologue = "step -1" in the steady-state issue order: A(0); Bq0..3(0) with A(1) after Bq2 / Bq3
  #pragma unroll
  for (int j = 0; j < 5; ++j) issueA(j, 0);
  issueB(0, 0);
  issueB(1, 0);
  issueB(2, 0);
  if (KT > 1) { issueA(0, 1); issueA(1, 1); issueA(2, 1); }
  issueB(3, 0);
  if (KT > 1) { issueA(3, 1); issueA(4, 1); }
  // A(0) and Bq0(0) landed: younger are Bq1..3(0) and A(1)
  if (KT > 1) wait_vmcnt<8>(); else wait_vmcnt<3>();
  lds_barrier();
  if (wave >= 4) bar();
  // one K step s in buffer buf (a std::integral_constant when the loop below is unrolled by the
  // two buffers -- KT even -- else s & 1)
  auto step = [&](int s, auto buf) __attribute__((always_inline)) {
    const bool a1 = s + 1 < KT, a2 = s + 2 < KT;
    // phase 0: A fragments + B quarter 0; retire Bq1(s) (younger: 2 + 6 a1)
    readA(buf); readB(0, buf);
    if (a1) issueB(0, s + 1);
    if (a1) wait_vmcnt<8>(); else wait_vmcnt<2>();
    bar(); mma(0); bar();
    // phase 1: retire Bq2(s) (younger: 1 + 7 a1)
    readB(1, buf);
    if (a1) issueB(1, s + 1);
    if (a1) wait_vmcnt<8>(); else wait_vmcnt<1>();
    bar(); mma(1); bar();
    // phase 2: A(s+2) pieces 0-2 into this step's buffer; retire Bq3(s) (younger: 5 a1 + 3 a2)
    readB(2, buf);
    if (a1) issueB(2, s + 1);
    if (a2) { issueA(0, s + 2); issueA(1, s + 2); issueA(2, s + 2); }
    if (a2) wait_vmcnt<8>(); else if (a1) wait_vmcnt<5>(); else wait_vmcnt<0>();
    bar(); mma(2); bar();
    // phase 3: retire A(s+1) and Bq0(s+1) (younger: 3 + 5 a2)
    readB(3, buf);
    if (a1) issueB(3, s + 1);
    if (a2) { issueA(3, s + 2); issueA(4, s + 2); }
    if (a2) wait_vmcnt<8>(); else if (a1) wait_vmcnt<3>();
    bar(); mma(3); bar();
  };
  if ((KT & 1) == 0) {
    for (int s = 0; s < KT; s += 2) {
      step(s, std::integral_constant<int, 0>{});
      step(s + 1, std::integral_constant<int, 1>{});
    }
  } else {
    for (int s = 0; s < KT; ++s) step(s, s & 1);
  }
  if (wave < 4) bar();
  if (p.dbg & DBG_NO_EPILOGUE) {   // ablation (tools/gemm_bench.py --ablate): no epilogue
    #pragma unroll
    for (int i = 0; i < FM; ++i)
      #pragma unroll
      for (int j = 0; j < FN; ++j) asm volatile("" ::"v"(acc[i][j][0]), "v"(acc[i][j][1]), "v"(acc[i][j][2]), "v"(acc[i][j][3]));
    return;
  }
  lds_barrier();   // the ring is free once every wave has left the K loop
  if constexpr (LNM == 3 || LNM == 4) {
    epilogue_hilo_ln<K_, FM, FN, LNM == 3 ? 3 : 1>(p, acc, smem + wave * 13312, lane, m0 + wm * TM, n0 + wn * TN);
    if (p.ln_rs_out) ln_merge_last(p, tile_m, BM, smem, tid);
  }
  else if constexpr (LNM == 1)
    epilogue_acc32_wide_ln<K_, FM, FN>(p, acc, smem + wave * 8192, lane, m0 + wm * TM, n0 + wn * TN);
  else if constexpr (EACT >= EPI_ACC)
    epilogue_acc32_wide<EACT - EPI_ACC, FM, FN>(p, acc, smem + wave * SLAB, lane, m0 + wm * TM, n0 + wn * TN);
  else if constexpr (LNM == 2)
    epilogue_mfma_lnc<K_, EACT, FM, FN, TN>(p, acc, smem + wave * 8192, lane, m0 + wm * TM, n0 + wn * TN);
  else
    epilogue_mfma<K_, EACT, FM, FN, TN, PF>(p, acc, smem + wave * SLAB, lane, m0 + wm * TM, n0 + wn * TN);
}

template <typename K_>
int launch_8ph320(const GemmP& p0, hipStream_t s) {
  GemmP p = p0;
  p.tiles_n = p.N / 256;
  p.tiles_m = (p.M + 319) / 320;
  const int ea = fast_epi_act(p);
  // (a defensive re-check on the GemmP: what the engine takes is stated in serves_8ph320, dp_gemm.hip)
  if (p.N % 256 || ea < 0 || p.relu_a) return DP_ERR_ARG;
  dim3 grid(p.tiles_n * p.tiles_m);
  if (p.ln_xl) {         // folded-LN producer on the split (hi + lo) residual stream
    if (!p.ln_xb_out || p.act != DP_ACT_NONE) return DP_ERR_ARG;
    static_assert(8 * 13312 <= 2 * (320 * 128 + 256 * 128), "hi/lo staging fits the ring");
    if (p.dbg & DBG_HILO_AHEAD1) hipLaunchKernelGGL((gemm_8ph320_kernel<K_, EPI_ACC + DP_ACT_NONE, 4>), grid, dim3(512), 0, s, p);
    else hipLaunchKernelGGL((gemm_8ph320_kernel<K_, EPI_ACC + DP_ACT_NONE, 3>), grid, dim3(512), 0, s, p);
    DP_CHECK_LAUNCH();
    return 0;
  }
  if (p.ln_part_out) {   // folded-LN producer: the residual accumulate
    if (ea != EPI_ACC + DP_ACT_NONE || !p.ln_xb_out) return DP_ERR_ARG;
    hipLaunchKernelGGL((gemm_8ph320_kernel<K_, EPI_ACC + DP_ACT_NONE, 1>), grid, dim3(512), 0, s, p);
    DP_CHECK_LAUNCH();
    return 0;
  }
  if (p.ln_part_in) {    // folded-LN consumer (qkv / fc1): 16-bit C, K = 1024
    switch (ea) {
      case DP_ACT_NONE: hipLaunchKernelGGL((gemm_8ph320_kernel<K_, DP_ACT_NONE, 2>), grid, dim3(512), 0, s, p); break;
      case DP_ACT_GELU: hipLaunchKernelGGL((gemm_8ph320_kernel<K_, DP_ACT_GELU, 2>), grid, dim3(512), 0, s, p); break;
      default: return DP_ERR_ARG;
    }
    DP_CHECK_LAUNCH();
    return 0;
  }
  switch (ea) {
    case DP_ACT_NONE: hipLaunchKernelGGL((gemm_8ph320_kernel<K_, DP_ACT_NONE>), grid, dim3(512), 0, s, p); break;
    case DP_ACT_RELU: hipLaunchKernelGGL((gemm_8ph320_kernel<K_, DP_ACT_RELU>), grid, dim3(512), 0, s, p); break;
    case DP_ACT_GELU: hipLaunchKernelGGL((gemm_8ph320_kernel<K_, DP_ACT_GELU>), grid, dim3(512), 0, s, p); break;
    case EPI_ACC + DP_ACT_NONE: hipLaunchKernelGGL((gemm_8ph320_kernel<K_, EPI_ACC + DP_ACT_NONE>), grid, dim3(512), 0, s, p); break;
    default: return DP_ERR_ARG;
  }
  DP_CHECK_LAUNCH();
  return 0;
}

}  // namespace

namespace dpg {
int launch_part_8ph320(const GemmP& p, bool conv, bool bf16, hipStream_t s) {
  if (conv) return DP_ERR_ARG;
  return bf16 ? launch_8ph320<KBF16>(p, s) : launch_8ph320<KF16>(p, s);
}
}  // namespace dpg
