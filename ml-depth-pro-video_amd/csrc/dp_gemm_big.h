#pragma once
// dp_gemm_big.h -- the big-tile engine (gemm_big_kernel, launch_big): BM x BN x 64 tiles, BM x BN
// in {256 x 256, 256 x 128, 128 x 128, 320 x 256, 512 x 128}; 512 threads = 8 wave64s, or 4 with
// two workgroups per CU.  Operands stream global -> LDS by LDS-DMA into an NS-stage ring; the
// loads for K-tile t+2 are issued as soon as tile t has been consumed, so a whole tile of MFMA
// work covers their latency.  The 256-row A panel halves L2->LDS traffic per FLOP compared with a
// 128^2 tile.  Instantiated by dp_gemm_big.hip (256 x 256, 256 x 128, grouped 128 x 128),
// dp_gemm_big320.hip (320 x 256, 512 x 128), dp_gemm_splitk.hip (SPLIT) and dp_gemm_small.hip
// (launch_dual: NW = 4).

#include "dp_gemm_dev.h"
#include "dp_gemm_epilogue.h"
#include "dp_ln_merge.h"

namespace {

// NW = waves per workgroup: 8 (one workgroup per CU), or 4 (two workgroups per CU, each
// wave one per SIMD: one workgroup's epilogue runs beside the other's K loop).
// EACT: -1 = the general epilogue (runtime operand set); DP_ACT_* = the load-free MFMA-layout
// epilogue with that activation (epilogue_mfma; fast_epi_act decides on the host); EPI_ACC + act:
// epilogue_acc32; EPI_LNP / EPI_LNC + act: the grouped 128 x 128 folded-LayerNorm producer / consumer.
// GRP: a dp_gemm_grouped launch -- the workgroup's problem (wgid / tiles per problem) supplies the
// operand pointers.
template <typename K_, int BM, int BN, int BKT, int NS, bool PIPE, bool CONV, bool RELU, int NW = 8, int EACT = -1,
          bool GRP = false, bool SPLIT = false>
__global__ void __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) gemm_big_kernel(const GemmP p_arg) {
  // 8 waves as WM x WN; the 512 x 128 tile (N = 128 layers) uses 4 x 2 so that every
  // wave still owns a 128 x 64 sub-tile (same fragment reuse as the 256 x 256 tile);
  // 4 waves as 2 x 2 (256 x 128: 128 x 64 per wave)
  constexpr int WN = NW == 4 ? 2 : (BM == 512 ? 2 : 4), WM = NW / WN;
  constexpr int TM = BM / WM, TN = BN / WN;
  constexpr int FM = TM / 16, FN = TN / 16;
  constexpr int RB = BKT * 2;                 // LDS row bytes
  constexpr int CR = BKT / 8;                 // 16-B chunks per row
  constexpr int ROWS_PER_WAVE_PIECE = 1024 / RB;
  constexpr int ROWS_PER_ROUND = NW * ROWS_PER_WAVE_PIECE;  // rows covered by one piece of every wave
  constexpr int A_BYTES = BM * RB, B_BYTES = BN * RB;
  constexpr int STAGE = A_BYTES + B_BYTES;
  constexpr int LA = BM / ROWS_PER_ROUND;     // LDS-DMA pieces per thread per A tile
  constexpr int LB = BN / ROWS_PER_ROUND;
  constexpr int LT = LA + LB;
  constexpr int EPI_BYTES = NW * 32 * (TN + 4) * 4;  // epilogue staging (NW waves x 32 fp32 rows)
  constexpr int SMEM = NS * STAGE > EPI_BYTES ? NS * STAGE : EPI_BYTES;
  static_assert(NS >= 2 && SMEM <= 160 * 1024 && LB >= 1, "LDS ring");
  __shared__ __attribute__((aligned(1024))) char smem[SMEM];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int wm = wave / WN, wn = wave % WN;

  // XCD-aware bijective remap (blocks b and b+8 share an XCD under round-robin dispatch)
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
  int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  GemmP p_grp;
  if constexpr (GRP) {
    const int per = p_arg.tiles_m * p_arg.tiles_n;
    const int g = wgid / per;
    wgid -= g * per;
    p_grp = p_arg;
    const GemmP::Group& q = p_arg.grp[g];
    p_grp.A = q.A; p_grp.B = q.B; p_grp.bias = q.bias; p_grp.gamma = q.gamma; p_grp.pos = q.pos;
    p_grp.R1 = q.R1; p_grp.R2 = q.R2; p_grp.C = q.C;
    p_grp.ln_part_out = q.ln_part_out; p_grp.ln_xb_out = q.ln_xb_out;
    p_grp.ln_part_in = q.ln_part_in; p_grp.ln_colsum = q.ln_colsum;
  }
  // split-K: this workgroup's K-step range and its fp32 partial slab as a plain C (no epilogue
  // operands: the reduce launch applies them to the sum)
  int kbeg = 0, kcnt = p_arg.K / BKT;
  if constexpr (SPLIT) {
    const int per = p_arg.tiles_m * p_arg.tiles_n;
    const int sp = wgid / per;
    wgid -= sp * per;
    const int kt_all = p_arg.K / BKT;
    kbeg = sp * kt_all / p_arg.ksplit;
    kcnt = (sp + 1) * kt_all / p_arg.ksplit - kbeg;
    p_grp = p_arg;
    p_grp.C = p_arg.kpart + (long long)sp * p_arg.M * p_arg.N;
    p_grp.ldc = p_arg.N; p_grp.c_dtype = DP_F32; p_grp.accumulate = 0; p_grp.store_mode = DP_STORE_ROWS;
    p_grp.bias = nullptr; p_grp.gamma = nullptr; p_grp.pos = nullptr; p_grp.R1 = nullptr; p_grp.R2 = nullptr;
    p_grp.act = DP_ACT_NONE; p_grp.row_group = 0; p_grp.head_w = nullptr; p_grp.head_corr = nullptr;
  }
  const GemmP& p = (GRP || SPLIT) ? p_grp : p_arg;
  int tile_m, tile_n;
  tile_coords(p, wgid, tile_m, tile_n);
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  DP_STAMPS_DECL;
  DP_STAMP(st0_);
  // folded-LN consumer (EPI_LNC): thread r < BM asks for tile row r's 8 chunk statistics now (16
  // VGPRs over the K loop, older than every LDS-DMA piece, so the counted waits cover them) and
  // merges them after the loop -- no load latency in the epilogue
  constexpr bool LNP = EACT == EPI_LNP, LNC = EACT >= EPI_LNC;
  static_assert(!(LNP || LNC) || (GRP && BM == 128 && BN == 128 && NW == 8), "folded LN: the grouped 128 x 128 tile");
  f32x4_t lnc_part[4];
  if constexpr (LNC) {
    if (tid < BM) {
      const f32x4_t* pp = (const f32x4_t*)(p.ln_part_in + (long long)min(m0 + tid, p.M - 1) * 16);
      #pragma unroll
      for (int i = 0; i < 4; ++i) lnc_part[i] = pp[i];
    }
  }

  // LDS-DMA piece i of this thread covers tile row i*ROWS_PER_ROUND + wave*ROWS_PER_WAVE_PIECE + lane/CR;
  // LDS slot lane%CR of that row holds logical chunk (lane%CR) ^ swz(row): the swizzle is
  // applied on the SOURCE address, the LDS image stays lane-linear.
  const int prow = wave * ROWS_PER_WAVE_PIECE + lane / CR;
  const int pchunk = BKT == 64 ? ((lane & 7) ^ ((lane >> 3) & 7)) : ((lane & 3) ^ ((lane >> 3) & 3));
  const u16* a_src[LA];
  ConvRow a_cr[LA];
  #pragma unroll
  for (int i = 0; i < LA; ++i) {
    const int m = m0 + i * ROWS_PER_ROUND + prow;
    if constexpr (CONV) {
      a_cr[i] = conv_row(p, m);
    } else {
      a_src[i] = p.A + (long long)(m < p.M ? m : p.M - 1) * p.lda + pchunk * 8;
    }
  }
  const u16* b_src[LB];
  #pragma unroll
  for (int i = 0; i < LB; ++i) {
    const int n = n0 + i * ROWS_PER_ROUND + prow;
    b_src[i] = p.B + (long long)(n < p.N ? n : p.N - 1) * p.ldb + pchunk * 8;
  }
  const uint32_t lds_base = __builtin_amdgcn_readfirstlane(lds_addr(smem)) + wave_u * 1024;
  auto issue = [&](int kt, int stage) {
    const uint32_t sa = lds_base + stage * STAGE;
    const uint32_t sb = sa + A_BYTES;
    const int k0 = (kt + kbeg) * BKT;
    int t_ky = 0, t_kx = 0, t_ci = 0;
    if constexpr (CONV) conv_tap(p, k0, t_ky, t_kx, t_ci);
    #pragma unroll
    for (int i = 0; i < LA; ++i) {
      const void* src;
      if constexpr (CONV) {
        bool inb;
        const u16* s = conv_src(p, a_cr[i], t_ky, t_kx, t_ci + pchunk * 8, inb);
        src = inb ? (const void*)s : (const void*)g_zero_page;
      } else {
        src = a_src[i] + k0;
      }
      glds16(src, sa + i * NW * 1024);
    }
    #pragma unroll
    for (int i = 0; i < LB; ++i) glds16(b_src[i] + k0, sb + i * NW * 1024);
  };

  f32x4_t acc[FM][FN];
  #pragma unroll
  for (int i = 0; i < FM; ++i)
    #pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  // (measured and rejected, round 2: static priority 1 for waves 4-7 instead of the raise / drop
  // around every MFMA group, profiles/r02q_prio_band/)

  const int frow = lane & 15, fchunk = lane >> 4;
  constexpr int KS = BKT / 32;
  auto compute = [&](int stage) {
    const u16* sa = (const u16*)(smem + stage * STAGE);
    const u16* sb = (const u16*)(smem + stage * STAGE + A_BYTES);
    #pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      uint4 bf[FN];
      #pragma unroll
      for (int j = 0; j < FN; ++j)
        bf[j] = *(const uint4*)(sb + lds_off_t<BKT>(wn * TN + j * 16 + frow, ks * 4 + fchunk));
      // all FM A fragments of the sub-step are read up front: the MFMAs then wait
      // on lgkmcnt(FM-1 .. 0) instead of one read at a time (fc1 191 -> 182 us,
      // 768^2 conv 675 -> 650 us on the 320x256 / 256x256 engines, same VGPR count)
      uint4 afs[FM];
      #pragma unroll
      for (int i = 0; i < FM; ++i) afs[i] = *(const uint4*)(sa + lds_off_t<BKT>(wm * TM + i * 16 + frow, ks * 4 + fchunk));
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int i = 0; i < FM; ++i) {
        uint4 af = afs[i];
        if constexpr (RELU) af = relu_pk16(af);
        #pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = K_::mfma16(bf[j], af, acc[i][j]);
      }
      __builtin_amdgcn_s_setprio(0);
    }
  };

  const int KT = kcnt;
  auto nxt = [&](int st) { return st + 1 == NS ? 0 : st + 1; };
  // wait until tile t has landed: tiles issued so far are 0 .. min(KT-1, t+NS-2)
  auto wait_tile = [&](int t) { wait_vmcnt_le<(NS - 2) * LT>(min(NS - 2, KT - 1 - t) * LT); };
  if constexpr (!PIPE) {
    // NS-stage ring, one barrier per K step.  Top of iteration kt: tiles kt ..
    // kt+NS-2 are in flight; wait for tile kt only (counted vmcnt), then the
    // barrier makes it visible to every wave AND certifies that every wave
    // finished compute(kt-1), whose stage is refilled with tile kt+NS-1 right
    // away -- NS-1 steps of MFMA work cover each load.
    #pragma unroll
    for (int t = 0; t < NS - 1; ++t)
      if (t < KT) issue(t, t);
    int stage = 0;
    for (int kt = 0; kt < KT; ++kt) {
      wait_tile(kt);
      lds_barrier();
#ifdef DP_STAMPS
      if (kt == 0) DP_STAMP(st1_);
#endif
      if (kt + NS - 1 < KT && !(p.dbg & DBG_NO_LOOP_LOADS)) {
        const int st = stage + NS - 1;
        issue(kt + NS - 1, st >= NS ? st - NS : st);
      }
      if (p.dbg & DBG_NO_MFMA) {
        const u16* sa = (const u16*)(smem + stage * STAGE);
        uint4 t = *(const uint4*)(sa + lds_off_t<BKT>(wm * TM + frow, fchunk));
        asm volatile("" ::"v"(t.x));
      } else {
        compute(stage);
      }
      stage = nxt(stage);
    }
  } else {
    // NS >= 3: software-pipelined.  The fragments of the next k sub-step (or of
    // the next K step's first sub-step, once its tile is visible) are read from
    // LDS while the MFMAs of the current sub-step run, alternating between two
    // register sets; one barrier per K step, NS-2 steps of loads in flight.
    uint4 fa0[FM], fb0[FN], fa1[FM], fb1[FN];
    auto rd = [&](uint4 (&fa)[FM], uint4 (&fb)[FN], int stg, int ks) {
      const u16* sa = (const u16*)(smem + stg * STAGE);
      const u16* sb = (const u16*)(smem + stg * STAGE + A_BYTES);
      #pragma unroll
      for (int j = 0; j < FN; ++j)
        fb[j] = *(const uint4*)(sb + lds_off_t<BKT>(wn * TN + j * 16 + frow, ks * 4 + fchunk));
      #pragma unroll
      for (int i = 0; i < FM; ++i)
        fa[i] = *(const uint4*)(sa + lds_off_t<BKT>(wm * TM + i * 16 + frow, ks * 4 + fchunk));
    };
    auto mma = [&](const uint4 (&fa)[FM], const uint4 (&fb)[FN]) {
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int i = 0; i < FM; ++i) {
        uint4 a = fa[i];
        if constexpr (RELU) a = relu_pk16(a);
        #pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = K_::mfma16(fb[j], a, acc[i][j]);
      }
      __builtin_amdgcn_s_setprio(0);
    };
    #pragma unroll
    for (int t = 0; t < NS - 1; ++t)
      if (t < KT) issue(t, t);
    wait_tile(0);
    lds_barrier();
    DP_STAMP(st1_);
    rd(fa0, fb0, 0, 0);
    int stage = 0;
    if constexpr (KS == 2) {
      for (int kt = 0; kt < KT; ++kt) {
        if (kt + NS - 1 < KT) {
          int st = stage + NS - 1;
          issue(kt + NS - 1, st >= NS ? st - NS : st);
        }
        rd(fa1, fb1, stage, 1);
        mma(fa0, fb0);
        const int nst = nxt(stage);
        if (kt + 1 < KT) {
          wait_tile(kt + 1);
          lds_barrier();
          rd(fa0, fb0, nst, 0);
        }
        mma(fa1, fb1);
        stage = nst;
      }
    } else {
      for (int kt = 0; kt < KT; kt += 2) {
        if (kt + NS - 1 < KT) {
          int st = stage + NS - 1;
          issue(kt + NS - 1, st >= NS ? st - NS : st);
        }
        int nst = nxt(stage);
        if (kt + 1 < KT) {
          wait_tile(kt + 1);
          lds_barrier();
          rd(fa1, fb1, nst, 0);
        }
        mma(fa0, fb0);
        stage = nst;
        if (kt + 1 >= KT) break;
        if (kt + NS < KT) {
          int st = stage + NS - 1;
          issue(kt + NS, st >= NS ? st - NS : st);
        }
        nst = nxt(stage);
        if (kt + 2 < KT) {
          wait_tile(kt + 2);
          lds_barrier();
          rd(fa0, fb0, nst, 0);
        }
        mma(fa1, fb1);
        stage = nst;
      }
    }
  }

  DP_STAMP(st2_);
  if (p.dbg & DBG_NO_EPILOGUE) {
    #pragma unroll
    for (int i = 0; i < FM; ++i)
      #pragma unroll
      for (int j = 0; j < FN; ++j) asm volatile("" ::"v"(acc[i][j][0]), "v"(acc[i][j][1]), "v"(acc[i][j][2]), "v"(acc[i][j][3]));
    return;
  }
  if constexpr (LNC) {
    // folded-LN consumer: the tile rows' (rstd, -rstd * mean), merged once per workgroup (table
    // beside the ring), then epilogue_mfma with them
    __shared__ float2 ln_rs_s[BM];
    if (tid < BM) ln_rs_s[tid] = ln_merge_row(lnc_part, p.ln_eps);
    lds_barrier();  // the ring is free once every wave has left the K loop; the table is written
    constexpr int PF = (FM * 16 * TN * 2 * NW <= SMEM) ? FM : FM / 2;
    epilogue_mfma<K_, EACT - EPI_LNC, FM, FN, TN, PF, true>(p, acc, smem + wave * (PF * 16 * TN * 2), lane,
                                                             m0 + wm * TM, n0 + wn * TN, ln_rs_s + wm * TM);
    return;
  } else if constexpr (LNP) {
    // folded-LN producer: every wave leaves its rows' 32-column sums in the table (beside the
    // ring: no barrier before), then thread r merges tile row r's four into part[m][chunk n0 / 128]
    static_assert(WN == 4 && TN == 32, "one 128-column chunk over 4 waves");
    __shared__ f32x4_t ln_st[BM * 4];
    epilogue_acc32_ln<K_, FM, FN>(p, acc, ln_st + wm * TM * 4 + wn, lane, m0 + wm * TM, n0 + wn * TN);
    lds_barrier();
    if (tid < BM && m0 + tid < p.M) {
      f32x4_t e[4];
      #pragma unroll
      for (int w = 0; w < 4; ++w) e[w] = ln_st[tid * 4 + w];
      *(float2*)(p.ln_part_out + ((long long)(m0 + tid) * (p.N / 128) + n0 / 128) * 2) = ln_chunk_merge(e);
    }
    return;
  } else if constexpr (EACT >= EPI_ACC) {
    epilogue_acc32<EACT - EPI_ACC, FM, FN>(p, acc, lane, m0 + wm * TM, n0 + wn * TN);
    return;
  } else if constexpr (EACT >= 0) {
    lds_barrier();  // the ring is free once every wave has left the K loop
    constexpr int PF = (FM * 16 * TN * 2 * NW <= SMEM) ? FM : FM / 2;
    epilogue_mfma<K_, EACT, FM, FN, TN, PF>(p, acc, smem + wave * (PF * 16 * TN * 2), lane, m0 + wm * TM,
                                            n0 + wn * TN);
    return;
  }
  // Epilogue through LDS: the MFMA layout gives each lane 4 columns of one row
  // (16 rows x 32-64 B per store instruction -- partial cache lines, measured at
  // ~half of the kernel's time on the ViT shapes).  Each wave instead parks 32
  // rows of its fp32 tile in a private LDS slab and reads them back row-major,
  // so every lane owns 8 consecutive columns and a store instruction writes
  // whole 128-256 B row segments.
  lds_barrier();  // the ring is free once every wave has left the K loop
  constexpr int SROW = TN + 4;                // fp32 row stride (bank-conflict-free writes)
  constexpr int CPR = TN / 8;                 // 8-column chunks per row
  constexpr int RPI = 64 / CPR;               // rows per read instruction
  float* stg = (float*)smem + wave * (32 * SROW);
  constexpr int NIT = 32 / RPI;
  const int c8 = (lane % CPR) * 8, n_l = n0 + wn * TN + c8;
  ColConst cc;
  load_colconst(p, n_l, cc);
  #pragma unroll
  for (int q = 0; q < FM / 2; ++q) {          // 32 rows (two 16-row fragments) per pass
    #pragma unroll
    for (int i = 0; i < 2; ++i)
      #pragma unroll
      for (int j = 0; j < FN; ++j)
        *(f32x4_t*)(stg + (i * 16 + (lane & 15)) * SROW + j * 16 + 4 * (lane >> 4)) = acc[2 * q + i][j];
    // rows of per-row operands batched per epilogue call: all of a pass's rows, except
    // for the 128-160-row wave tiles whose accumulators leave room for only 2 at a time
    constexpr int NITC = FM >= 8 && NIT > 2 ? 2 : NIT;
    #pragma unroll
    for (int c0 = 0; c0 < NIT; c0 += NITC) {
      float v[NITC][8];
      int ms[NITC];
      #pragma unroll
      for (int it = 0; it < NITC; ++it) {
        const int row = (c0 + it) * RPI + lane / CPR;
        const f32x4_t lo = *(const f32x4_t*)(stg + row * SROW + c8);
        const f32x4_t hi = *(const f32x4_t*)(stg + row * SROW + c8 + 4);
        #pragma unroll
        for (int r = 0; r < 4; ++r) { v[it][r] = lo[r]; v[it][4 + r] = hi[r]; }
        ms[it] = m0 + wm * TM + q * 32 + row;
      }
      if constexpr (TN % 32 == 0) {
        if (p.store_mode == DP_STORE_HEAD_PS) {
          head_ps_rows<NITC>(p, cc, ms, n_l, v, lane);
          continue;
        }
      }
      epilogue_rows<K_, NITC, CONV && BM == 512 && !RELU>(p, cc, ms, n_l, v);
    }
  }
  DP_STAMP(st3_);
  DP_STAMP_SAVE(wgid);
}

// NS = ring depth; PIPE = software-pipelined fragment reads (two register sets:
// only affordable for BN = 128, the 256x256 accumulators leave no room).
template <typename K_, int BM, int BN, int BKT, int NS, bool PIPE>
int launch_big(const GemmP& p0, bool conv, hipStream_t s) {
  GemmP p = p0;
  p.tiles_n = (p.N + BN - 1) / BN;
  p.tiles_m = (p.M + BM - 1) / BM;
  dim3 grid(p.tiles_n * p.tiles_m);
  // the load-free epilogue for launches without per-row operands (needs_rowld), on the BK = 64
  // engines the planner picks; debug 1 << 20: always the general one (A/B)
  int ea = BKT == 64 ? fast_epi_act(p) : -1;
  if (ea >= EPI_ACC && p.N % BN != 0) ea = -1;   // epilogue_acc32 has no column predicate: whole column tiles only
  if (p.groups > 1) {
    // grouped launches (the side encoders' dense GEMMs) exist for the 256 x 128 / 128 x 128 dense engines
    if constexpr ((BM == 256 || BM == 128) && BN == 128 && BKT == 64 && NS == 3 && PIPE) {
      if (conv || p.relu_a) return DP_ERR_ARG;
      dim3 g(p.tiles_n * p.tiles_m * p.groups);
#define DP_GRP(E_) hipLaunchKernelGGL((gemm_big_kernel<K_, BM, BN, 64, 3, true, false, false, 8, E_, true>), g, dim3(NT_BIG), 0, s, p)
      // the folded-LN forms (dp_gemm_grouped checked them): the 128 x 128 tile's own epilogues
      const bool lnp = p.grp[0].ln_part_out, lnc = p.grp[0].ln_part_in;
      if constexpr (BM == 128) {
        if (lnp) DP_GRP(EPI_LNP);
        else if (lnc && p.act == DP_ACT_GELU) DP_GRP(EPI_LNC + DP_ACT_GELU);
        else if (lnc) DP_GRP(EPI_LNC + DP_ACT_NONE);
      } else if (lnp || lnc) {
        return DP_ERR_ARG;
      }
      if (lnp || lnc) { /* launched above */ }
      else if (ea == DP_ACT_NONE) DP_GRP(DP_ACT_NONE);
      else if (ea == DP_ACT_GELU) DP_GRP(DP_ACT_GELU);
      else if (ea == EPI_ACC) DP_GRP(EPI_ACC);
      else DP_GRP(-1);
#undef DP_GRP
      DP_CHECK_LAUNCH();
      return 0;
    } else {
      return DP_ERR_ARG;
    }
  }
#define DP_BIGE(C_, R_, E_) hipLaunchKernelGGL((gemm_big_kernel<K_, BM, BN, BKT, NS, PIPE, C_, R_, 8, E_>), grid, dim3(NT_BIG), 0, s, p)
#define DP_BIG(C_, R_) do { \
    if (ea < 0) DP_BIGE(C_, R_, -1); \
    else if constexpr (BKT == 64) { \
      if (ea == DP_ACT_NONE) DP_BIGE(C_, R_, DP_ACT_NONE); \
      else if (ea == DP_ACT_RELU) DP_BIGE(C_, R_, DP_ACT_RELU); \
      else if (ea == DP_ACT_GELU) DP_BIGE(C_, R_, DP_ACT_GELU); \
      else if constexpr (!C_ && !R_) { if (ea == EPI_ACC) DP_BIGE(C_, R_, EPI_ACC); else DP_BIGE(C_, R_, -1); } \
      else DP_BIGE(C_, R_, -1); } \
  } while (0)
  if (conv && p.relu_a) DP_BIG(true, true);
  else if (conv) DP_BIG(true, false);
  else if (p.relu_a) DP_BIG(false, true);
  else DP_BIG(false, false);
#undef DP_BIG
#undef DP_BIGE
  DP_CHECK_LAUNCH();
  return 0;
}

}  // namespace
