// dp_gemm_8ph.hip: the 8-phase 256 x 256 engine.
//
// 256 x 256 x 64 tile, 8 waves (2 x 4, wave tile 128 x 64), K loop cut into 4
// phases per K tile -- one 64 x 32 C quadrant x K 64 = 16 MFMAs per wave per
// phase -- each phase {fragment ds_reads, ONE half-tile LDS-DMA prefetch,
// s_barrier, lgkmcnt(0), 16 MFMAs at raised priority, s_barrier}.  The LDS
// holds 2 K tiles as 4 half-tiles each (A rows 0-127 / 128-255, B cols
// 0-127 / 128-255, 16 KiB each); a half is refilled one phase after its last
// read, so global loads stream continuously with up to 3 half-tiles in flight
// and the only vmcnt wait is once per K tile (counted, never a drain while
// tiles remain).  Quadrant order (qm,qn): (0,0) (0,1) (1,0) (1,1); reads:
// p0 A(qm0)+B(qn0), p1 B(qn1), p2 A(qm1), p3 none.  Issue order of tile
// t+1 / t+2 halves: p0 A0(t+1), p1 A1(t+1), p2 B0(t+2), p3 B1(t+2).
#include "dp_gemm_dev.h"
#include "dp_gemm_epilogue.h"

namespace {

template <typename K_, bool CONV, bool RELU, int EACT = -1>
__global__ void __launch_bounds__(512, 1) gemm_8ph_kernel(const GemmP p) {
  constexpr int HALF = 128 * 128;   // bytes: 128 rows x 64 16-bit
  constexpr int TILEB = 4 * HALF;   // A0 A1 B0 B1
  constexpr int TN = 64, TM = 128;
  constexpr int EPI_BYTES = 8 * 32 * (TN + 4) * 4;
  constexpr int SMEM = 2 * TILEB > EPI_BYTES ? 2 * TILEB : EPI_BYTES;
  __shared__ __attribute__((aligned(1024))) char smem[SMEM];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int wm = wave >> 2, wn = wave & 3;
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  int tile_m, tile_n;
  tile_coords(p, wgid, tile_m, tile_n);
  const int m0 = tile_m * 256, n0 = tile_n * 256;

  // LDS-DMA pieces: half-tile row r = i*64 + wave*8 + lane/8 (i = 0,1), swizzle on the source
  const int prow = wave * 8 + (lane >> 3);
  const int pchunk = (lane & 7) ^ ((lane >> 3) & 7);
  const u16* a_src[2][2];
  ConvRow a_cr[2][2];
  const u16* b_src[2][2];
  #pragma unroll
  for (int h = 0; h < 2; ++h)
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = m0 + 128 * h + i * 64 + prow;
      if constexpr (CONV) a_cr[h][i] = conv_row(p, m);
      else a_src[h][i] = p.A + (long long)(m < p.M ? m : p.M - 1) * p.lda + pchunk * 8;
      const int n = n0 + 128 * h + i * 64 + prow;
      b_src[h][i] = p.B + (long long)(n < p.N ? n : p.N - 1) * p.ldb + pchunk * 8;
    }
  const uint32_t lds_base = __builtin_amdgcn_readfirstlane(lds_addr(smem)) + wave_u * 1024;
  auto issueA = [&](int h, int t) {  // A half h of K tile t -> buffer t&1
    const uint32_t dst = lds_base + (t & 1) * TILEB + h * HALF;
    int ci = 0, ky = 0, kx = 0;
    if constexpr (CONV) {
      conv_tap(p, t * 64, ky, kx, ci);
    }
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
      const void* src;
      if constexpr (CONV) {
        bool inb;
        const u16* s = conv_src(p, a_cr[h][i], ky, kx, ci + pchunk * 8, inb);
        src = inb ? (const void*)s : (const void*)g_zero_page;
      } else {
        src = a_src[h][i] + t * 64;
      }
      glds16(src, dst + i * 8192);
    }
  };
  auto issueB = [&](int h, int t) {
    const uint32_t dst = lds_base + (t & 1) * TILEB + (2 + h) * HALF;
    #pragma unroll
    for (int i = 0; i < 2; ++i) glds16(b_src[h][i] + t * 64, dst + i * 8192);
  };

  f32x4_t acc[8][4];
  #pragma unroll
  for (int i = 0; i < 8; ++i)
    #pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int frow = lane & 15, fchunk = lane >> 4;
  uint4 af[2][4], bf[2][2][2];
  auto readA = [&](int qm, int buf) {
    const u16* sa = (const u16*)(smem + buf * TILEB + wm * HALF);
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      #pragma unroll
      for (int fm = 0; fm < 4; ++fm)
        af[ks][fm] = *(const uint4*)(sa + lds_off(qm * 64 + fm * 16 + frow, ks * 4 + fchunk));
  };
  auto readB = [&](int qn, int buf) {
    const u16* sb = (const u16*)(smem + buf * TILEB + (2 + (wn >> 1)) * HALF);
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      #pragma unroll
      for (int fn = 0; fn < 2; ++fn)
        bf[qn][ks][fn] = *(const uint4*)(sb + lds_off((wn & 1) * 64 + qn * 32 + fn * 16 + frow, ks * 4 + fchunk));
  };
  auto mma = [&](int qm, int qn) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      #pragma unroll
      for (int fm = 0; fm < 4; ++fm) {
        uint4 a = af[ks][fm];
        if constexpr (RELU) a = relu_pk16(a);
        #pragma unroll
        for (int fn = 0; fn < 2; ++fn)
          acc[qm * 4 + fm][qn * 2 + fn] = K_::mfma16(bf[qn][ks][fn], a, acc[qm * 4 + fm][qn * 2 + fn]);
      }
    __builtin_amdgcn_s_setprio(0);
  };
  auto bar = [&]() { asm volatile("s_barrier" ::: "memory"); };

  const int KT = p.K / 64;
  issueA(0, 0); issueA(1, 0); issueB(0, 0); issueB(1, 0);
  if (KT > 1) {
    issueB(0, 1); issueB(1, 1);
    wait_vmcnt<4>();
  } else {
    wait_vmcnt<0>();
  }
  lds_barrier();
  // Wave rows run staggered by one barrier: while one wave of a SIMD waits on
  // its fragment reads the other issues MFMAs.  Every LDS-DMA wait therefore
  // sits one phase before the first read of what it retires (phase 3 for the
  // next K tile, read from phase 0 on), so both wave groups have passed their
  // wait before either reads.
  if (wm == 1) bar();
  for (int t = 0; t < KT; ++t) {
    const int buf = t & 1;
    const bool n1 = t + 1 < KT, n2 = t + 2 < KT;
    // phase 0: quadrant (0,0)
    readA(0, buf); readB(0, buf);
    if (n1) issueA(0, t + 1);
    bar(); mma(0, 0); bar();
    // phase 1: quadrant (0,1)
    readB(1, buf);
    if (n1) issueA(1, t + 1);
    bar(); mma(0, 1); bar();
    // phase 2: quadrant (1,0)
    readA(1, buf);
    if (n2) issueB(0, t + 2);
    bar(); mma(1, 0); bar();
    // phase 3: quadrant (1,1); tile t+1 must have landed before this phase's first barrier
    if (n2) wait_vmcnt<2>(); else wait_vmcnt<0>();
    if (n2) issueB(1, t + 2);
    bar(); mma(1, 1);
    bar();
  }
  if (wm == 0) bar();
  if (p.dbg & DBG_NO_EPILOGUE) {   // ablation (tools/gemm_bench.py --ablate): no epilogue
    #pragma unroll
    for (int i = 0; i < 8; ++i)
      #pragma unroll
      for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(acc[i][j][0]), "v"(acc[i][j][1]), "v"(acc[i][j][2]), "v"(acc[i][j][3]));
    return;
  }

  if constexpr (EACT >= 0) {
    lds_barrier();   // the ring (128 KiB) is free: a 16 KiB slab per wave holds its whole 128 x 64 tile
    epilogue_mfma<K_, EACT, 8, 4, 64, 8>(p, acc, smem + wave * 16384, lane, m0 + wm * TM, n0 + wn * TN);
    return;
  }
  // epilogue: identical to the big engine (LDS-staged, row-coalesced)
  lds_barrier();
  constexpr int SROW = TN + 4, CPR = TN / 8, RPI = 64 / CPR, NIT = 32 / RPI;
  float* stg = (float*)smem + wave * (32 * SROW);
  const int c8 = (lane % CPR) * 8, n_l = n0 + wn * TN + c8;
  ColConst cc;
  load_colconst(p, n_l, cc);
  #pragma unroll
  for (int q = 0; q < 4; ++q) {
    #pragma unroll
    for (int i = 0; i < 2; ++i)
      #pragma unroll
      for (int j = 0; j < 4; ++j)
        *(f32x4_t*)(stg + (i * 16 + (lane & 15)) * SROW + j * 16 + 4 * (lane >> 4)) = acc[2 * q + i][j];
    #pragma unroll
    for (int c0 = 0; c0 < NIT; c0 += 2) {     // 2 rows per call: 128 accumulators still live
      float v[2][8];
      int ms[2];
      #pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int row = (c0 + it) * RPI + lane / CPR;
        const f32x4_t lo = *(const f32x4_t*)(stg + row * SROW + c8);
        const f32x4_t hi = *(const f32x4_t*)(stg + row * SROW + c8 + 4);
        #pragma unroll
        for (int r = 0; r < 4; ++r) { v[it][r] = lo[r]; v[it][4 + r] = hi[r]; }
        ms[it] = m0 + wm * TM + q * 32 + row;
      }
      epilogue_rows<K_, 2>(p, cc, ms, n_l, v);
    }
  }
}

template <typename K_>
int launch_8ph(const GemmP& p0, bool conv, hipStream_t s) {
  GemmP p = p0;
  p.tiles_n = (p.N + 255) / 256;
  p.tiles_m = (p.M + 255) / 256;
  dim3 grid(p.tiles_n * p.tiles_m);
  const int ea = fast_epi_act(p);   // debug 1 << 20: the general epilogue (A/B)
#define DP_8PH(C_, R_) do { \
    if (ea == DP_ACT_NONE) hipLaunchKernelGGL((gemm_8ph_kernel<K_, C_, R_, DP_ACT_NONE>), grid, dim3(512), 0, s, p); \
    else if (ea == DP_ACT_RELU) hipLaunchKernelGGL((gemm_8ph_kernel<K_, C_, R_, DP_ACT_RELU>), grid, dim3(512), 0, s, p); \
    else if (ea == DP_ACT_GELU) hipLaunchKernelGGL((gemm_8ph_kernel<K_, C_, R_, DP_ACT_GELU>), grid, dim3(512), 0, s, p); \
    else hipLaunchKernelGGL((gemm_8ph_kernel<K_, C_, R_, -1>), grid, dim3(512), 0, s, p); } while (0)   /* (acc: general) */
  if (conv && p.relu_a) DP_8PH(true, true);
  else if (conv) DP_8PH(true, false);
  else if (p.relu_a) DP_8PH(false, true);
  else DP_8PH(false, false);
#undef DP_8PH
  DP_CHECK_LAUNCH();
  return 0;
}

#ifdef DP_STAMPS
// the persistent 8-phase engine: per workgroup and tile (up to P8_STAMP_TILES) [K loop start, K loop
// done (boundary issue + epilogue begin), epilogue done (its stores issued)], + hw_id | xcc_id << 32
constexpr int P8_STAMP_TILES = 8, P8_STAMP_W = 3 * P8_STAMP_TILES + 1;
__device__ unsigned long long g_p8_stamps[P8_STAMP_W * 1024];
#endif

// ============================================ persistent 8-phase 256x256 engine
// gemm_8ph_kernel's K loop run over the workgroup's whole tile list (tiles wgid, wgid + G,
// ... of the band raster, G = min(tiles, CUs)) as ONE stream of K steps: the LDS-DMA of the
// next tile's first K steps is issued by the same per-phase schedule as any other step, so
// it is in flight (or landed) while this tile's epilogue runs, and there is no per-tile
// dispatch, prologue or store drain.  At a tile boundary the next tile's second A tile is
// issued BEFORE the epilogue's stores, so the counted wait that retires it (phase 3 of the
// next tile's first step) can leave the stores draining: vmcnt counts loads, stores and
// LDS-DMA together in issue order (MI355X_MICROARCH.md), and the epilogue issues exactly
// ESTORES buffer stores per lane (every lane stores; rows past M / columns past N get an
// out-of-range offset, dropped by the hardware), so the count is a compile-time constant.
// The epilogue is the load-free MFMA-layout one (bias, activation, gamma; 16-bit C) staged
// through a 2 KiB slab per wave beside the 128 KiB ring (+ 2 x 1 KiB column-constant slots
// per wave: 160 KiB of LDS in all), so no LDS the ring uses is touched.  Dense A only (the ViT's fc1 / qkv).  Requires K >= 128.
// The wave's column constants (bias / gamma of its 64 columns) come from its LDS const slot
// (filled by LDS-DMA with the tile's loads), so the epilogue issues no global load: hipcc
// would put a vmcnt(0) in front of one -- a wait for every LDS-DMA in flight, i.e. the next
// tile's first K steps.
template <typename K_, int ACT, bool HG, bool DCV, bool LNC = false>
__device__ __forceinline__ void epilogue_mfma_buf(const GemmP& p, f32x4_t (&acc)[8][4], char* slab,
                                                  const float* cst, int lane, int m_base, int n_base,
                                                  __amdgpu_buffer_rsrc_t crs, const char* rstat = nullptr) {
  constexpr int FM = 8, FN = 4, TN = 64, PF = 1, CH = TN / 8, RPI = 64 / CH;
  const int t = lane & 15, g = lane >> 4;
  f32x4_t bias[FN], gam[FN];
  #pragma unroll
  for (int fn = 0; fn < FN; ++fn) {
    bias[fn] = *(const f32x4_t*)(cst + fn * 16 + 4 * g);
    if constexpr (HG || LNC) gam[fn] = *(const f32x4_t*)(cst + 64 + fn * 16 + 4 * g);   // LNC: colsum
  }
  // folded LayerNorm: row r = fm * 16 + t of the wave group's 128 lives in the const slot of its
  // wave wn' = r / 32 (each wave DMAs 32 rows' (rstd, -rstd * mean), issue_cst); all 8 read up front
  float2 rst[LNC ? FM : 1];
  if constexpr (LNC) {
    #pragma unroll
    for (int fm = 0; fm < FM; ++fm) {
      const int r = fm * 16 + t;
      rst[fm] = *(const float2*)(rstat + (r >> 5) * 2048 + (r & 31) * 8);
    }
  }
  // DP_STORE_DECONV2X2: a lane's 8 columns are one sub-pixel q and channels co..co+7 for the whole
  // tile, and its rows advance by RPI = 8 pixels per store: (b, y, x) of its first row once per
  // tile, then stepped (the per-store integer divisions cost the 384^2 -> 768^2 deconv 32 us of
  // 158: the same GEMM with a row store ran 126 us, tools/gemm_bench.py)
  int dq = 0, dco = 0, db = 0, dy = 0, dx = 0;
  if constexpr (DCV) {
    const int n = n_base + (lane % CH) * 8;
    dq = n / p.dc_cout;
    dco = n - dq * p.dc_cout;
    const int m = m_base + lane / CH, hw = p.dc_h * p.dc_w;
    db = m / hw;
    const int rr = m - db * hw;
    dy = rr / p.dc_w;
    dx = rr - dy * p.dc_w;
  }
  #pragma unroll
  for (int f0 = 0; f0 < FM; f0 += PF) {
    #pragma unroll
    for (int fm = 0; fm < PF; ++fm)
      #pragma unroll
      for (int fn = 0; fn < FN; ++fn) {
        // packed-f32 arithmetic (the 4 columns of a lane as one vector): same values as the
        // scalar epilogue_mfma, half the VALU issue slots
        f32x4_t x;
        if constexpr (LNC) {
          x = __builtin_elementwise_fma(acc[f0 + fm][fn], (f32x4_t)(rst[f0 + fm].x),
                                        __builtin_elementwise_fma(gam[fn], (f32x4_t)(rst[f0 + fm].y), bias[fn]));
        } else {
          x = acc[f0 + fm][fn] + bias[fn];
        }
        if constexpr (ACT == DP_ACT_RELU) {
          #pragma unroll
          for (int r = 0; r < 4; ++r) x[r] = fmaxf(x[r], 0.f);
        } else if constexpr (ACT == DP_ACT_GELU) {
          x = gelu_erf4(x);
        }
        if constexpr (HG) x = x * gam[fn];
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
      unsigned bo = p.c_bytes;
      if (m < p.M && n < p.N) {
        if constexpr (DCV) {
          // DP_STORE_DECONV2X2 (epilogue4): row m = input pixel (b, y, x), column n = sub-pixel q,
          // channel co -> output pixel (b, 2y + q / 2, 2x + q % 2)
          const long long pix = ((long long)db * 2 * p.dc_h + 2 * dy + (dq >> 1)) * (2 * p.dc_w) + 2 * dx + (dq & 1);
          bo = (unsigned)((pix * p.ldc + dco) * 2);
        } else {
          bo = (unsigned)(((long long)m * p.ldc + n) * 2);
        }
      }
      __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{d.x, d.y, d.z, d.w}, crs, bo, 0, 0);
      if constexpr (DCV) {   // the lane's next row: RPI = 8 pixels on (host: dc_w >= 8)
        dx += RPI;
        if (dx >= p.dc_w) {
          dx -= p.dc_w;
          if (++dy == p.dc_h) { dy = 0; ++db; }
        }
      }
    }
  }
}

template <typename K_, bool RELU, int ACT, bool HG, bool DCV = false, bool LNC = false>
__global__ void __launch_bounds__(512, 1) gemm_p8ph_kernel(const GemmP p) {
  constexpr int HALF = 128 * 128;   // bytes: 128 rows x 64 16-bit
  constexpr int TILEB = 4 * HALF;   // A0 A1 B0 B1
  constexpr int RING = 2 * TILEB;   // 128 KiB
  constexpr int TN = 64, TM = 128;
  constexpr int SLAB = 16 * TN * 2;              // epilogue slab per wave (1 fragment row)
  constexpr int CST = 1024;                      // column-constant slot per wave and tile parity
  constexpr int ESTORES = 8 * 16 * TN * 2 / 1024; // 16-B stores per lane per tile
  // ring | 8 slabs | 8 x 2 const slots = 128 + 16 + 16 KiB
  __shared__ __attribute__((aligned(1024))) char smem[RING + 8 * SLAB + 16 * CST];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int wm = wave >> 2, wn = wave & 3;
  const int G = gridDim.x, bid = blockIdx.x;
  const int T = p.tiles_m * p.tiles_n;
  const int KT = p.K / 64;
  // tile order: the static walk wgid, wgid + G, ... (XCD-contiguous, as the data-parallel
  // launch's rounds).  Measured and rejected: per-XCD tile-ticket queues (a workgroup that
  // starts late takes fewer tiles), 44.63 / 44.56 vs 44.98 / 44.96 fps (profiles/r03c_p8ph/).
  const int xcd = bid & 7, q8 = G >> 3, r8 = G & 7;
  const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  if (wgid >= T) return;
  auto next_tile = [&](int t) { return t + G < T ? t + G : -1; };
  int t_cur = wgid, t_nxt = next_tile(t_cur);

  const int prow = wave * 8 + (lane >> 3);
  const int pchunk = (lane & 7) ^ ((lane >> 3) & 7);
  const uint32_t lds_base = __builtin_amdgcn_readfirstlane(lds_addr(smem)) + wave_u * 1024;

  // issue cursors: the next A K tile to stream is global step sa (tile ta, k ka), the next B
  // K tile step sb (tile tb, k kb); a cursor whose tile is -1 is done (it wraps to its tile's
  // successor in the walk: up to two tiles ahead of the one computed at KT = 2).  32-bit
  // element offsets of this lane's rows (host: M * lda, N * ldb < 2^31).
  int sa = 0, ta = t_cur, ka = 0, sb = 0, tb = t_cur, kb = 0;
  // byte offsets of this lane's rows from the K step's scalar base (p.A + 64 ka, p.B + 64 kb): the
  // DMA is issued in the saddr form, no per-lane 64-bit address arithmetic per K step (host: M * lda,
  // N * ldb < 2^31 elements)
  uint32_t aoff[2][2], boff[2][2];
  auto a_tile = [&](int t) {
    int tm, tn;
    tile_coords(p, t, tm, tn);
    #pragma unroll
    for (int h = 0; h < 2; ++h)
      #pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int m = tm * 256 + 128 * h + j * 64 + prow;
        aoff[h][j] = 2u * (uint32_t)((m < p.M ? m : p.M - 1) * (int)p.lda + pchunk * 8);
      }
  };
  auto b_tile = [&](int t) {
    int tm, tn;
    tile_coords(p, t, tm, tn);
    #pragma unroll
    for (int h = 0; h < 2; ++h)
      #pragma unroll
      for (int j = 0; j < 2; ++j) boff[h][j] = 2u * (uint32_t)((tn * 256 + 128 * h + j * 64 + prow) * (int)p.ldb + pchunk * 8);
  };
  auto issueA = [&](int h) {   // A half h of step sa -> buffer sa & 1
    const uint32_t dst = lds_base + (sa & 1) * TILEB + h * HALF;
    #pragma unroll
    for (int j = 0; j < 2; ++j) glds16s(aoff[h][j], p.A + ka * 64, dst + j * 8192);
  };
  auto nextA = [&]() {
    ++sa;
    if (++ka == KT) {
      ka = 0;
      ta = next_tile(ta);
      if (ta >= 0) a_tile(ta);
    }
  };
  auto issueB = [&](int h) {
    const uint32_t dst = lds_base + (sb & 1) * TILEB + (2 + h) * HALF;
    #pragma unroll
    for (int j = 0; j < 2; ++j) glds16s(boff[h][j], p.B + kb * 64, dst + j * 8192);
  };
  auto nextB = [&]() {
    ++sb;
    if (++kb == KT) {
      kb = 0;
      tb = next_tile(tb);
      if (tb >= 0) b_tile(tb);
    }
  };
  f32x4_t acc[8][4];
  const int frow = lane & 15, fchunk = lane >> 4;
  uint4 af[2][4], bf[2][2][2];
  // fragment addresses: per-lane bases per (buffer, ks) + compile-time ds_read immediates -- a
  // fragment row r = q 64 / 32 + f 16 + frow has r & 7 = frow & 7, so its swizzled chunk is lane-fixed;
  // the K loop below is unrolled by the two buffers (KT even), so the base is a constant choice
  typedef __attribute__((address_space(3))) const char lds_c;
  typedef __attribute__((address_space(3))) const u32x4_t lds_u4;
  uint32_t abase[2], bbase[2];   // buffer 0; buffer 1 sits TILEB above (64 KB: past the ds_read immediate)
  {
    const uint32_t l0 = lds_addr(smem);
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const uint32_t sw = (uint32_t)(((ks * 4 + fchunk) ^ (frow & 7)) << 4);
      abase[ks] = l0 + wm * HALF + frow * 128 + sw;
      bbase[ks] = l0 + (2 + (wn >> 1)) * HALF + ((wn & 1) * 64 + frow) * 128 + sw;
    }
  }
  // the buffer as a std::integral_constant (unrolled loop) or a runtime int (odd KT); buffer 1's
  // address is one add on a laundered base, so the compiler does not keep both in registers
  auto pick = [](const uint32_t (&b)[2], auto buf, int ks) __attribute__((always_inline)) -> uint32_t {
    uint32_t x = b[ks];
    if constexpr (std::is_integral_v<decltype(buf)>) return x + (buf ? (uint32_t)TILEB : 0u);
    else if constexpr (decltype(buf)::value == 0) return x;
    else {
      asm volatile("" : "+v"(x));
      return x + (uint32_t)TILEB;
    }
  };
  auto readA = [&](int qm, auto buf) __attribute__((always_inline)) {
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      lds_c* base = (lds_c*)(uintptr_t)pick(abase, buf, ks);
      #pragma unroll
      for (int fm = 0; fm < 4; ++fm)
        af[ks][fm] = __builtin_bit_cast(uint4, *(lds_u4*)(base + (qm * 64 + fm * 16) * 128));
    }
  };
  auto readB = [&](int qn, auto buf) __attribute__((always_inline)) {
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      lds_c* base = (lds_c*)(uintptr_t)pick(bbase, buf, ks);
      #pragma unroll
      for (int fn = 0; fn < 2; ++fn)
        bf[qn][ks][fn] = __builtin_bit_cast(uint4, *(lds_u4*)(base + (qn * 32 + fn * 16) * 128));
    }
  };
  // FIRST: a tile's first K step -- its ks = 0 MFMAs start from a zero accumulator (no
  // per-tile clearing of the 128 accumulator registers)
  auto mma = [&](int qm, int qn, auto first) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks)
      #pragma unroll
      for (int fm = 0; fm < 4; ++fm) {
        uint4 a = af[ks][fm];
        if constexpr (RELU) a = relu_pk16(a);
        #pragma unroll
        for (int fn = 0; fn < 2; ++fn) {
          f32x4_t& c = acc[qm * 4 + fm][qn * 2 + fn];
          if constexpr (decltype(first)::value) c = K_::mfma16(bf[qn][ks][fn], a, ks == 0 ? f32x4_t{0.f, 0.f, 0.f, 0.f} : c);
          else c = K_::mfma16(bf[qn][ks][fn], a, c);
        }
      }
    __builtin_amdgcn_s_setprio(0);
  };
  auto bar = [&]() { asm volatile("s_barrier" ::: "memory"); };
  const __amdgpu_buffer_rsrc_t crs = __builtin_amdgcn_make_buffer_rsrc((void*)p.C, (short)0, (int)p.c_bytes, 0x00020000);
  char* slab = smem + RING + wave * SLAB;
  // column constants of tile t -> this wave's const slot `par`: ONE LDS-DMA piece per wave
  // (lanes 0-15: bias of the wave's 64 columns, 16-31: gamma, 32-63 repeat 0-31), issued
  // with the tile's loads and retired by the same counted waits (only this wave reads it)
  // LNC (folded-LayerNorm consumer): lanes 16-31 bring the column sums instead of gamma and
  // lanes 32-47 the (rstd, -rstd * mean) of 32 of the wave group's 128 rows (2 rows per lane,
  // rows wn * 32 ..), so the 4 waves of a group hold its rows between them (read across waves
  // in the epilogue: that tile's whole K loop, with its barriers, lies between)
  auto issue_cst = [&](int t, int par) {
    int tm, tn;
    tile_coords(p, t, tm, tn);
    const int l = lane & 15, n = tn * 256 + wn * TN + 4 * l;
    const float* src;
    if ((lane & 16) == 0 && lane < 32) src = p.bias ? p.bias + n : (const float*)g_zero_page + 4 * l;
    else if (lane < 32) src = HG ? p.gamma + n : LNC ? p.ln_colsum + n : (const float*)g_zero_page + 4 * l;
    else if (LNC && lane < 48) {
      // rows past M (the last row tile) re-read the pair holding row M - 1, whose values they
      // never store: the caller's buffer holds M rounded up to even rows
      const int row = tm * 256 + wm * TM + wn * 32 + 2 * (lane - 32);
      src = p.ln_rs + 2 * (row < p.M ? row : ((p.M - 1) & ~1));
    }
    else src = (const float*)g_zero_page + 4 * l;
    glds16(src, __builtin_amdgcn_readfirstlane(lds_addr(smem)) + RING + 8 * SLAB + (wave_u * 2 + par) * CST);
  };

  // prologue: tile 0's column constants, step 0 (A and B) and step 1's B (KT >= 2)
  issue_cst(t_cur, 0);
  a_tile(t_cur);
  b_tile(t_cur);
  issueA(0); issueA(1); nextA();
  issueB(0); issueB(1); nextB();
  issueB(0); issueB(1); nextB();
  wait_vmcnt<4>();
  lds_barrier();
  // wave rows staggered by one barrier (gemm_8ph_kernel); kept across tiles
  if (wm == 1) bar();
  int s = 0;
  // one K step s (k-th of the i-th tile): the 8-phase schedule of gemm_8ph_kernel with the
  // issue cursors deciding what streams in
  auto step = [&](int i, int k, auto first, auto buf) __attribute__((always_inline)) {
    const bool a1 = sa == s + 1 && ta >= 0;   // step s+1's A not issued yet (it was at a boundary)
    const bool b2 = tb >= 0;                  // sb == s + 2
    // phase 0: quadrant (0,0)
    readA(0, buf); readB(0, buf);
    if (a1) issueA(0);
    bar(); mma(0, 0, first); bar();
    // phase 1: quadrant (0,1)
    readB(1, buf);
    if (a1) { issueA(1); nextA(); }
    bar(); mma(0, 1, first); bar();
    // phase 2: quadrant (1,0)
    readA(1, buf);
    if (b2) issueB(0);
    bar(); mma(1, 0, first); bar();
    // phase 3: step s+1 must have landed before this phase's first barrier; younger than
    // it: B0 of step s+2 (this step's phase 2) and, in a tile's first step, the previous
    // tile's epilogue stores (issued after step s+1's loads)
    if (k == 0 && i > 0) {
      if (b2) wait_vmcnt<ESTORES + 2>(); else wait_vmcnt<ESTORES>();
    } else {
      if (b2) wait_vmcnt<2>(); else wait_vmcnt<0>();
    }
    if (b2) { issueB(1); nextB(); }
    bar(); mma(1, 1, first);
    bar();
    ++s;
  };
#ifdef DP_STAMPS
  unsigned long long p8st_[3 * P8_STAMP_TILES] = {};
#endif
  for (int i = 0;; ++i) {
#ifdef DP_STAMPS
    if (i < P8_STAMP_TILES) DP_STAMP(p8st_[3 * i]);
#endif
    using B0 = std::integral_constant<int, 0>;
    using B1 = std::integral_constant<int, 1>;
    if ((KT & 1) == 0) {   // step s = i KT + k is in buffer k & 1
      step(i, 0, std::true_type{}, B0{});
      int k = 1;
      for (; k + 1 < KT; k += 2) {
        step(i, k, std::false_type{}, B1{});
        step(i, k + 1, std::false_type{}, B0{});
      }
      step(i, k, std::false_type{}, B1{});
    } else {
      step(i, 0, std::true_type{}, s & 1);
      for (int k = 1; k < KT; ++k) step(i, k, std::false_type{}, s & 1);
    }
#ifdef DP_STAMPS
    if (i < P8_STAMP_TILES) DP_STAMP(p8st_[3 * i + 1]);
#endif
    // tile boundary: the next tile's second A K tile goes out before the epilogue's stores
    // (its buffer's last reads were this step's phases 0 / 2, two barriers back)
    if (t_nxt >= 0) {
      if (ta >= 0) { issueA(0); issueA(1); nextA(); }
      issue_cst(t_nxt, (i + 1) & 1);
    }
    int tm, tn;
    tile_coords(p, t_cur, tm, tn);
    const float* cst = (const float*)(smem + RING + 8 * SLAB + (wave * 2 + (i & 1)) * CST);
    const char* rstat = smem + RING + 8 * SLAB + (wm * 8 + (i & 1)) * CST + 512;   // wave group's row stats
    epilogue_mfma_buf<K_, ACT, HG, DCV, LNC>(p, acc, slab, cst, lane, tm * 256 + wm * TM, tn * 256 + wn * TN, crs,
                                             rstat);
#ifdef DP_STAMPS
    if (i < P8_STAMP_TILES) DP_STAMP(p8st_[3 * i + 2]);
#endif
    if (t_nxt < 0) break;
    t_cur = t_nxt;
    t_nxt = next_tile(t_cur);
  }
  if (wm == 0) bar();
#ifdef DP_STAMPS
  if (threadIdx.x == 0 && wgid < 1024) {
    unsigned hw_, xcc_;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_));
    unsigned long long* d_ = g_p8_stamps + P8_STAMP_W * wgid;
    for (int j = 0; j < 3 * P8_STAMP_TILES; ++j) d_[j] = p8st_[j];
    d_[3 * P8_STAMP_TILES] = hw_ | ((unsigned long long)xcc_ << 32);
  }
#endif
}

template <typename K_>
int launch_p8ph(const GemmP& p0, hipStream_t s) {
  GemmP p = p0;
  p.tiles_n = p.N / 256;
  p.tiles_m = (p.M + 255) / 256;
  const int T = p.tiles_n * p.tiles_m;
  const bool dcv = p.store_mode == DP_STORE_DECONV2X2;
  const int ea = dcv ? p.act : fast_epi_act(p);
  // (a defensive re-check on the GemmP: what the engine takes is stated in serves_p8ph, dp_gemm.hip)
  if (p.N % 256 || p.K < 128 || !p.c_bytes || p.c_dtype == DP_F32 || ea < 0 || ea >= EPI_ACC) return DP_ERR_ARG;
  int G = num_cus();
  if (G > T) G = T;
  dim3 grid(G);
  if (dcv) {   // the 2x2 stride-2 deconvs: bias only (no per-row operands, no activation)
    if (p.relu_a || p.gamma || p.pos || p.R1 || p.R2 || p.accumulate || p.row_group || p.head_w || p.head_corr ||
        ea != DP_ACT_NONE || p.dc_cout % 8 || p.dbg & DBG_NO_FAST_EPILOGUE)
      return DP_ERR_ARG;
    hipLaunchKernelGGL((gemm_p8ph_kernel<K_, false, DP_ACT_NONE, false, true>), grid, dim3(512), 0, s, p);
    DP_CHECK_LAUNCH();
    return 0;
  }
  if (p.store_mode != DP_STORE_ROWS) return DP_ERR_ARG;
  if (p.ln_rs) {   // folded-LayerNorm consumer (the ViT fc1): dense, no ReLU prologue, no gamma
    if (p.relu_a || p.gamma) return DP_ERR_ARG;
    if (ea == DP_ACT_NONE) hipLaunchKernelGGL((gemm_p8ph_kernel<K_, false, DP_ACT_NONE, false, false, true>), grid, dim3(512), 0, s, p);
    else if (ea == DP_ACT_GELU) hipLaunchKernelGGL((gemm_p8ph_kernel<K_, false, DP_ACT_GELU, false, false, true>), grid, dim3(512), 0, s, p);
    else return DP_ERR_ARG;
    DP_CHECK_LAUNCH();
    return 0;
  }
#define DP_P8(R_, G_) do { \
    if (ea == DP_ACT_NONE) hipLaunchKernelGGL((gemm_p8ph_kernel<K_, R_, DP_ACT_NONE, G_>), grid, dim3(512), 0, s, p); \
    else if (ea == DP_ACT_RELU) hipLaunchKernelGGL((gemm_p8ph_kernel<K_, R_, DP_ACT_RELU, G_>), grid, dim3(512), 0, s, p); \
    else hipLaunchKernelGGL((gemm_p8ph_kernel<K_, R_, DP_ACT_GELU, G_>), grid, dim3(512), 0, s, p); } while (0)
  // (a gamma-free launch -- fc1 -- skips the multiply by 1 per output)
  if (p.relu_a) { if (p.gamma) DP_P8(true, true); else DP_P8(true, false); }
  else { if (p.gamma) DP_P8(false, true); else DP_P8(false, false); }
#undef DP_P8
  DP_CHECK_LAUNCH();
  return 0;
}

}  // namespace

namespace dpg {
int launch_part_8ph(const GemmP& p, int tile, bool conv, bool bf16, hipStream_t s) {
  if (tile == DP_TILE_P8PH_256x256) {
    if (conv) return DP_ERR_ARG;
    return bf16 ? launch_p8ph<KBF16>(p, s) : launch_p8ph<KF16>(p, s);
  }
  return (bf16 ? launch_8ph<KBF16>(p, conv, s) : launch_8ph<KF16>(p, conv, s));
}
}  // namespace dpg

#ifdef DP_STAMPS
// timing-only builds: the persistent 8-phase engine's per-tile stamps of its last launch
// (tools/p8ph_stamps.py); this translation unit instantiates that engine
extern "C" int dp_p8_stamps(void* host_dst, int n_wg) {
  return (int)hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(g_p8_stamps), (size_t)n_wg * P8_STAMP_W * 8, 0,
                                  hipMemcpyDeviceToHost);
}
#endif
