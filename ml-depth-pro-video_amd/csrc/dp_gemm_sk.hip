// dp_gemm_sk.hip: the stream-K engine.
//
// 256 x 256 x 64 tiles, 8 waves (2 x 4, wave tile 128 x 64), one persistent
// workgroup per CU.  The T tiles x KT k-steps of the GEMM form one list of
// "units" (tile-major, k inner) that is cut into G equal contiguous ranges,
// one per workgroup (stream-K), so that
//  * every CU gets the same work (no 3.7-round quantisation tail),
//  * the LDS-DMA ring runs on across tile boundaries: the next tile's first
//    k-step is in flight while the previous tile's epilogue runs (no prologue
//    per tile), and
//  * tile boundaries -- hence the epilogue store bursts -- fall at different
//    times on different CUs instead of all 256 CUs storing at once.
// A range that starts inside a tile computes that tile's last k-steps and
// publishes them as an fp32 partial (write-through stores + flag); the
// workgroup whose range covers the tile's k-step 0 (it reaches it at the END
// of its range) owns the tile: it adds every partial of the tile, then runs the
// normal epilogue.  A workgroup only ever waits for a higher-numbered one,
// which published at the START of its range: no cycle, no deadlock, and the
// spin is bounded (a timeout sets an error word instead of hanging the GPU).
// The epilogue stages 16-row slices through its own 32 KiB of LDS so that the
// 128 KiB ring stays live underneath it.
#include "dp_gemm_dev.h"
#include "dp_gemm_epilogue.h"

namespace {

constexpr int SK_A_BYTES = 256 * 128;            // 256 rows x 64 16-bit
constexpr int SK_STAGE = 2 * SK_A_BYTES;         // A + B
constexpr int SK_RING = 2 * SK_STAGE;            // 2 stages: 128 KiB
constexpr int SK_EPI = 8 * 16 * 64 * 4;          // 8 waves x 16 rows x 64 fp32

struct SkP {
  uint32_t* flags;
  float* part;
  int kt, tiles, units;
};

// ROWLD: the epilogue reads per-row operands (residuals R1/R2, the fp32 C being
// accumulated into, pos-embed); without them it needs ~40 fewer VGPRs.
template <typename K_, bool CONV, bool RELU, bool ROWLD>
__global__ void __launch_bounds__(512, 1) gemm_sk_kernel(const GemmP p, const SkP s) {
  constexpr int TM = 128, TN = 64, FM = 8, FN = 4;
  __shared__ __attribute__((aligned(1024))) char smem[SK_RING + SK_EPI];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int wm = wave >> 2, wn = wave & 3;
  const int G = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, q8 = G >> 3, r8 = G & 7;
  const int w = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int KT = s.kt, U = s.units;
  const int u0 = (int)((long long)w * U / G), u1 = (int)((long long)(w + 1) * U / G);
  auto wg_of_unit = [&](int u) { return (int)(((long long)(u + 1) * G - 1) / U); };
  // Tile positions are walked column-major over an R x G grid of tile ids
  // (id = row * G + column): range w then covers ~column w, i.e. tiles w, w+G,
  // w+2G, ... as in a data-parallel launch, so the tiles in flight at any
  // moment are ~consecutive ids (shared A/B panels in L2), while the fractional
  // range length staggers the tile boundaries across workgroups.
  const int T = s.tiles, R = (T + G - 1) / G, r0 = T - (R - 1) * G;
  auto tile_of = [&](int pos) {
    int c, r;
    if (pos < r0 * R) {
      c = pos / R;
      r = pos - c * R;
    } else {
      const int q = pos - r0 * R;
      c = r0 + q / (R - 1);
      r = q - (c - r0) * (R - 1);
    }
    return r * G + c;
  };

  // ---- LDS-DMA issue side (runs one unit ahead of the MFMAs).  Only the
  // tile's scalar origin is kept: per-lane source addresses are recomputed per
  // issue (a few VALU ops under 64 MFMAs) so the 128 accumulators, the
  // fragments and the epilogue fit in 256 VGPRs without spilling.
  const int prow = wave * 8 + (lane >> 3);
  const int pchunk = (lane & 7) ^ ((lane >> 3) & 7);
  int is_tile = -1, is_m0 = 0, is_n0 = 0;
  ConvRow a_cr[CONV ? 4 : 1];
  const uint32_t lds_base = __builtin_amdgcn_readfirstlane(lds_addr(smem)) + wave_u * 1024;
  auto issue = [&](int u, int stage) {
    const int t = u / KT, ks = u - t * KT;
    if (t != is_tile) {
      is_tile = t;
      const int id = tile_of(t);
      is_m0 = (id / p.tiles_n) * 256;
      is_n0 = (id % p.tiles_n) * 256;
      if constexpr (CONV) {
        #pragma unroll
        for (int i = 0; i < 4; ++i) a_cr[i] = conv_row(p, is_m0 + i * 64 + prow);
      }
    }
    const uint32_t sa = lds_base + stage * SK_STAGE, sb = sa + SK_A_BYTES;
    const int k0 = ks * 64;
    int ky = 0, kx = 0, ci = 0;
    if constexpr (CONV) {
      conv_tap(p, k0, ky, kx, ci);
    }
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
      const void* src;
      if constexpr (CONV) {
        bool inb;
        const u16* q = conv_src(p, a_cr[i], ky, kx, ci + pchunk * 8, inb);
        src = inb ? (const void*)q : (const void*)g_zero_page;
      } else {
        const int m = is_m0 + i * 64 + prow;
        src = p.A + (long long)(m < p.M ? m : p.M - 1) * p.lda + k0 + pchunk * 8;
      }
      glds16(src, sa + i * 8192);
    }
    #pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = is_n0 + i * 64 + prow;
      glds16(p.B + (long long)(n < p.N ? n : p.N - 1) * p.ldb + k0 + pchunk * 8, sb + i * 8192);
    }
  };

  f32x4_t acc[FM][FN];
  auto zero_acc = [&]() {
    #pragma unroll
    for (int i = 0; i < FM; ++i)
      #pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  };
  const int frow = lane & 15, fchunk = lane >> 4;
  auto compute = [&](int stage) {
    const u16* sa = (const u16*)(smem + stage * SK_STAGE);
    const u16* sb = (const u16*)(smem + stage * SK_STAGE + SK_A_BYTES);
    #pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      uint4 bf[FN];
      #pragma unroll
      for (int j = 0; j < FN; ++j) bf[j] = *(const uint4*)(sb + lds_off(wn * TN + j * 16 + frow, ks * 4 + fchunk));
      __builtin_amdgcn_s_setprio(1);
      #pragma unroll
      for (int i = 0; i < FM; ++i) {
        uint4 af = *(const uint4*)(sa + lds_off(wm * TM + i * 16 + frow, ks * 4 + fchunk));
        if constexpr (RELU) af = relu_pk16(af);
        #pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = K_::mfma16(bf[j], af, acc[i][j]);
      }
      __builtin_amdgcn_s_setprio(0);
    }
  };

  // ---- epilogue of one finished tile: 16-row slices through this wave's LDS slab,
  // read back row-major (8 rows x 8 columns per lane instruction pair)
  float* stg = (float*)(smem + SK_RING) + wave * (16 * 64);
  auto epilogue = [&](int t) {
    const int id = tile_of(t);
    const int m0 = (id / p.tiles_n) * 256, n0 = (id % p.tiles_n) * 256;
    const int c8 = (lane & 7) * 8, n_l = n0 + wn * TN + c8;
    ColConst cc;                     // bias / LayerScale of this lane's 8 columns, loaded once
    load_colconst(p, n_l, cc);
    #pragma unroll
    for (int i = 0; i < FM; ++i) {
      // lane holds row (lane & 15), 16-B chunks j*4 + (lane >> 4); chunk index XOR row
      #pragma unroll
      for (int j = 0; j < FN; ++j)
        *(f32x4_t*)(stg + frow * 64 + (((j * 4 + fchunk) ^ frow) << 2)) = acc[i][j];
      float v[2][8];
      int ms[2];
      #pragma unroll
      for (int it = 0; it < 2; ++it) {
        const int row = it * 8 + (lane >> 3);
        const f32x4_t lo = *(const f32x4_t*)(stg + row * 64 + (((2 * (lane & 7)) ^ row) << 2));
        const f32x4_t hi = *(const f32x4_t*)(stg + row * 64 + (((2 * (lane & 7) + 1) ^ row) << 2));
        #pragma unroll
        for (int r = 0; r < 4; ++r) { v[it][r] = lo[r]; v[it][4 + r] = hi[r]; }
        ms[it] = m0 + wm * TM + i * 16 + row;
      }
      if constexpr (ROWLD) {
        epilogue_rows<K_, 2>(p, cc, ms, n_l, v);   // both rows' loads issued before any math
      } else {
        GemmP q = p;
        q.R1 = nullptr; q.R2 = nullptr; q.pos = nullptr; q.accumulate = 0;
        epilogue_rows<K_, 2>(q, cc, ms, n_l, v);
      }
    }
  };

  // partial slot layout: [wave][i][j][lane] x f32x4 -> 1 KiB contiguous per wave instruction
  auto slot_ptr = [&](int q, int i, int j) {
    return s.part + (long long)q * SK_TILE_F + ((((wave * FM + i) * FN + j) * 64 + lane) << 2);
  };
  auto publish = [&]() {
    // write-through (sc1) 16-B buffer stores of this wave's accumulators into slot w:
    // visible to the owner after its agent-scope acquire (Guideline 16, R1)
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc(s.part + (long long)w * SK_TILE_F, (short)0, SK_TILE_F * 4, 0x00020000);
    const int vo = (wave * FM * FN * 64 + lane) * 16;
    #pragma unroll
    for (int i = 0; i < FM; ++i)
      #pragma unroll
      for (int j = 0; j < FN; ++j)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, acc[i][j]), rs, vo + (i * FN + j) * 1024, 0,
                                               16 /* sc1 */);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wave drains its stores
    __syncthreads();
    if (tid == 0) __hip_atomic_store(s.flags + w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  auto absorb = [&](int q) {   // add workgroup q's published partial of the tile
    if (tid == 0) {
      unsigned spins = 0;
      // debug bit 64 (tests only): give up at once, as a starved wait would
      const unsigned limit = (p.dbg & DBG_SK_GIVE_UP) ? 0u : (1u << 24);
      while (__hip_atomic_load(s.flags + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u || (p.dbg & DBG_SK_GIVE_UP)) {
        __builtin_amdgcn_s_sleep(2);
        if (++spins > limit) {  // ~seconds: never hang the GPU; report in the sticky error word instead
          __hip_atomic_store(s.flags + 1023, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
      }
      // consumed: back to 0, so every flag is 0 again when the launch ends (no per-launch
      // clearing; a memset node of a replayed HIP graph raced the next launch's polls and let
      // an owner add the previous replay's partials -- found by tools/parity_probe.py)
      __hip_atomic_store(s.flags + q, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    #pragma unroll
    for (int i = 0; i < FM; ++i) {   // one fragment row at a time (bounded live registers)
      #pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] += *(const f32x4_t*)slot_ptr(q, i, j);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  if (u0 >= u1) return;
  zero_acc();
  issue(u0, 0);
  int stage = 0, seg0 = u0;
  int t = u0 / KT, ks = u0 - t * KT;
  for (int u = u0; u < u1; ++u) {
    wait_vmcnt<0>();
    lds_barrier();
    if (u + 1 < u1) issue(u + 1, stage ^ 1);
    compute(stage);
    stage ^= 1;
    if (ks == KT - 1 || u + 1 == u1) {
      const bool head = seg0 == t * KT;
      if (!head) {
        publish();                       // only ever this range's first segment
      } else {
        if (ks != KT - 1) {              // split tile, owned here: the range's last segment
          const int last = wg_of_unit(t * KT + KT - 1);
          for (int q = w + 1; q <= last; ++q) absorb(q);
        }
        epilogue(t);
      }
      zero_acc();
      seg0 = u + 1;
      ++t;
      ks = 0;
    } else {
      ++ks;
    }
  }
}

template <typename K_>
int launch_sk(const GemmP& p0, bool conv, void* ws, hipStream_t st) {
  GemmP p = p0;
  SkP s;
  s.kt = p.K / 64;
  s.tiles = p.tiles_m * p.tiles_n;
  s.units = s.tiles * s.kt;
  const int G = sk_grid(p);
  s.flags = (uint32_t*)ws;
  s.part = (float*)((char*)ws + SK_FLAG_BYTES);
  dim3 grid(G);
  const bool rowld = p.R1 || p.R2 || p.pos || p.accumulate;
#define DP_SK(C_, R_, L_) hipLaunchKernelGGL((gemm_sk_kernel<K_, C_, R_, L_>), grid, dim3(512), 0, st, p, s)
  if (rowld) {
    if (conv && p.relu_a) DP_SK(true, true, true);
    else if (conv) DP_SK(true, false, true);
    else if (p.relu_a) DP_SK(false, true, true);
    else DP_SK(false, false, true);
  } else {
    if (conv && p.relu_a) DP_SK(true, true, false);
    else if (conv) DP_SK(true, false, false);
    else if (p.relu_a) DP_SK(false, true, false);
    else DP_SK(false, false, false);
  }
#undef DP_SK
  DP_CHECK_LAUNCH();
  return 0;
}

}  // namespace

namespace dpg {
int launch_part_sk(const GemmP& p, bool conv, void* ws, bool bf16, hipStream_t s) {
  return (bf16 ? launch_sk<KBF16>(p, conv, ws, s) : launch_sk<KF16>(p, conv, ws, s));
}
}  // namespace dpg
