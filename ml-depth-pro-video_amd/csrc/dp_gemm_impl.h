#pragma once
// dp_gemm_impl.h -- the host-side core of dp_gemm (bf16 / f16 MFMA GEMM with an implicit-conv A
// loader and a fused epilogue, gfx950): what more than one translation unit needs on the host.
// GemmP (the planned launch), the DBG_* bits, TILES[] (the engines by DP_TILE_*), the launch_part_*
// entry of every engine family, the workspace layout and the host's choice of epilogue
// (needs_rowld, fast_epi_act).  No device code: dp_gemm.hip (argument checks, the planner, the C
// ABI) includes this header and dp_ln_merge.h only.
//
// Where the rest is:
//   dp_gemm_dev.h       device basics every engine uses: LDS swizzle, LDS-DMA (glds16*), counted
//                       waits, the tile raster, the implicit-conv addressing, the DP_STAMP* macros
//   dp_gemm_epilogue.h  the epilogues several engines share: epilogue_rows, epilogue_mfma,
//                       epilogue_acc32, head_ps_rows
//   dp_gemm_big.h       gemm_big_kernel + launch_big: the big-tile engine, instantiated by
//                       dp_gemm_big.hip, dp_gemm_big320.hip, dp_gemm_splitk.hip and (launch_dual)
//                       dp_gemm_small.hip
//   dp_ln_merge.h       ln_merge_row, the folded-LayerNorm row merge (dp_gemm.hip's
//                       ln_merge_kernel and dp_gemm_8ph320.hip's ln_merge_last)
// and one engine per file, kernel, private epilogue and launcher together:
//   dp_gemm_pbig.hip    persistent big engine (gemm_pbig_kernel)
//   dp_gemm_8ph.hip     8-phase 256 x 256 engine and its persistent form (gemm_8ph_kernel,
//                       gemm_p8ph_kernel)
//   dp_gemm_8ph320.hip  8-phase 320 x 256 engine with the folded-LayerNorm epilogues
//                       (gemm_8ph320_kernel)
//   dp_gemm_sk.hip      stream-K engine (gemm_sk_kernel)
//   dp_gemm_splitk.hip  split-K: the big engine over K ranges + splitk_reduce_kernel
//   dp_gemm_small.hip   register-staged small tiles (gemm_kernel) and the 2-workgroup-per-CU
//                       launch of the big engine (launch_dual)
//   dp_gemm_cv3.hip     3x3 patch-conv engine

#include "dp_common.h"

#include <atomic>

namespace dpg {

constexpr int BK = 64;
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));

constexpr int DP_MAX_GROUPS = 4;   // dp_gemm_grouped

struct GemmP {
  int M, N, K;
  const u16* A;
  long long lda;
  const u16* B;
  long long ldb;
  int relu_a;
  int in_h, in_w, in_c, k_h, k_w, stride, pad, out_h, out_w;
  const float* bias;
  int act;
  const float* gamma;
  const float* pos;
  long long ldpos;
  int pos_group, pos_off;
  const u16* R1;
  long long ldr1;
  const u16* R2;
  long long ldr2;
  void* C;
  long long ldc;
  int c_dtype;
  int accumulate;
  int store_mode;
  int dc_h, dc_w, dc_cout;
  int row_group, row_group_out, row_off;
  const float* head_w;
  float head_b;
  const float* head_corr;
  int tiles_n, tiles_m;
  int dbg;  // ablation / A-B bits (DBG_* below)
  unsigned c_bytes;  // persistent engine: byte extent of C from p.C (buffer-store bound)
  // LayerNorm folded across the GEMM boundary (dp_gemm_args.ln_*; the 8-phase 320 x 256 engine)
  float* ln_part_out;      // producer: (mean, M2) per 128-column chunk of the new C rows
  u16* ln_xb_out;          // producer: the new C rows in 16 bits ([M][ldc])
  u16* ln_xl;              // producer on a split residual (hi = ln_xb_out, lo = ln_xl; read + written)
  const float* ln_part_in; // consumer: the A rows' chunk statistics ([M][K/128][2])
  const float* ln_colsum;  // consumer: sum_k B[n][k]
  float ln_eps;
  const float* ln_rs;      // consumer on the persistent 8-phase engine: per row (rstd, -rstd * mean),
                           // merged from ln_part_in by ln_merge_kernel into the GEMM workspace, or
                           // the producer's ln_rs_out (ABI 13)
  float* ln_rs_out;        // split producer: the last workgroup of each row tile merges its rows
  unsigned* ln_cnt;        // ... counting the tile's arrivals here (workspace words LN_CNT_WORD ..)
  // dp_gemm_grouped: `groups` problems of one shape in one launch (workgroup range g * tiles_m *
  // tiles_n ... covers problem g, whose operand pointers are grp[g]); 1 otherwise
  int groups;
  // split-K (DP_TILE_SPLITK_256x256): workgroup range s * tiles ... covers K-steps [s KT / ksplit,
  // (s+1) KT / ksplit) of every tile and stores raw fp32 partials into kpart + s M N; a reduce
  // launch adds them and runs the epilogue; 1 otherwise
  int ksplit;
  float* kpart;
  struct Group {
    const u16* A;
    const u16* B;
    const float* bias;
    const float* gamma;
    const float* pos;
    const u16* R1;
    const u16* R2;
    void* C;
    // the grouped folded-LN forms (dp_gemm_grouped): producer outputs / consumer inputs of problem g
    float* ln_part_out;
    u16* ln_xb_out;
    const float* ln_part_in;
    const float* ln_colsum;
  } grp[DP_MAX_GROUPS];
};

// Process-wide ablation / fault-injection bits (dp_gemm.hip), set only by dp_gemm_debug_flags
// (tools and tests; not in the ABI header).  Read once per dp_gemm call.
extern std::atomic<int> g_dbg_flags;
// The bits (GemmP::dbg).  Tools and tests pass the integers; every reader uses these names.
enum : int {
  DBG_NO_EPILOGUE = 1,              // kernels skip the epilogue (tools/gemm_bench.py --ablate, head_bench.py, hilo_bench.py)
  DBG_NO_LOOP_LOADS = 2,            // big engine: no loads in the K loop (tools/gemm_bench.py --ablate)
  DBG_NO_MFMA = 4,                  // big engine: no MFMAs in the K loop (tools/gemm_bench.py --ablate)
  DBG_ROW_MAJOR_TILES = 16,         // tile_coords: row-major instead of 4-row bands (tools/gemm_bench.py --dbg 16)
  DBG_NO_SMALL_STREAMK = 32,        // planner + sk_grid: no stream-K K split for small conv grids (tools/frame_shapes.py --dbg 32)
  DBG_SK_GIVE_UP = 64,              // stream-K: a waiting workgroup gives up at once (tests: the sticky error word)
  DBG_NO_PBIG = 1024,               // planner: no persistent 320 x 256 / 256 x 256 upgrade (DP_GEMM_DEBUG, tools/ab_bench.sh)
  DBG_PBIG_DENSE = 2048,            // planner: the persistent upgrade for dense (ViT) GEMMs too (DP_GEMM_DEBUG, tools/ab_bench.sh)
  DBG_NO_CV3_HEAD = 4096,           // planner: the N = 128 head conv on the 512 x 128 engine (tests/test_abi.py, tools/head_bench.py)
  DBG_FC1_BIG320 = 8192,            // planner: the 8-phase choice (fc1) -> 320 x 256 (tools/fc1_bench.py, tests/test_bench_cli.py)
  DBG_FC1_BIG256 = 16384,           // planner: the 8-phase choice (fc1) -> 256 x 256 (tools/fc1_bench.py)
  DBG_NO_8PH320 = 1 << 15,          // planner: no 8-phase 320 x 256 upgrade (DP_GEMM_DEBUG, tools/ab_bench.sh)
  DBG_NO_CV3 = 1 << 16,             // planner: no patch-conv upgrade of the 3x3 convs (DP_GEMM_DEBUG, tools/ab_bench.sh)
  DBG_BAND8 = 1 << 18,              // tile_coords: bands of 8 tile rows (tools/p8ph_stamps.py)
  DBG_BAND2 = 1 << 19,              // tile_coords: bands of 2 tile rows (tools/p8ph_stamps.py)
  DBG_NO_FAST_EPILOGUE = 1 << 20,   // no load-free epilogues, so no P8PH / 8PH_320x256 engine (DP_GEMM_DEBUG, tools/ab_bench.sh)
  DBG_NO_P8PH = 1 << 22,            // planner: no persistent upgrade of the 8-phase engine (DP_GEMM_DEBUG, tools/ab_bench.sh)
  DBG_NO_P8PH_DECONV = 1 << 23,     // planner: the deconvs not on the persistent 8-phase engine (tests/test_abi.py)
  DBG_CV3_ABLATION = 1 << 24,       // launch_cv3: bits 0..10 select a K-loop ablation / stamp variant (tools/cv3_stamps.py)
  DBG_LNC_8PH320 = 1 << 25,         // planner: folded-LN consumers on the 320 x 256 engine (DP_GEMM_DEBUG, tools/ab_bench.sh)
  DBG_HILO_AHEAD1 = 1 << 27,        // split-residual producer: the one-chunk-ahead epilogue (tools/hilo_bench.py, tests/test_gpu_kernels.py)
};
constexpr int DBG_CV3_ABLATION_MASK = 2047;   // the variant number under DBG_CV3_ABLATION
// CU count of the current device (cached, dp_gemm.hip)
int num_cus();

// The engines by DP_TILE_* value: tile rows x columns, the family (translation unit) that launches
// it, whether the grid is capped at the CU count (persistent workgroups), and whether the epilogue
// works on 8-column chunks (dp_mi355x.h: the 8-column rules).
enum TileFamily { FAM_NONE, FAM_SMALL, FAM_BIG, FAM_BIG320, FAM_8PH, FAM_8PH320, FAM_PBIG, FAM_SK, FAM_SPLITK, FAM_CV3 };
struct TileInfo {
  int bm, bn;
  TileFamily fam;
  bool cu_capped, col8;
};
constexpr TileInfo TILES[] = {
    {0, 0, FAM_NONE, false, false},        // DP_TILE_AUTO
    {128, 128, FAM_SMALL, false, false},   // DP_TILE_128x128
    {256, 64, FAM_SMALL, false, false},    // DP_TILE_256x64
    {256, 32, FAM_SMALL, false, false},    // DP_TILE_256x32
    {256, 256, FAM_BIG, false, true},      // DP_TILE_BIG_256x256
    {256, 128, FAM_BIG, false, true},      // DP_TILE_BIG_256x128
    {256, 256, FAM_BIG, false, true},      // DP_TILE_BIG_256x256_K32
    {256, 128, FAM_BIG, false, true},      // DP_TILE_BIG_256x128_K32
    {256, 256, FAM_8PH, false, true},      // DP_TILE_8PH_256x256
    {256, 256, FAM_BIG, false, true},      // DP_TILE_DEEP4_256x256
    {256, 256, FAM_BIG, false, true},      // DP_TILE_DEEP5_256x256
    {256, 128, FAM_BIG, false, true},      // DP_TILE_DEEP_256x128
    {256, 256, FAM_SK, false, true},       // DP_TILE_STREAMK_256x256 (grid: sk_grid)
    {320, 256, FAM_BIG320, false, true},   // DP_TILE_BIG_320x256
    {512, 128, FAM_BIG320, false, true},   // DP_TILE_BIG_512x128
    {320, 256, FAM_PBIG, true, true},      // DP_TILE_PBIG_320x256
    {256, 256, FAM_PBIG, true, true},      // DP_TILE_PBIG_256x256
    {256, 128, FAM_SMALL, false, true},    // DP_TILE_DUAL_256x128
    {256, 256, FAM_8PH, true, true},       // DP_TILE_P8PH_256x256
    {320, 256, FAM_8PH320, false, true},   // DP_TILE_8PH_320x256
    {256, 256, FAM_CV3, false, true},      // DP_TILE_CV3_256x256 (16 x 16 pixels)
    {256, 256, FAM_SPLITK, false, true},   // DP_TILE_SPLITK_256x256 (grid: x the K split)
    {192, 256, FAM_CV3, false, true},      // DP_TILE_CV3_192x256 (12 x 16 pixels)
    {384, 128, FAM_CV3, false, true},      // DP_TILE_CV3_384x128 (24 x 16 pixels)
};
constexpr int N_TILES = sizeof(TILES) / sizeof(TILES[0]);
static_assert(N_TILES == 24 && DP_TILE_CV3_384x128 == N_TILES - 1, "one entry per DP_TILE_*");
// (a hint outside the enum plans and runs as DP_TILE_BIG_256x256, the big engine's default instantiation)
inline const TileInfo& tile_info(int tile) { return TILES[tile >= 0 && tile < N_TILES ? tile : DP_TILE_BIG_256x256]; }

// Engine families, one translation unit each: launch `p` (planned by dp_gemm.hip) on `tile`.
int launch_part_big(const GemmP& p, int tile, bool conv, bool bf16, hipStream_t s);      // dp_gemm_big.hip
constexpr int TILE_GRP_128x128 = -1;   // internal: the grouped (side-encoder) launches' 128 x 128 big tile
int launch_part_big320(const GemmP& p, int tile, bool conv, bool bf16, hipStream_t s);   // dp_gemm_big320.hip
int launch_part_8ph(const GemmP& p, int tile, bool conv, bool bf16, hipStream_t s);      // dp_gemm_8ph.hip
int launch_part_8ph320(const GemmP& p, bool conv, bool bf16, hipStream_t s);             // dp_gemm_8ph320.hip
int launch_part_cv3(const GemmP& p, bool conv, bool bf16, hipStream_t s, int th = 16);                // dp_gemm_cv3.hip
int launch_part_pbig(const GemmP& p, int tile, bool conv, bool bf16, hipStream_t s);     // dp_gemm_pbig.hip
int launch_part_small(const GemmP& p, int tile, bool conv, bool bf16, hipStream_t s);    // dp_gemm_small.hip
int launch_part_sk(const GemmP& p, bool conv, void* ws, bool bf16, hipStream_t s);       // dp_gemm_sk.hip
int launch_part_splitk(const GemmP& p, bool conv, bool bf16, hipStream_t s);             // dp_gemm_splitk.hip
}  // namespace dpg

namespace {
using namespace dpg;

// Fewer tiles than CUs (the decoder's 48^2 - 192^2 convs: 9 - 144 tiles of 256 x 256,
// 36 - 144 k-steps): the K range of every tile is split over up to SK_MAX_SPLIT
// workgroups of >= SK_MIN_STEPS k-steps each (the owner adds the others' fp32
// partials, 256 KiB apiece), or, at more than half a chip of tiles, spread over
// every CU.  debug flag 32 restores one workgroup per tile.
constexpr int SK_MIN_STEPS = 8, SK_MAX_SPLIT = 6;
int sk_grid(const GemmP& p) {
  const int tiles = p.tiles_m * p.tiles_n;
  int g = num_cus();
  if (g > 256) g = 256;   // == SK_MAX_WG (workspace slots)
  if (tiles >= g) return g;
  if (p.dbg & DBG_NO_SMALL_STREAMK) return tiles;
  const int kt = p.K / 64;
  int s = g / tiles;
  if (s < 2) return kt >= 2 * SK_MIN_STEPS ? g : tiles;
  if (s > SK_MAX_SPLIT) s = SK_MAX_SPLIT;
  if (s > kt / SK_MIN_STEPS) s = kt / SK_MIN_STEPS;
  return tiles * (s < 1 ? 1 : s);
}

// GEMM workspace layout (dp_gemm_workspace_size, dp_gemm.hip): the stream-K engine's hand-off
// flags and partial slots (dp_gemm_sk.hip) and the split producer's row-tile counters
// (dp_gemm_8ph320.hip)
constexpr int SK_TILE_F = 256 * 256;             // floats per partial slot
constexpr long long SK_FLAG_BYTES = 4096;        // flags [0, G) (each reset by its consumer), error word at [1023] (sticky)
constexpr int LN_CNT_WORD = 512;                 // the split producer's row-tile counters: words [512, 1023)
static_assert(DP_GEMM_WS_ERROR_OFFSET == 4 * 1023, "error word offset (dp_mi355x.h)");
constexpr int SK_MAX_WG = 256;

// Epilogue variants.  needs_rowld: the launch reads per-row operands (R1 / R2, pos, the fp32 C
// it accumulates into) or stores through a remap (deconv pixel shuffle, row groups, the fused /
// composed heads).  Without any of those (and with a 16-bit C) the engines take the load-free
// epilogue_mfma (dp_gemm_epilogue.h): no loads at all, so the compiler needs no `s_waitcnt vmcnt(0)` between
// row batches (in the general epilogue a runtime-conditional load in a batch makes it wait for
// every older VMEM op, i.e. for the previous batches' stores: the epilogue serialised on store
// latency, fc1 221.6 -> 211.2 us and qkv 146.3 -> 135.1 us without it).
__host__ __device__ inline bool needs_rowld(const GemmP& p) {
  return p.R1 || p.R2 || p.pos || p.accumulate || p.store_mode != DP_STORE_ROWS || p.row_group || p.head_corr ||
         p.head_w;
}

// EACT of the engine variants: the compile-time epilogue.  -1: the general, runtime one;
// DP_ACT_*: epilogue_mfma (no per-row operand, 16-bit C); EPI_ACC + DP_ACT_*: epilogue_acc32
// (fp32 C accumulated into, no other per-row operand); EPI_LNP / EPI_LNC + DP_ACT_*: below.
constexpr int EPI_ACC = 16;
// the grouped 128 x 128 launches' folded-LN epilogues (dp_gemm_big.h): EPI_LNP = the producer
// (epilogue_acc32 + 16-bit rows + chunk statistics), EPI_LNC + DP_ACT_* = the consumer (epilogue_mfma
// with the rows' mean / rstd applied)
constexpr int EPI_LNP = 32, EPI_LNC = 48;
__host__ inline int fast_epi_act(const GemmP& p) {
  if (p.dbg & DBG_NO_FAST_EPILOGUE) return -1;
  if (!needs_rowld(p)) return p.c_dtype == DP_F32 ? -1 : p.act;
  const bool acc_only = p.accumulate && p.c_dtype == DP_F32 && !p.R1 && !p.R2 && !p.pos &&
                        p.store_mode == DP_STORE_ROWS && !p.row_group && !p.head_corr && !p.head_w;
  return acc_only ? EPI_ACC + p.act : -1;
}

}  // namespace
