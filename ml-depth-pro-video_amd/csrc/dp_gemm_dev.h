#pragma once
// dp_gemm_dev.h -- device basics of the dp_gemm engines (dp_gemm_*.hip, dp_gemm_big.h).
//
// LDS rows are 128 B (64 x 16-bit) with the 16-B chunk index XOR-swizzled by (row & 7) ->
// conflict-free ds_read_b128 fragment reads (lds_off, lds_off_t).  Operands stream global -> LDS
// directly with global_load_lds_dwordx4 (glds16*: no VGPR staging), and the waits are counted
// (`s_waitcnt vmcnt(N)` + raw `s_barrier`, never a full drain in a K loop).  The MFMA
// v_mfma_f32_16x16x32_{bf16,f16} is issued with the weight fragment as its A-operand and the
// activation fragment as B, so D = C^T: each lane ends up with 4 consecutive output channels of one
// output row, and bias / gamma / residual loads and the stores are 8-16 B per lane.  Block ids are
// remapped so that the blocks one XCD runs are a contiguous range of tiles (tile_coords).

#include "dp_gemm_impl.h"

#include <type_traits>

namespace {

#ifdef DP_STAMPS
// Timing-only builds (make stamps): per-workgroup s_memrealtime (100 MHz) stamps
// [start, first tile visible, main loop done, end, hw_id | xcc_id << 32].
__device__ unsigned long long g_stamps[5 * 65536];
#define DP_STAMP(v)                                                                   \
  do {                                                                                \
    __builtin_amdgcn_sched_barrier(0);                                                \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory");    \
    __builtin_amdgcn_sched_barrier(0);                                                \
  } while (0)
#define DP_STAMPS_DECL unsigned long long st0_ = 0, st1_ = 0, st2_ = 0, st3_ = 0
#define DP_STAMP_SAVE(wg)                                                             \
  do {                                                                                \
    if (threadIdx.x == 0 && (wg) < 65536) {                                           \
      unsigned hw_, xcc_;                                                             \
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_));              \
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_));            \
      unsigned long long* d_ = g_stamps + 5 * (wg);                                   \
      d_[0] = st0_; d_[1] = st1_; d_[2] = st2_; d_[3] = st3_;                         \
      d_[4] = hw_ | ((unsigned long long)xcc_ << 32);                                 \
    }                                                                                 \
  } while (0)
#else
#define DP_STAMP(v) do { } while (0)
#define DP_STAMPS_DECL
#define DP_STAMP_SAVE(wg) do { } while (0)
#endif

// 256 zero bytes: source of the implicit-conv zero padding for LDS-DMA loads and of the
// persistent engine's absent column constants
__device__ __attribute__((aligned(16))) uint32_t g_zero_page[64];

__device__ __forceinline__ int lds_off(int row, int chunk) {  // element offset, 64-wide rows
  return row * BK + ((chunk ^ (row & 7)) << 3);
}

// Tile order within the XCD-contiguous workgroup ranges.  Row-major (tile_n fastest)
// puts the 32 workgroups an XCD runs at once on ~2 rows of tiles x all columns;
// with BAND > 1 they sweep bands of BAND tile rows column by column instead, so the
// tiles in flight on one XCD form a squarer block (e.g. 4 x 8) that shares fewer
// distinct A / B panels in its 4 MiB L2: qkv 155 -> 150 us, fc1 197 -> 190 us
// (tools/gemm_bench.py --dbg 16 restores row-major, for A/B).
__device__ __forceinline__ void tile_coords(const GemmP& p, int wgid, int& tile_m, int& tile_n) {
  // debug 16: row-major; 1 << 18: bands of 8 rows; 1 << 19: bands of 2 rows (A/B)
  const int band = (p.dbg & DBG_ROW_MAJOR_TILES) ? 1 : (p.dbg & DBG_BAND8) ? 8 : (p.dbg & DBG_BAND2) ? 2 : 4;
  const int tm_full = p.tiles_m / band * band;       // rows covered by whole bands
  const int per_band = band * p.tiles_n;
  if (band > 1 && wgid < tm_full * p.tiles_n) {
    const int b = wgid / per_band, r = wgid - b * per_band;
    tile_n = r / band;
    tile_m = b * band + (r - tile_n * band);
  } else {
    tile_n = wgid % p.tiles_n;
    tile_m = wgid / p.tiles_n;
  }
}

// implicit-conv row descriptor: output pixel m -> top-left input tap
struct ConvRow {
  int iy, ix, pix;
};
__device__ __forceinline__ ConvRow conv_row(const GemmP& p, int m) {
  ConvRow r;
  const bool ok = m < p.M;
  const int mc = ok ? m : p.M - 1;
  const int hw = p.out_h * p.out_w;
  const int b = mc / hw, rr = mc - b * hw;
  const int oy = rr / p.out_w, ox = rr - oy * p.out_w;
  r.iy = ok ? oy * p.stride - p.pad : -(1 << 28);
  r.ix = ox * p.stride - p.pad;
  r.pix = b * p.in_h * p.in_w;
  return r;
}
__device__ __forceinline__ const u16* conv_src(const GemmP& p, const ConvRow& r, int ky, int kx, int ci, bool& inb) {
  const int iy = r.iy + ky, ix = r.ix + kx;
  inb = (unsigned)iy < (unsigned)p.in_h && (unsigned)ix < (unsigned)p.in_w;
  const long long pix = (long long)r.pix + (long long)iy * p.in_w + ix;
  return p.A + pix * p.in_c + ci;
}

// Implicit-conv K order: k = ((cb * k_h + ky) * k_w + kx) * 64 + c -- the taps of one
// 64-channel block are consecutive K steps, so the shifted re-reads of the same input
// lines by neighbouring taps are one K step apart and hit in L2 (with the channel block
// innermost, the re-read came 4-36 steps later, after the XCD's 32 workgroups had
// streamed several MiB through the 4 MiB L2).  Weights are packed to match
// ([Cout][Cin/64][ky][kx][64], ops.conv_weight).  k0 % 32 == 0.
__device__ __forceinline__ void conv_tap(const GemmP& p, int k0, int& ky, int& kx, int& ci) {
  const int chunk = k0 >> 6, c = k0 & 63;
  const int taps = p.k_h * p.k_w;
  const int cb = chunk / taps, tap = chunk - cb * taps;
  ky = tap / p.k_w;
  kx = tap - ky * p.k_w;
  ci = cb * 64 + c;
}

// workgroup size of the 8-wave engines
constexpr int NT_BIG = 512;

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}
// One 16-B-per-lane LDS-DMA piece (1 KiB per wave) written at the wave-uniform
// LDS byte address `lds_dst`.  Issued from inline asm so the compiler does not
// add its conservative `s_waitcnt vmcnt(0)` in front of every later ds_read:
// completion is tracked by hand with the counted waits below.
__device__ __forceinline__ void glds16(const void* src, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(src), "s"(lds_dst)
      : "memory");
}

// The same with a wave-uniform 64-bit base in SGPRs and a 32-bit per-lane byte offset (saddr form):
// a K step's addresses are one scalar add away from the last step's, no per-lane 64-bit arithmetic.
__device__ __forceinline__ void glds16s(uint32_t voff, const void* sbase, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_dst)
      : "memory");
}

// The same through a buffer resource (4 SGPRs: base, num_records = bytes, raw): a lane whose byte
// offset is past the buffer's end reads zeros -- the implicit conv's zero padding without a second
// (zero page) address per lane.
__device__ __forceinline__ void glds16b(uint32_t voff, u32x4_t rsrc, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
      "buffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(rsrc), "s"(lds_dst)
      : "memory");
}
// Raw buffer resource of `bytes` bytes at p (stride 0): the SGPR words of glds16b's rsrc.
__device__ __forceinline__ u32x4_t raw_rsrc(const void* p, uint32_t bytes) {
  const unsigned long long a = (unsigned long long)(uintptr_t)p;
  u32x4_t r;
  r.x = __builtin_amdgcn_readfirstlane((uint32_t)a);
  r.y = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32) & 0xffffu);
  r.z = __builtin_amdgcn_readfirstlane(bytes);
  r.w = 0x00020000u;
  return r;
}

// LDS image of one operand tile: rows of BKT 16-bit elements (64 or 128 B), the
// 16-B chunk index XOR-swizzled so that the 16 rows one ds_read_b128 lane group
// reads hit 16 distinct bank slots (conflict-free, checked with SQ_LDS_BANK_CONFLICT).
template <int BKT>
__device__ __forceinline__ int lds_off_t(int row, int chunk) {
  if constexpr (BKT == 64) return row * 64 + ((chunk ^ (row & 7)) << 3);
  else return row * 32 + ((chunk ^ ((row >> 1) & 3)) << 3);
}

template <int N>
__device__ __forceinline__ void wait_vmcnt_le(int n) {  // s_waitcnt vmcnt(n), n <= N, n a multiple of step
  if constexpr (N == 0) {
    wait_vmcnt<0>();
  } else {
    if (n >= N) wait_vmcnt<N>();
    else wait_vmcnt_le<N - 1>(n);
  }
}

}  // namespace
