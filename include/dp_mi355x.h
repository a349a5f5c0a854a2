/*
 * dp_mi355x.h -- C ABI of the MI355X-native Depth Pro hot path (libdp_mi355x.so).
 *
 * The reference (tdj28/ml-depth-pro-video) has no native code: its hot path
 * `DepthPro.infer` (src/depth_pro/depth_pro.py:243-298) dispatches PyTorch and
 * timm ops.  Each entry point below replaces a group of those ops; the comment
 * on each one cites the reference code it stands in for.  The binding the
 * reference-side would add (ctypes) is shown in INTEGRATION.md.
 *
 * Conventions (all entry points):
 *   - plain device pointers (HBM), sizes and a HIP stream (hipStream_t passed as
 *     an opaque pointer; NULL = legacy default stream);
 *   - no allocation, no host<->device copies, no synchronisation, so every call
 *     is hipGraph-capturable; the caller owns all buffers;
 *   - return 0 on success, a hipError_t value (< 1000) if a launch failed, or a
 *     DP_ERR_* code (>= 1000) for an argument/shape error detected on the host
 *     before anything was launched;
 *   - 16-bit tensors are raw bits (uint16) whose kind is given by a DP_BF16 /
 *     DP_F16 dtype argument; fp32 tensors are `float`.
 *   - safe for concurrent calls from several host threads on distinct streams: the
 *     library's only process-wide state is a per-device CU-count cache (written once,
 *     same value from every writer) and the debug/fault-injection word of the
 *     tools-only `dp_gemm_debug_flags` (not declared here), which must not change
 *     while other threads launch.
 */
#ifndef DP_MI355X_H
#define DP_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dp_stream_t;

enum { DP_BF16 = 0, DP_F16 = 1, DP_F32 = 2 };
enum { DP_OK = 0, DP_ERR_ARG = 1000, DP_ERR_SHAPE = 1001, DP_ERR_ALIGN = 1002, DP_ERR_DTYPE = 1003 };
enum { DP_ACT_NONE = 0, DP_ACT_RELU = 1, DP_ACT_GELU = 2 };
enum { DP_A_DENSE = 0, DP_A_CONV = 1 };
enum { DP_STORE_ROWS = 0, DP_STORE_DECONV2X2 = 1, DP_STORE_HEAD_PS = 2 };

/* ABI version of this header; the Python loader refuses a mismatching .so. */
#define DP_ABI_VERSION 20
int dp_abi_version(void);

/*
 * dp_gemm: C = epilogue(A . B^T), bf16/f16 MFMA (v_mfma_f32_16x16x32_*), fp32 accumulate.
 *
 * Replaces every Linear / Conv2d / ConvTranspose2d(k2 s2) of the hot path:
 *   timm ViT qkv / proj / fc1 / fc2 Linears and the k16 s16 patch-embed conv
 *     (vit_factory.py:97-99; DINOv2 Block), fov.encoder.1 Linear (fov.py:45-47);
 *   encoder 1x1 projections + k2s2 deconvs + fuse_lowres (encoder.py:60-130, 314-324);
 *   decoder 3x3 convs, residual blocks, deconv+out_conv (decoder.py:54-206);
 *   depth head (depth_pro.py:182-207) and FOV convs (fov.py:28-54, 75-82).
 *
 * A operand: DP_A_DENSE  -> A[m][k] row-major, leading dim lda (elements);
 *            DP_A_CONV   -> implicit im2col of an NHWC tensor [batch][in_h][in_w][in_c]
 *                           for a k_h x k_w conv (stride, pad) with output out_h x out_w;
 *                           M = batch*out_h*out_w, K = k_h*k_w*in_c,
 *                           k = ((ci/64 * k_h + ky) * k_w + kx) * 64 + ci%64 (the taps of one
 *                           64-channel block are consecutive: shifted input re-reads hit L2).
 * B operand: packed weights B[n][k] row-major (ldb), i.e. W for a Linear,
 *            [Cout][Cin/64][ky][kx][64] for a conv, [(dy,dx,Cout)][Cin] for a k2s2 deconv.
 * Requirements: K % 64 == 0, N % 4 == 0 (DP_ERR_SHAPE), lda/ldb % 8 == 0 (DP_ERR_ALIGN),
 *   in_c % 64 == 0 (conv).  Any M >= 1; any conv geometry with M = batch*out_h*out_w.
 * Alignment of the epilogue operands (DP_ERR_ALIGN; elements; a rule applies only where the operand
 *   is used): every epilogue reads and writes 4 consecutive columns at row*ld + n in one 8- or
 *   16-byte access, so on every engine
 *     ldc % 4 == 0 (16-bit and fp32 C; no ldc with the fused head / DP_STORE_HEAD_PS),
 *     ldr1 % 4 == 0, ldr2 % 4 == 0, ldpos % 4 == 0, dc_cout % 4 == 0 (DP_ERR_SHAPE),
 *   and the pointers C, R1, R2, pos, bias, gamma, head_w aligned to 4 of their elements (A, B: 8).
 *   The 8-column engines (every DP_TILE_* from DP_TILE_BIG_256x256 = 4 up, below) work on 8
 *   consecutive columns (16-byte accesses to 16-bit rows, one deconv sub-pixel per 8 columns):
 *     N % 8 == 0 and, with DP_STORE_DECONV2X2, dc_cout % 8 == 0      (DP_ERR_SHAPE), then
 *     ldr1 % 8 == 0, ldr2 % 8 == 0, and ldc % 8 == 0 for a 16-bit C  (DP_ERR_ALIGN; those
 *     pointers aligned to 8 elements)
 *   (an fp32 C and pos keep the % 4 rule).  Under DP_TILE_AUTO a problem that does not meet the
 *   8-column rules runs on the 4-column engines (DP_TILE_128x128 for N > 64); with a hint for an
 *   8-column engine it is the error named above.
 *
 * Epilogue, per element, in this order:
 *   v = acc (+ bias[n]) ; act(v) ; (* gamma[n]) ; (+ pos[(m % pos_group) + pos_off][n])
 *   (+ R1[m][n]) (+ R2[m][n]) ; (+ C[m][n] when accumulate) ; store
 * Store:   DP_STORE_ROWS      -> C[row(m)][n], row(m) = m, or grouped remap
 *                                (m / row_group) * row_group_out + row_off + m % row_group;
 *          DP_STORE_DECONV2X2 -> pixel shuffle: m = (b, y, x) on a dc_h x dc_w grid,
 *                                n = (dy*2+dx)*dc_cout + co  ->  out pixel (b, 2y+dy, 2x+dx),
 *                                address C + pixel*ldc + co.
 * Fused 1x1 head (head_w != NULL; requires N <= 32): out[m] = relu(sum_n v[n]*head_w[n] + head_b)
 *   written as fp32 to C[m] (the depth head tail, depth_pro.py:200-204).
 * DP_STORE_HEAD_PS (depth head deconv + conv3x3 + ReLU + 1x1 + ReLU, depth_pro.py:182-207, composed
 *   at pack time into ONE 3x3 implicit conv over the pre-upsampling map): A_CONV over [out_h][out_w]
 *   pixels, N = 128 columns = (parity q = 2*dy+dx, channel o < 32); per output pixel
 *   (2y+dy, 2x+dx) of the 2*out_h x 2*out_w fp32 map C:
 *   relu(sum_o head_w[o] * relu(v[q*32+o] - border(q, y, x, o)) + head_b), where border() sums
 *   head_corr[(a*3+c)*32 + o] over the taps (a, c) of the 3x3 kernel that fall outside the
 *   upsampled image (the deconv bias those zero-padded taps must not carry).
 *   Compact form (no new field: recognised from the call): with a 3x3 / stride 1 / pad 1 geometry,
 *   K == 4*in_c instead of 9*in_c means B = [q = 4][o = 32][j = 4][in_c] (ldb >= 4*in_c): parity q's
 *   weights at its 2 x 2 taps (ty, tx) = (dy + j/2, dx + j%2) only -- the other five taps of a
 *   composed head are zero by construction (the k2 s2 deconv under a 3x3 conv reaches two h0 rows
 *   and two h0 columns per parity).  Same result as the dense form on the patch-conv engine, bit
 *   for bit, in 4/9 of its K steps.  Runs on DP_TILE_CV3_256x256 / DP_TILE_CV3_384x128 only (the
 *   auto choice: 384x128 when the side % 48 == 0, else 256x256); a shape those cannot take (side
 *   % 16 != 0, relu_a, M * in_c >= 2^30) or any other hint is DP_ERR_ARG -- the dense weights are
 *   a different buffer, so there is no fallback.  bias, head_w, head_b, head_corr ([9][32]) are
 *   those of the dense form.
 */
typedef struct dp_gemm_args {
  int32_t M, N, K;
  int32_t dtype;            /* DP_BF16 | DP_F16 : element kind of A, B, R1, R2 */
  const void* A;
  int64_t lda;
  const void* B;
  int64_t ldb;
  int32_t a_mode;           /* DP_A_DENSE | DP_A_CONV */
  int32_t relu_a;           /* apply ReLU to A elements as they are loaded */
  int32_t in_h, in_w, in_c, k_h, k_w, stride, pad, out_h, out_w;  /* conv geometry */
  const float* bias;        /* [N] or NULL */
  int32_t act;              /* DP_ACT_* */
  const float* gamma;       /* [N] or NULL (LayerScale) */
  const float* pos;         /* fp32 [*][ldpos] or NULL */
  int64_t ldpos;
  int32_t pos_group, pos_off;
  const void* R1;           /* residuals, same element kind, or NULL */
  int64_t ldr1;
  const void* R2;
  int64_t ldr2;
  void* C;
  int64_t ldc;
  int32_t c_dtype;          /* DP_BF16 | DP_F16 | DP_F32 */
  int32_t accumulate;       /* C += v (fp32 C only) */
  int32_t store_mode;       /* DP_STORE_* */
  int32_t dc_h, dc_w, dc_cout;
  int32_t row_group, row_group_out, row_off;
  const float* head_w;      /* [N] or NULL */
  float head_b;
  const float* head_corr;   /* DP_STORE_HEAD_PS: [9][32] border corrections; DP_STORE_ROWS with a
                               stride-1 pad-1 3x3 implicit conv on the 512x128 or the patch-conv
                               engine (N = 128 at M >= 512*256, or those tile hints): [9][N]
                               per-tap values subtracted where the tap falls in the zero padding
                               (a composed 1x1-then-3x3 conv's bias); else NULL */
  int32_t tile;             /* 0 = auto, else a DP_TILE_* hint */
  void* workspace;          /* NULL, or >= dp_gemm_workspace_size() bytes of device memory owned by
                               the caller for THIS stream (never shared by concurrent launches);
                               enables the persistent stream-K engine for large 256x256-tiled GEMMs */
  int64_t workspace_bytes;
  /* LayerNorm folded across the GEMM boundary (timm Block norm1 / norm2, eps ln_eps), dense A,
   * the 8-phase 320 x 256 engine (DP_TILE_8PH_320x256; NULL fields: off):
   *  producer -- the residual GEMM (accumulate into fp32 C, act none) also writes
   *    ln_xb_out:   the new rows of C in 16 bits (dtype), [M][ldc];
   *    ln_part_out: fp32 [M][N/128][2]: (mean, M2) of each 128-column chunk of the new rows;
   *  consumer -- A = a producer's ln_xb_out (un-normalised rows), B = W o ln.weight (per k)
   *    [o gamma (per n)], bias = (b + W . ln.bias) [* gamma], gamma = NULL,
   *    ln_part_in = the producer's ln_part_out ([M][K/128][2]), ln_colsum[N] = sum_k B[n][k]
   *    (the 16-bit values, summed exactly); the epilogue's value before act is
   *      v = rstd * acc - rstd * mean * ln_colsum[n] + bias[n]
   *    with (mean, rstd) of the row merged from its K/128 chunks: LN(x) . W^T + b exactly, up
   *    to where the 16-bit rounding falls (x instead of LN(x)).
   *  producer on a SPLIT residual (ABI 12, ln_xl != NULL): the residual stream is held as a 16-bit
   *    high part (ln_xb_out, dtype, [M][ldc]) and an int8 low part (ln_xl, [M][ldc] bytes), read and
   *    updated in place:  x = hi + q * 2^(e - S)  with e the frexp exponent of hi (hi = m 2^e,
   *    m in [0.5, 1)), S = 16 (bf16) / 19 (f16), i.e. q counts steps of ulp(hi) / 256 for a
   *    normal hi;
   *    x' = v + x, v = (acc + bias[n]) * gamma[n];  hi' = x' rounded to 16 bits (nearest even);
   *    q' = clamp(rint((x' - hi') 2^(S - e')), -128, 127), e' the frexp exponent of hi': half a
   *    step of error, 1.5 steps at the one clamped value (the exact tie x' - hi' = +ulp(hi') / 2
   *    gives 128).  Edges: hi = 0 has e = 0 and q = 0.  A subnormal f16 hi (|hi| < 2^-14) keeps
   *    its frexp exponent, so its step 2^(e - 19) is finer than ulp(hi) / 256 = 2^-32 and
   *    |x - hi| <= 2^-25 can be up to 2^(-6 - e) >= 256 steps: q then saturates at -128 / 127
   *    and the error is bounded by the 16-bit rounding's 2^-25 instead of half a step.  An f16
   *    hi' of +-inf (|x'| >= 65520) is stored as such with q' = -128 / 127, and the element
   *    stays +-inf from then on (the fp32 C, when given, still receives the finite x')
   *    (~16 significant bits: the patch encoder's error vs fp32 moves 2.3788e-3 -> 2.3809e-3,
   *    tools/hilo_emul.py); ln_part_out as above or NULL; C (fp32, [M][ldc]) is not read: NULL, or
   *    written with x' (for a reader of the fp32 rows); accumulate = 1, act none, ldc % 8 == 0,
   *    M * ldc * 4 < 2^32 - 256.  6 instead of 10 bytes of HBM traffic per element in a residual
   *    GEMM's epilogue.
   *  What a launch with an ln_* field must meet (DP_ERR_ARG otherwise; checked right after the
   *  general checks -- where accumulate with a 16-bit C is DP_ERR_DTYPE -- and before the 8-column
   *  rules, which apply to every ln_* launch whatever the hint: ldc % 8 == 0 for a 16-bit C):
   *    every ln_* launch: what DP_TILE_8PH_320x256 takes (dense A, no relu_a, N % 256 == 0,
   *      DP_STORE_ROWS, no R1 / R2 / pos / row groups / head, M * lda and N * ldb below 2^31);
   *      a tile hint other than DP_TILE_AUTO and DP_TILE_8PH_320x256 is DP_ERR_ARG, except
   *      DP_TILE_P8PH_256x256 on a consumer; no producer field together with a consumer field;
   *    fp32 producer (ln_xl NULL): ln_part_out and ln_xb_out both, C fp32 and accumulated into,
   *      act none;
   *    split producer: ln_xb_out, accumulate = 1 and c_dtype DP_F32 (also when C is NULL), act
   *      none, ldc % 8 == 0, the extent limit above;
   *    consumer: ln_colsum and exactly one of ln_part_in / ln_rs_in, K == 1024, ln_eps > 0 (0,
   *      negative and NaN are refused), act none or GELU, gamma NULL, a 16-bit C, no accumulate.
   *      It runs on the 8-phase 320 x 256 engine, or on the persistent 8-phase engine where the
   *      planner or a DP_TILE_P8PH_256x256 hint puts it and its merged row statistics have a
   *      place: ln_rs_in, or ln_part_in with a workspace and M <= 32768.  An ln_part_in consumer
   *      hinted DP_TILE_P8PH_256x256 without those runs on the 320 x 256 engine -- the one hint
   *      that is rerouted rather than refused (both engines compute the same contract); a
   *      problem the persistent engine does not take at all stays DP_ERR_ARG under the hint. */
  float* ln_part_out;
  void* ln_xb_out;
  const float* ln_part_in;
  const float* ln_colsum;
  float ln_eps;
  void* ln_xl;
  /* ABI 13: the row statistics merged by the producer (the persistent consumer's merge pre-pass
   * folded into the split-residual producer): with ln_rs_out set (split producer, N == 1024,
   * ln_part_out set, a workspace), the last workgroup to finish each row tile merges the tile's
   * rows' 8 chunk statistics into ln_rs_out[m] = (rstd, -rstd * mean) (eps ln_eps; the arithmetic
   * of the pre-pass, bit for bit); a consumer on the persistent 8-phase engine takes ln_rs_in =
   * that array instead of ln_part_in (no pre-pass launch, no workspace needed).  ln_rs_in holds
   * M rounded up to an even number of rows (its reads go in row pairs; the pad row's values are
   * never used).  ln_rs_out needs (DP_ERR_ARG): ln_xl, ln_part_out, N == 1024, ln_eps > 0, a
   * workspace of dp_gemm_workspace_size() bytes, and ceil(M / 320) <= 511, i.e. M <= 163520 (one
   * counter per row tile, workspace words 512 .. 1022; each is zero again when the launch ends).
   * ln_rs_in runs only on the persistent engine: DP_TILE_AUTO and DP_TILE_P8PH_256x256 both mean
   * that engine, at every M; any other hint is DP_ERR_ARG. */
  float* ln_rs_out;
  const float* ln_rs_in;
} dp_gemm_args;

enum { DP_TILE_AUTO = 0, DP_TILE_128x128 = 1, DP_TILE_256x64 = 2, DP_TILE_256x32 = 3,
       DP_TILE_BIG_256x256 = 4, DP_TILE_BIG_256x128 = 5, DP_TILE_BIG_256x256_K32 = 6,
       DP_TILE_BIG_256x128_K32 = 7, DP_TILE_8PH_256x256 = 8, DP_TILE_DEEP4_256x256 = 9,
       DP_TILE_DEEP5_256x256 = 10, DP_TILE_DEEP_256x128 = 11, DP_TILE_STREAMK_256x256 = 12,
       DP_TILE_BIG_320x256 = 13, DP_TILE_BIG_512x128 = 14, DP_TILE_PBIG_320x256 = 15,
       DP_TILE_PBIG_256x256 = 16, DP_TILE_DUAL_256x128 = 17,
       DP_TILE_P8PH_256x256 = 18, DP_TILE_8PH_320x256 = 19, DP_TILE_CV3_256x256 = 20,
       DP_TILE_SPLITK_256x256 = 21, DP_TILE_CV3_192x256 = 22, DP_TILE_CV3_384x128 = 23 };
/* What a tile hint accepts.  DP_TILE_AUTO never fails for a problem the contract above allows.  The
   checks run in this order; the first that fails gives the return code:
   1. the general argument checks (above), for every hint;
   2. the fused 1x1 head (head_w with DP_STORE_ROWS) always runs on DP_TILE_256x32 and
      DP_STORE_HEAD_PS on a 128-column conv engine (the hint is kept only if it is
      DP_TILE_BIG_256x128, DP_TILE_CV3_256x256 or DP_TILE_CV3_384x128): other hints are ignored,
      not rejected -- except for the compact form (K == 4*in_c), which only the two DP_TILE_CV3_*
      engines walk: any other hint is DP_ERR_ARG;
   3. hints 1 - 3 (DP_TILE_128x128, 256x64, 256x32: the 4-column engines) take everything else
      except head_corr (DP_ERR_ARG);
   4. every hint >= DP_TILE_BIG_256x256: the 8-column rules (DP_ERR_SHAPE, then DP_ERR_ALIGN);
   5. then per engine (DP_ERR_ARG unless noted):
      - DP_TILE_BIG_* / DEEP* / DUAL / 8PH_256x256 (4 - 11, 13, 14, 17): nothing more (dense and
        conv A, every epilogue operand and store mode); head_corr with DP_STORE_ROWS only on
        DP_TILE_BIG_512x128 (and the CV3 engines);
      - DP_TILE_STREAMK_256x256: a workspace, N % 256 == 0;
      - DP_TILE_SPLITK_256x256: a workspace, N % 256 == 0, DP_STORE_ROWS without row groups; then
        DP_ERR_SHAPE unless min(CUs / tiles, (K / 64) / 2, (workspace_bytes - 4096) / (4 M N), 32)
        >= 2, tiles = ceil(M / 256) * (N / 256);
      - DP_TILE_PBIG_320x256 / PBIG_256x256: N % 256 == 0, DP_STORE_ROWS (row groups allowed), the
        byte extent of C below 2^32 - 256, M * lda and N * ldb below 2^31;
      - DP_TILE_P8PH_256x256: dense A, N % 256 == 0, K >= 128, a 16-bit C, no R1 / R2 / pos /
        accumulate / row groups, the same extent limits, and DP_STORE_ROWS, or DP_STORE_DECONV2X2
        without relu_a / act / gamma and with dc_w >= 8;
      - DP_TILE_8PH_320x256: dense A, no relu_a, N % 256 == 0, DP_STORE_ROWS, no R1 / R2 / pos /
        row groups, M * lda and N * ldb below 2^31, and either a 16-bit C (not accumulated) or an
        fp32 C accumulated into without activation;
      - DP_TILE_CV3_*: a stride-1 pad-1 3x3 conv over square maps (in = out side S, S % 16 == 0;
        S % 48 == 0 for 192x256 and 384x128), no gamma / pos / accumulate / row groups / GELU,
        M * in_c < 2^30; a 16-bit C with N % 256 == 0 (N % 128 == 0 with head_corr, then no
        R1 / R2), or DP_STORE_HEAD_PS; 192x256 without head_corr; 384x128 only with head_corr or
        DP_STORE_HEAD_PS at N == 128.
   DP_TILE_P8PH_256x256: persistent 8-phase engine (min(tiles, CUs) workgroups, each a stream of
   K steps over its tiles; dense A, N % 256 == 0, K >= 128, 16-bit C without per-row operands);
   the auto choice for the ViT fc1.  DP_TILE_8PH_320x256: 8-phase 320 x 256 engine (dense A, no
   ReLU prologue, N % 256 == 0; 16-bit C without per-row operands, or an fp32 C accumulated into
   without activation); the auto choice for the ViT qkv / proj / fc2.  A hint an engine cannot
   serve returns DP_ERR_ARG.  DP_TILE_CV3_256x256: stride-1 pad-1 3x3 implicit conv on 16 x 16 pixel
   tiles with the input patch in LDS (square maps, side % 16 == 0, in_c % 64 == 0; N % 256 == 0 with
   ReLU / residual epilogues, or N % 128 == 0 with head_corr, or DP_STORE_HEAD_PS); the auto choice
   for the many-round ResidualBlock convs and the border-corrected composed conv at 768^2.
   DP_TILE_CV3_192x256: the same engine on 12 x 16-pixel tiles (side % 48 == 0, N % 256 == 0, the
   ReLU / residual epilogues): the auto choice where those tiles make whole rounds of workgroups and
   16 x 16 ones do not (the 384^2 ResidualBlock convs and projection: 768 tiles = 3 rounds).
   DP_TILE_CV3_384x128 (ABI 14): the same engine on 24 x 16-pixel tiles of 128 output channels
   (side % 48 == 0, N == 128, with head_corr: the border-corrected composed conv, or
   DP_STORE_HEAD_PS): the auto choice for the former (out_conv∘head.0 at 768^2: 1536 tiles =
   6 rounds); a hint for the dense composed depth head, whose auto choice stays the 512 x 128
   engine, and the auto choice for its compact form (K == 4*in_c, above).
   DP_TILE_SPLITK_256x256 (ABI 11, a hint only, needs a workspace): split-K for small grids -- the
   256 x 256 tiles' K steps split over up to (CUs / tiles) workgroups that write fp32 partials into
   the workspace, then a reduce launch sums them in split order and runs the epilogue
   (DP_STORE_ROWS, no row groups / head); DP_ERR_SHAPE when no split of >= 2 fits.
   Sizes: the 8-phase 320 x 256 engine, the persistent engines (P8PH, PBIG) and the patch-conv
   engine keep 32-bit element offsets from the A / B bases, so they serve M * lda and N * ldb
   below 2^31 only; past that the planner takes the 64-bit-pointer engines and a hint for one
   of those returns DP_ERR_ARG. */

int dp_gemm(const dp_gemm_args* args, dp_stream_t stream);

/*
 * dp_gemm_grouped: `groups` (1..4) dp_gemm problems in ONE launch.  args[0..groups-1] must agree
 * in every field but the operand pointers A, B, bias, gamma, pos, R1, R2 and C (dense A, row
 * stores, no fused head); each problem gives exactly the result its own dp_gemm call would
 * (the 256 x 128 big engine; the tile hint is ignored).  Replaces the image encoder's and the FOV
 * encoder's ViT Linears / patch embeds -- two ViT-L with their own weights over the same x2 input
 * (encoder.py:308-311, fov.py:66-72) -- run side by side as one workgroup range per problem.
 *
 * Folded LayerNorm with groups >= 2 (additive; ABI 20): two forms of the ln_* fields, with
 * ln_part_out / ln_xb_out / ln_part_in / ln_colsum per problem (all problems set the same ones) and
 * the meaning they have in dp_gemm_args:
 *   producer (the side proj / fc2): ln_part_out and ln_xb_out both, C fp32 and accumulated into,
 *     act NONE, N % 128 == 0, no R1 / R2 / pos / row_group.  C is what the launch without ln_*
 *     writes, bit for bit; ln_xb_out[m][ldc] = those fp32 values rounded to dtype;
 *     ln_part_out[m][N/128][2] = (mean, M2) of each 128-column chunk of them.
 *   consumer (the side qkv / fc1): ln_part_in and ln_colsum both, K == 1024, a 16-bit C with
 *     ldc % 8 == 0, act NONE or GELU, no gamma (a per-column scale is folded into B / bias /
 *     ln_colsum), ln_eps > 0 and equal in every problem, no accumulate / R1 / R2 / pos / row_group:
 *     v = rstd * acc - rstd * mean * ln_colsum[n] + bias[n], then act.
 * Any other ln_* field or combination in a grouped call (ln_xl, ln_rs_out, ln_rs_in, K != 1024 for
 * a consumer, N % 128 != 0 for a producer, ...) is DP_ERR_ARG.  groups == 1 is dp_gemm, with its rules.
 */
int dp_gemm_grouped(const dp_gemm_args* args, int32_t groups, dp_stream_t stream);

/*
 * Bytes of workspace the stream-K engine needs (flags + one fp32 256x256 partial
 * tile per persistent workgroup).  The caller zeroes it once after allocation; every
 * hand-off flag a stream-K launch sets is reset by the workgroup that consumes it, so
 * the flags are zero again whenever a launch ends (no per-launch clearing, nothing but
 * kernels touches it -- graph-replay safe), the rest is scratch -- except the ERROR WORD: the
 * uint32 at byte offset DP_GEMM_WS_ERROR_OFFSET becomes non-zero when a stream-K
 * launch on this workspace gave up waiting for another workgroup's partial tile
 * (bounded spin; the output of that launch is then wrong).  It is sticky: nothing
 * but the caller clears it, so one read after a whole forward / graph replay covers
 * every launch in it.  After a timeout the flags may be left set: zero the first 1 KiB
 * (or the whole workspace) before reusing it.
 */
#define DP_GEMM_WS_ERROR_OFFSET 4092
int64_t dp_gemm_workspace_size(void);

/*
 * dp_gemm_workspace_check: for the end of a forward (after every launch on `workspace`):
 * *status (device int32) = the sticky error word; if it is set, the error word and every
 * hand-off flag are zeroed, so the next forward starts clean and its own status reflects only
 * its own launches.  One tiny kernel, graph-capturable.  (Reference: none -- the per-frame
 * failure detection of SURVEY.md section 5 replacing the reference's per-frame try/except,
 * generate_depth_maps.py:147-151.)
 */
int dp_gemm_workspace_check(void* workspace, int32_t* status, dp_stream_t stream);

/*
 * Which engine / tile and how many workgroups dp_gemm would launch for `args`
 * (no launch): *tile receives a DP_TILE_* value (DP_TILE_STREAMK_256x256 for the
 * persistent engine), *grid the workgroup count.  For tests and the bench.
 */
int dp_gemm_plan(const dp_gemm_args* args, int32_t* tile, int32_t* grid);

/*
 * dp_layernorm: y[r] = LN(x[r]) * w + b over `cols`, fp32 in, 16-bit out.
 * Replaces timm Block norm1/norm2 and the final `norm` (eps 1e-6).
 * cols: 256, 512, 1024 or 2048; ldx % 4 == 0, ldy % 4 == 0 (% 8 above 256 columns).  x, w and b
 * must be 16-B aligned, y 8-B aligned at 256 columns and 16-B aligned above (DP_ERR_ALIGN).
 */
int dp_layernorm(const float* x, int64_t ldx, const float* w, const float* b, void* y, int64_t ldy,
                 int32_t rows, int32_t cols, float eps, int32_t dtype, dp_stream_t stream);

/*
 * dp_layernorm_stats: the input side of a folded LayerNorm (dp_gemm_args.ln_*): for the rows of
 * fp32 x [rows][cols] (cols: 512, 1024 or 2048) write x in 16 bits (xb [rows][ldxb], dtype) and
 * part fp32 [rows][cols/128][2] = (mean, M2) of each 128-column chunk -- what the residual GEMMs'
 * producer epilogue writes, for the rows no GEMM produced (the patch embed + cls rows that enter
 * ViT block 0).  xl (ABI 12; NULL: none): the int8 low part of the split residual ([rows][ldxb]
 * bytes, the encoding of dp_gemm_args.ln_xl), so that (xb, xl) is the stream a split-residual
 * producer reads.  ldx % 4 == 0, ldxb % 8 == 0; x and xb must be 16-B aligned, xl and part 8-B
 * aligned (DP_ERR_ALIGN).  Checks, in this order: x, xb or part NULL (DP_ERR_ARG); rows <= 0
 * (DP_ERR_SHAPE); ldx, ldxb, then the pointers (DP_ERR_ALIGN); cols not one of the three
 * (DP_ERR_SHAPE); dtype not DP_BF16 / DP_F16 (DP_ERR_DTYPE).
 */
int dp_layernorm_stats(const float* x, int64_t ldx, int32_t rows, int32_t cols, void* xb, int64_t ldxb,
                       void* xl, float* part, int32_t dtype, dp_stream_t stream);

/*
 * dp_layernorm_grouped: dp_layernorm over groups * rows_per_group rows, rows of group g taking
 * w[g] / b[g] (w, b: HOST arrays of `groups` (1..4) device pointers) -- the image and FOV
 * encoders' norm1 / norm2 / final norm in one launch.  Alignment as dp_layernorm, for x, y and
 * every w[g] / b[g].
 */
int dp_layernorm_grouped(const float* x, int64_t ldx, const float* const* w, const float* const* b,
                         int32_t groups, void* y, int64_t ldy, int32_t rows_per_group, int32_t cols,
                         float eps, int32_t dtype, dp_stream_t stream);

/*
 * dp_attention: multi-head softmax attention, flash-style (no S x S in HBM).
 * qkv: [batch*seq][3*heads*head_dim] (timm's qkv Linear output, (3, heads, hd) column order);
 * out: [batch*seq][heads*head_dim] (timm's transpose(1,2).reshape). head_dim must be 64.
 * Replaces timm Attention's F.scaled_dot_product_attention (scale = head_dim^-0.5).
 * out = softmax(scale * Q K^T) V per (image, head); scale must be finite and >= 0 (DP_ERR_ARG;
 * 0 gives the mean of V).  qkv and out must be 16-B aligned (DP_ERR_ALIGN); the launch has
 * ceil(seq / 128) * heads * batch workgroups, which must stay below 2^31 (DP_ERR_SHAPE).
 */
int dp_attention(const void* qkv, void* out, int32_t batch, int32_t seq, int32_t heads,
                 int32_t head_dim, float scale, int32_t dtype, dp_stream_t stream);

/*
 * dp_attention_log2q: dp_attention for a qkv whose Q columns already hold
 * Q * scale * log2(e) -- folded into the qkv Linear's epilogue as a per-column gamma --
 * so the scores leave the MFMA in log2 units and the softmax needs one exp2 per score.
 * Same result as dp_attention up to where the scale is rounded (before the 16-bit Q); the same
 * alignment and size rules.
 */
int dp_attention_log2q(const void* qkv, void* out, int32_t batch, int32_t seq, int32_t heads,
                       int32_t head_dim, int32_t dtype, dp_stream_t stream);

/*
 * dp_normalize_u8: uint8 HWC image -> (x/255 - 0.5)/0.5 planar CHW (fp32 or 16-bit).
 * The value is computed in fp32 (IEEE division); a 16-bit output is that fp32 value rounded to
 * nearest even.  Replaces the transform Compose (depth_pro.py:125-132) with the u8 upload + GPU normalize.
 */
int dp_normalize_u8(const uint8_t* img_hwc, int32_t H, int32_t W, void* out_chw, int32_t out_dtype,
                    dp_stream_t stream);

/*
 * dp_resize_bilinear: planar C x H x W (fp32 or 16-bit) -> C x OH x OW fp32,
 * bilinear, align_corners=False, no antialias, optional scalar pre-multiply
 * (F.interpolate as used by DepthPro.infer, depth_pro.py:271-279 and 288-291).
 */
int dp_resize_bilinear(const void* src, int32_t src_dtype, int32_t C, int32_t H, int32_t W,
                       float* dst, int32_t OH, int32_t OW, dp_stream_t stream);

/*
 * dp_resize: dp_resize_bilinear with the F.interpolate mode DepthPro.infer passes through
 * (`interpolation_mode`, depth_pro.py:243-279): DP_INTERP_BILINEAR, or DP_INTERP_BICUBIC
 * (upsample_bicubic2d, align_corners=False, A = -0.75, border taps clamped).
 * Same size in and out (H == OH and W == OW) is a copy in either mode, at any element alignment
 * of src and dst: every value, a NaN or an infinity included, arrives unchanged (a 16-bit source
 * upcast exactly) and touches no neighbour.
 */
enum { DP_INTERP_BILINEAR = 0, DP_INTERP_BICUBIC = 1 };
int dp_resize(const void* src, int32_t src_dtype, int32_t C, int32_t H, int32_t W, float* dst,
              int32_t OH, int32_t OW, int32_t mode, dp_stream_t stream);

/*
 * dp_patchify_pyramid: 1536^2 planar fp32 image -> im2col rows of the 35 sliding
 * windows [35*576][768] (k = c*256 + ky*16 + kx), building the 768^2 and 384^2
 * pyramid levels on the fly (the bilinear 0.5 / 0.25 resizes are exact 2x2 box
 * averages).  Replaces _create_pyramid + split + cat (encoder.py:151-188, 245-263)
 * and the patch-embed unfold.  Window 34 (384^2 level) is also the image-encoder
 * and FOV-encoder input (encoder.py:308-311, fov.py:66-72).
 */
int dp_patchify_pyramid(const float* x0, void* cols, int32_t dtype, dp_stream_t stream);

/*
 * dp_vit_cls_rows: x[w*577] = cls + pos[0] for w < n_images (timm _pos_embed cls row),
 * x fp32 [n_images*577][1024].
 */
int dp_vit_cls_rows(float* x, const float* cls, const float* pos, int32_t n_images, dp_stream_t stream);

/*
 * dp_merge_windows: stitch steps x steps token windows into an NHWC map, dropping the
 * cls token and cropping `padding` tokens at inner edges (encoder.py:190-231).
 * src rows: window w token t at row (w*577 + t), ld_src elements, fp32 or 16-bit;
 * dst: [S][S][1024] 16-bit with S = steps*24 - 2*padding*(steps-1).
 */
int dp_merge_windows(const void* src, int32_t src_dtype, int64_t ld_src, int32_t first_window,
                     int32_t steps, int32_t padding, void* dst, int32_t dtype, dp_stream_t stream);

/*
 * dp_merge_windows_range: dp_merge_windows restricted to the windows w_lo <= w < w_hi of the
 * steps x steps grid (w = row * steps + column); the other pixels of dst are not written.
 * For a patch encoder run as several independent window groups (each merges its own share
 * of a hooked block's output before it moves on).
 * Both calls reject, before any launch: ld_src % 8 != 0, steps > 1 with 24 - 2 * padding <= 0,
 * w_lo >= w_hi, w_lo < 0 or w_hi > steps * steps (DP_ERR_SHAPE); a 16-bit source of the other
 * 16-bit kind than `dtype`, or a `dtype` that is not 16-bit (DP_ERR_DTYPE).  steps == 1 ignores
 * `padding`.
 */
int dp_merge_windows_range(const void* src, int32_t src_dtype, int64_t ld_src, int32_t first_window,
                           int32_t steps, int32_t padding, int32_t w_lo, int32_t w_hi, void* dst,
                           int32_t dtype, dp_stream_t stream);

/*
 * dp_fov_tail: final FOV conv 6x6 (32 -> 1) + bias on the 6x6x32 NHWC map
 * (fov.py:46, head[4]).  w is the PyTorch weight [1][32][6][6] fp32.
 */
int dp_fov_tail(const void* x6, int32_t dtype, const float* w, float bias, float* fov_deg,
                dp_stream_t stream);

/*
 * dp_infer_epilogue (depth_pro.py:282-298):
 *   f_px = use_given ? f_given : 0.5*W / tan(0.5*deg2rad(fov_deg))   (fp32)
 *   inv  = canonical * scale, scale = use_given ? (float)(W / f_given) : W / f_px
 *   inv  = bilinear(inv, (H, W)) when (H, W) != (1536, 1536)
 *   depth = 1 / clamp(inv, 1e-4, 1e4)   (a NaN stays NaN, as torch.clamp)  -> depth [H][W] fp32
 * f_px_out (device float) receives f_px.  nonfinite (optional device int32): incremented by the
 * number of NaN / inf values written (depth and f_px) -- a per-frame health word the frame loops
 * read back before writing a frame's files.
 */
int dp_infer_epilogue(const float* canonical, int32_t src_h, int32_t src_w, const float* fov_deg,
                      int32_t use_given, double f_given, int32_t H, int32_t W, float* depth,
                      float* f_px_out, int32_t* nonfinite, dp_stream_t stream);

/* dp_infer_epilogue_mode: the same with the resize back to (H, W) in `mode` (DP_INTERP_*,
 * depth_pro.py:288-291 passes interpolation_mode). */
int dp_infer_epilogue_mode(const float* canonical, int32_t src_h, int32_t src_w, const float* fov_deg,
                           int32_t use_given, double f_given, int32_t H, int32_t W, float* depth,
                           float* f_px_out, int32_t* nonfinite, int32_t mode, dp_stream_t stream);

/*
 * dp_resize_u8_cv: cv2.resize of an 8-bit HWC 3-channel frame to OH x OW -- the reference's
 * --downscale_factor (generate_depth_maps.py:95-110: INTER_AREA for factor < 1, INTER_LINEAR
 * otherwise, new size int(H * factor) x int(W * factor)).  OpenCV 4.x's published fixed-point
 * bilinear (11-bit coefficients) and area-averaging rules, restated in oracle/cv_resize_oracle.py
 * (parity unpinned vs a cv2 binary: none is available).
 */
enum { DP_CV_INTER_LINEAR = 1, DP_CV_INTER_AREA = 3 };   /* cv2's constants */
int dp_resize_u8_cv(const uint8_t* src, int32_t H, int32_t W, uint8_t* dst, int32_t OH, int32_t OW,
                    int32_t interpolation, dp_stream_t stream);

/*
 * dp_depth_to_points: camera-space point cloud of a depth map -- the reference's
 * depth_to_3d (img_to_normalized_pointcloud.py:819-856), used before its PLY write-out
 * (:1318).  valid = !isnan(depth) && depth > 0, points in row-major pixel order (numpy
 * boolean indexing), fp64 as numpy computes them:
 *   x = -1*(u - W/2)*z/f, y = -1*(v - H/2)*z/f, z = depth      (f = f_px if use_given,
 *   else (double)*f_px_dev, e.g. dp_infer_epilogue's f_px_out).
 * row_offsets: int32 [H+1] scratch; receives the exclusive prefix of valid counts per row
 * and the total in row_offsets[H].  xyz: fp64 [H*W][3] (capacity); rgb_out (optional):
 * uint8 [H*W][3] colours gathered from rgb_hwc (uint8 [H][W][3]) at the same pixels.
 */
int dp_depth_to_points(const float* depth, int32_t H, int32_t W, const float* f_px_dev, double f_px,
                       int32_t use_given, const uint8_t* rgb_hwc, int32_t* row_offsets, double* xyz,
                       uint8_t* rgb_out, dp_stream_t stream);

/*
 * dp_depth_to_image: the frame loop's depth writers on the GPU (generate_depth_maps.py:15-44
 * colorize_depth, :135-143 --raw): nanmin / nanmax of depth[n] into minmax (2 x uint32 scratch,
 * order-preserving keys), then per pixel v = (d - min) / (max - min) in fp32 and
 *   DP_DEPTH_IMG_COLOR: out uint8 [n][3] = lut[trunc(clip(v, 0, 1) * N)] (N -> N - 1; NaN -> entry
 *     N + 2, matplotlib's "bad"); lut uint8 [(N + 3)][3] = (colormap lut * 255).astype(uint8);
 *   DP_DEPTH_IMG_RAW16: out uint16 [n] = (uint16)(v * 65535) (NaN -> 0).
 * Byte-identical to the reference's numpy / matplotlib arithmetic.
 */
enum { DP_DEPTH_IMG_COLOR = 0, DP_DEPTH_IMG_RAW16 = 1 };
int dp_depth_to_image(const float* depth, int64_t n, uint32_t* minmax, const uint8_t* lut, int32_t lut_n,
                      int32_t mode, void* out, dp_stream_t stream);

/*
 * ---- Ground-normalised point clouds (ABI 15, csrc/dp_ground.hip) ---------------------------------
 * The first stage of the reference's 3-D pipeline after depth_to_3d: ground-plane fit, levelling
 * and per-cell adjustment (img_to_normalized_pointcloud.py:601-816, :880-981, :983-1118).  All fp64,
 * each product and sum rounded on its own (no FMA) as numpy's ufuncs do; all on the caller's
 * stream, no synchronisation and no host read-back.
 *
 * Common conventions of every entry below:
 *   points     fp64 [n_max][3] device rows (x, y, z), as dp_depth_to_points writes them.
 *   n_dev      device int32: the first *n_dev rows are live (clamped to [0, n_max]); NULL: n_max.
 *              n_max < 2^31.  n_max = 0 (or *n_dev = 0) is valid: no point is touched, counts are 0.
 *   workspace  >= dp_ground_workspace_size(n_max) bytes of device memory, 8-byte aligned, owned by
 *              the call until the stream has passed it (its content need not be initialised).
 *   A point with a NaN or +-inf coordinate belongs to no segment anywhere, is counted in the
 *   "non-finite" output and is copied to points_out unchanged.  (The reference is undefined for
 *   such points -- its np.min / np.percentile would propagate them; this behaviour is ours.)
 */
#define DP_GROUND_MAX_SEG 1024   /* segments of one selection (32 x 32 grid cells) */
#define DP_GROUND_MAX_GRID 32    /* grid_size of the trace and of the adjustment */
int64_t dp_ground_workspace_size(int64_t n_max);

/*
 * dp_seg_select: order statistic of fp64 keys per segment (np.percentile / the k-th smallest of
 * np.partition), the primitive under every stage below.  keys[i * key_stride] (i < n) is the key of
 * element i, seg[i] in [0, n_seg) its segment, any other id (-1) "in no segment"; n_seg <= 1024.
 * Keys must not be NaN; -0.0 counts (and is returned) as +0.0.
 *   mode DP_SEL_PERCENTILE: values_out[s] = np.percentile(keys of s, param) with method="linear":
 *     v = (count - 1) * (param / 100), a, b = the floor(v)-th and next smallest, t = v - floor(v),
 *     a + (b - a) * t, replaced by b - (b - a) * (1 - t) where t >= 0.5 (numpy's _lerp).
 *   mode DP_SEL_KTH: values_out[s] = the k-th smallest key (1-based),
 *     k = min(count, max(kmin, (int)(param * count))) -- derived on the device from the count.
 * A segment takes part only if count > min_count (and count > 0); otherwise values_out[s] = NaN.
 * counts_out[s] (int32) = keys in segment s, always.  Selection is by most-significant-digit radix
 * passes (8 bits) over per-(segment, digit) histograms of order-preserving 64-bit keys; nothing is
 * sorted, and any number of equal keys costs the same.
 */
enum { DP_SEL_PERCENTILE = 0, DP_SEL_KTH = 1 };
int dp_seg_select(const double* keys, int64_t key_stride, const int32_t* seg, const int32_t* n_dev,
                  int32_t n_max, int32_t n_seg, int32_t mode, double param, int32_t kmin, int32_t min_count,
                  int32_t* counts_out, double* values_out, void* workspace, int64_t workspace_bytes,
                  dp_stream_t stream);

/*
 * dp_ground_trace: the ground trace of grid_based_ground_plane_fit with initial_ground_model=None
 * (img_to_normalized_pointcloud.py:629-700): z min / max, bin_edges = np.linspace(z_min, z_max,
 * grid_size + 1), bin = np.digitize(z, bin_edges) - 1 (so z == z_max falls outside every bin, as
 * in the reference); each bin with more than 10 points contributes the mean of its
 * max(1, int(0.05 * count)) lowest-y points, ties at the cut taken in index order.
 *   trace_out  fp64 [grid_size][4]: mean x, y, z and the bin's point count
 *   valid_out  int32 [grid_size]: 1 where the bin contributed
 *   info_out   fp64 [4]: finite points, non-finite points, z_min, z_max
 * grid_size <= 32.
 */
int dp_ground_trace(const double* points, const int32_t* n_dev, int32_t n_max, int32_t grid_size,
                    double* trace_out, int32_t* valid_out, double* info_out, void* workspace,
                    int64_t workspace_bytes, dp_stream_t stream);

/*
 * dp_ground_lowest: the fit's fallback trace (:702-707): the max(10, int(0.05 * count)) lowest-y
 * finite points (all of them if there are fewer), ties at the cut in index order.
 *   points_out fp64 [capacity][3], index_out int32 [capacity]: the selected points and their row
 *              indices, in no particular order (sort by index for the reference's order up to ties);
 *              capacity >= max(10, int(0.05 * n_max)) holds them all, extra ones are dropped.
 *   info_out   fp64 [2]: number selected, finite points
 */
int dp_ground_lowest(const double* points, const int32_t* n_dev, int32_t n_max, double* points_out,
                     int32_t* index_out, int32_t capacity, double* info_out, void* workspace,
                     int64_t workspace_bytes, dp_stream_t stream);

/*
 * dp_ground_dist_percentile: the fit's "push the plane down" inputs (:771-784): signed distances
 * dist = x*n0 + y*n1 + z*n2 + d of the finite points to plane = {n0, n1, n2, d} (host pointer),
 * their np.percentile(q) and the number below the plane.
 *   out fp64 [4]: percentile (NaN without points), points with dist < 0, finite points, non-finite
 */
int dp_ground_dist_percentile(const double* points, const int32_t* n_dev, int32_t n_max, const double* plane,
                              double q, double* out, void* workspace, int64_t workspace_bytes,
                              dp_stream_t stream);

/*
 * dp_ground_normalize: normalize_point_cloud_to_ground (:880-981).  model (host pointer, fp64 [15]):
 *   [0..2] unit normal, [3] d  (dist = p . n + d, point_plane_distances :858-878)
 *   [4..12] R row-major, [13] const, [14] rotate flag -- R (Rodrigues, :917-934) and
 *   const = -d / (R n)[1] are the caller's fp64 host values; flag 0 is the reference's
 *   |n . y| > 0.99 branch: the points are copied, R and const unused.
 * Per finite point p' = R p, y' -= const; ground level = np.percentile(y' of the points with
 * |dist| < 0.1, 2), subtracted only if there are more than 10 such points; then ground points
 * (|dist| < 0.05) with y' < 0 go to 0 and the others with y' < -0.1 go to -0.1.
 *   points_out fp64 [n_max][3] (must not alias points)
 *   stats_out  fp64 [8]: finite points, non-finite points, points with |dist| < 0.1, ground level
 *              (0 if not taken), level taken (0 / 1), ground points, set to 0, limited to -0.1
 *              (the last three are the reference's printed counts)
 */
int dp_ground_normalize(const double* points, double* points_out, const int32_t* n_dev, int32_t n_max,
                        const double* model, double* stats_out, void* workspace, int64_t workspace_bytes,
                        dp_stream_t stream);

/*
 * dp_ground_adjust: grid_based_ground_adjustment (:983-1118).  x / z min and max, np.linspace edges
 * (start + i * step, last edge = stop), cell = clip(digitize - 1) per axis, x_idx * grid_size +
 * z_idx.  A cell is adjusted if it has >= 10 points, >= 5 of them with y < 0.2, and
 * p = np.percentile(those y, percentile) > 0.01; its points then lose p (y < 0.1),
 * p * (1 - (y - 0.1) / 1.4) (0.1 <= y < 1.5) or nothing, and are clamped at 0.
 *   points_out fp64 [n_max][3] (must not alias points); grid_size <= 32
 *   stats_out  fp64 [8]: finite points, non-finite points, non-empty cells, cells with >= 10 points,
 *              cells adjusted, points adjusted (the reference's four summary numbers), 0, 0
 */
int dp_ground_adjust(const double* points, double* points_out, const int32_t* n_dev, int32_t n_max,
                     int32_t grid_size, double percentile, double* stats_out, void* workspace,
                     int64_t workspace_bytes, dp_stream_t stream);

/*
 * ---- Cleaned point clouds (ABI 16, csrc/dp_clean.hip) --------------------------------------------
 * The second stage of the reference's 3-D pipeline (pointcloud_pipeline.py, process_single_frame
 * step 2): remove_stray_points then clean_shadows (pointcloud_cleaner.py:142-207, :209-309), on a
 * stable device radix sort of (key, index) pairs, plus the order-preserving compaction between and
 * after them.  The ground section's conventions hold throughout: fp64 points [n_max][3], n_dev a
 * device int32 (NULL: n_max; clamped to [0, n_max]), n_max = 0 and *n_dev = 0 valid, everything on
 * the caller's stream with no synchronisation and no host read-back, each fp64 product and sum
 * rounded on its own (no FMA), argument errors returned as DP_ERR_* before any launch.
 *   workspace  >= dp_clean_workspace_size(n_max) bytes of device memory, 8-byte aligned, owned by
 *              the call until the stream has passed it (content need not be initialised).  About
 *              48 bytes per point + 1 KiB per 4096 points.
 *   keep_out   uint8 [n_max]: 1 = keep, 0 = remove, in the points' own order; entries at or beyond
 *              the live count are not written.
 * A "finite point" has three finite coordinates.
 */
int64_t dp_clean_workspace_size(int64_t n_max);

/*
 * dp_sort_pairs: stable ascending sort of the first *n_dev (keys[i], values[i]) pairs by the key
 * bits [bit_lo, bit_hi) (0 <= bit_lo <= bit_hi <= 64; bits outside the range are ignored, pairs
 * equal in the range keep their input order).  Least-significant-digit radix sort, 8 bits per pass;
 * only the passes whose digit overlaps [bit_lo, bit_hi) run (a partial digit is masked), so the
 * number of launches depends on bit_lo and bit_hi alone.  A pass is three kernels: per-workgroup
 * digit histogram, scan of the [256][workgroups] table, scatter with in-tile ranks in input order
 * (64-lane ballot groups + per-wave counts in LDS); no kernel waits for another workgroup.  Passes
 * ping-pong between the caller's arrays and the workspace; the RESULT IS ALWAYS IN keys / values
 * (an odd number of passes ends with a copy back).  Elements at or beyond *n_dev are neither read
 * nor written.  fp64 keys are sorted through the order-preserving map of dp_seg_select (sign flip,
 * -0.0 folded onto +0.0), which the stages below apply themselves.
 */
int dp_sort_pairs(uint64_t* keys, uint32_t* values, const int32_t* n_dev, int32_t n_max, int32_t bit_lo,
                  int32_t bit_hi, void* workspace, int64_t workspace_bytes, dp_stream_t stream);

/*
 * dp_clean_stray: remove_stray_points(pcd, nb_points, radius).  Point j is kept iff the number of
 * live finite points i, j itself included, with (dx*dx + dy*dy) + dz*dz < radius*radius (strict,
 * every operation rounded in fp64) is >= nb_points.  This restates Open3D's
 * KDTreeFlann.search_radius_vector_3d (nanoflann's radius result set admits dist < radius^2);
 * Open3D itself was not available to check against, so this sentence is the specification.
 * A point with a non-finite coordinate has no neighbours and is removed (ours; the reference is
 * undefined there).
 * Method: cells of edge radius * (1 + 2^-20), 21 bits per axis packed (x, y, z) with z lowest,
 * dp_sort_pairs on (cell, index), then each point scans the 9 (x, y) cell rows around it -- a row's
 * three z-adjacent cells are one key range -- testing the original coordinates, and stops as soon
 * as the count reaches nb_points.  The cells only select candidates (see the argument in the source).
 *   stats_out  fp64 [8]: finite points, non-finite points, kept, removed, error flag, 0, 0, 0
 * Error flag (device side): an axis would need more than 2^21 - 2 cells ((max - min) / edge).  Then
 * NO point is removed (keep_out all 1, kept = live count) rather than use a wrong neighbourhood.
 * radius not finite or <= 0, or nb_points < 1: DP_ERR_SHAPE.
 */
int dp_clean_stray(const double* points, const int32_t* n_dev, int32_t n_max, double radius, int32_t nb_points,
                   uint8_t* keep_out, double* stats_out, void* workspace, int64_t workspace_bytes,
                   dp_stream_t stream);

/*
 * dp_clean_shadows: clean_shadows(pcd, height_threshold, max_angle, min_points).
 *   x / z min and max over the live finite points (n of them);
 *   density = n / ((x_max - x_min) * (z_max - z_min)); v = 1.0 / sqrt(density / 10);
 *   cell = v if v > 0.05 else 0.05 (Python's max(0.05, v): zero area or a NaN give 0.05) -- all in a
 *   one-thread kernel, nothing is read back;
 *   x_bins = np.arange(x_min, x_max + cell, cell): ceil(((x_max + cell) - x_min) / cell) edges, filled
 *   as numpy fills them: e[0] = x_min, e[1] = x_min + cell, e[i] = x_min + i * (e[1] - e[0]);
 *   xi = np.digitize(x, x_bins) - 1 = the last i with e[i] <= x (found on the edges themselves, not
 *   from the quotient); the same for z; column = xi * len(z_bins) + zi.
 * A column with count >= min_points, count >= 3 and y_max - y_min > height_threshold is tested: its
 * points ordered by y, TIES IN INDEX ORDER (stated difference: the reference's np.argsort is
 * unstable for columns of more than 16 points), consecutive differences v,
 * a = arccos(clip(v_y / sqrt((v_x^2 + v_y^2) + v_z^2), -1, 1)) * 180 / pi, and the column is removed
 * iff np.median(a) < max_angle.  A zero-length v gives NaN and a NaN median: the column is kept, as
 * numpy does.  Order: dp_sort_pairs on the y key (64 bits), then on the column id (32 bits,
 * stable).  The median is decided without a second sort: with m angles, c of them below the limit,
 * odd m removes iff c >= (m + 1) / 2; even m removes if c > m / 2, keeps if c < m / 2, and for
 * c == m / 2 tests (largest angle below + smallest angle not below) / 2 < max_angle.  Per-column
 * values are reductions over the sorted run onto its head position (no dense table of columns).
 * A non-finite point is in no column, is kept and is counted.
 *   stats_out  fp64 [8]: finite points, non-finite points, columns occupied, columns tested,
 *              columns removed, points removed, cell size, error flag
 * Error flag (device side): len(x_bins) * len(z_bins) >= 2^31 (or not finite, or edges that do not
 * grow in fp64).  Then every point is kept.  min_points < 1 or a NaN threshold: DP_ERR_SHAPE.
 */
int dp_clean_shadows(const double* points, const int32_t* n_dev, int32_t n_max, double height_threshold,
                     double max_angle, int32_t min_points, uint8_t* keep_out, double* stats_out, void* workspace,
                     int64_t workspace_bytes, dp_stream_t stream);

/*
 * dp_compact_points: the first *n_out_dev rows of points_out (and colors_out, uint8 [n_max][3], if
 * colors != NULL) are the live rows with keep[i] != 0, in their original order; *n_out_dev (device
 * int32) is their number, so the next stage can take it as its n_dev.  Rows at or beyond that
 * count are not written.  Outputs must not alias inputs.  Workgroup counts, one scan of them, an
 * order-preserving scatter; no look-back.
 */
int dp_compact_points(const double* points, const uint8_t* colors, const uint8_t* keep, const int32_t* n_dev,
                      int32_t n_max, double* points_out, uint8_t* colors_out, int32_t* n_out_dev, void* workspace,
                      int64_t workspace_bytes, dp_stream_t stream);

/*
 * ---- Clustered point clouds (ABI 17, csrc/dp_cluster.hip) -----------------------------------------
 * The per-point part of the reference pipeline's last step, the floor plan: fit_shapes_to_clusters
 * (simple_pointcloud_viewer.py:332-412) runs DBSCAN(eps=0.2, min_samples=5) on the (-x, z)
 * coordinates of the points with y >= height_threshold and fits a shape to each cluster.  Here: the
 * DBSCAN labels, exactly as sklearn computes them, and a table + cluster-ordered index for the
 * shape fit (the fits themselves: "Cluster shapes", ABI 18, below).  The ground and clean sections' conventions hold:
 * fp64 points [n_max][3], n_dev a device int32 (NULL: n_max; clamped to [0, n_max]), n_max = 0 and
 * *n_dev = 0 valid, everything on the caller's stream with no synchronisation and no host read-back,
 * each fp64 product and sum rounded on its own (no FMA), argument errors returned as DP_ERR_* before
 * any launch.
 *   workspace  >= dp_cluster_workspace_size(n_max) bytes of device memory, 8-byte aligned, owned by
 *              the call until the stream has passed it.  About 100 bytes per point (the sort's
 *              workspace included).
 *
 * Specification.  Participants are the live rows that are finite, have y >= height_threshold (test
 * skipped for a NaN threshold) and are in the sample (below).  Clustering is over (x, z); negating
 * x, as the reference does, changes no distance and is not done.
 *   1. Participants i and j are neighbours iff dx*dx + dz*dz <= eps*eps: inclusive, i == j included,
 *      every product and sum rounded on its own in fp64 (what sklearn's kd-tree evaluates).
 *   2. A participant is a core point iff it has at least min_samples neighbours.
 *   3. Two core points are in one cluster iff a chain of core points, each a neighbour of the next,
 *      joins them.  Clusters are numbered 0, 1, ... in increasing order of their smallest core row.
 *   4. A non-core participant with a core neighbour gets the smallest cluster number among its core
 *      neighbours (sklearn expands clusters in that order, so the first to reach it is the smallest);
 *      without one it is noise: label -1.
 *   5. Live rows that do not take part get label -2.
 * Sampling: max_points = 0 clusters every eligible row (finite, high enough); max_points = m > 0 with
 * e > m eligible rows (e counted on the device) takes an even stride: the k-th eligible row, in row
 * order from k = 0, takes part iff k == 0 or floor(k m / e) != floor((k - 1) m / e) in 64-bit
 * integers -- exactly m rows.  e <= m takes them all.  Stated difference: the reference draws an
 * unseeded np.random.choice(100000); this is deterministic.
 *
 * Method.  Cells of edge eps / sqrt(2) * (1 - 2^-20) over (x, z), 21 bits per axis packed with z
 * lowest, dp_sort_pairs on (cell, row), coordinates gathered into sorted order.  Any two points of
 * one cell are neighbours in the rounded arithmetic (argument in the source), so a cell with
 * >= min_samples participants makes them all core and one set without a distance test.  A point's
 * neighbours lie in the 5 x 5 block of cells around its own; a block row is one key range found by
 * binary search.  (All 25 cells: with the shrunk edge two points across a corner of the block can
 * be nearer than eps, so the corners are walked too.)  Core flags count neighbours with an early
 * exit at min_samples.  Clusters: lock-free union-find over core points in row-index space, the
 * larger root hooked under the smaller by a CAS on the root's own word, then compressed, so every
 * root is its cluster's smallest core row; numbering = exclusive scan of the root flags in row
 * order.  Border points take the minimum over their core neighbours, one hit per dense cell.
 * Bounds this implementation keeps:
 *   - no kernel spins on another workgroup's progress; union-find retries on its own CAS only;
 *   - no thread loops to n_max: per-thread loops run over the contents of at most 25 cells (plus
 *     binary searches);
 *   - k coincident points cost O(k log n), not k^2 distance tests (the dense-cell rule);
 *   - an axis that would need more than 2^21 - 3 cells ((max - min) / edge over the participants)
 *     raises the device-side error flag: every participant is labelled -1 and *n_clusters_dev = 0.
 *     Nothing is labelled from a wrong neighbourhood.
 */
int64_t dp_cluster_workspace_size(int64_t n_max);

/*
 * dp_cluster_dbscan:
 *   labels_out      int32 [n_max], written for live rows only: cluster number, -1 noise, -2 not a
 *                   participant
 *   n_clusters_dev  device int32: the number of clusters
 *   stats_out       fp64 [8]: finite points, non-finite points, participants, core points, border
 *                   points, noise points, clusters, error flag
 * eps not finite or <= 0, min_samples < 1, max_points < 0 (or n_max < 0): DP_ERR_SHAPE.
 * The call leaves the clusters' smallest core rows in the head of its workspace, for
 * dp_cluster_table.
 */
int dp_cluster_dbscan(const double* points, const int32_t* n_dev, int32_t n_max, double eps, int32_t min_samples,
                      double height_threshold, int32_t max_points, int32_t* labels_out, int32_t* n_clusters_dev,
                      double* stats_out, void* workspace, int64_t workspace_bytes, dp_stream_t stream);

/*
 * dp_cluster_table: per-cluster rows and the cluster-ordered index, K = min(*n_clusters_dev,
 * max_clusters) clusters.
 *   table_out    fp64 [max_clusters][12], rows c < K written: count, smallest core row, x min, x max,
 *                z min, z max, y min, y max, sum x, sum y, sum z, 0.  Count and bounds are exact;
 *                a sum is accumulated in an unspecified order (wave-level sums, then fp64 atomics),
 *                so within (count - 1) * 2^-53 * sum |v| of the exact one.
 *   order_out    uint32 [n_max]: the rows with label >= 0, grouped by cluster and in row order inside
 *                a cluster (dp_sort_pairs on (label, row)); entries past their number are not written.
 *   offsets_out  int32 [max_clusters + 1], entries c <= K written: cluster c's members are
 *                order_out[offsets_out[c] : offsets_out[c + 1]] -- the reference's
 *                points_2d[labels == c] without a pass per cluster.
 * The smallest core row cannot be read off the labels (a border point may have a smaller row), so it
 * is taken from the workspace: pass the workspace of the dp_cluster_dbscan call that produced
 * `labels` (same n_max, not used by anything else in between) and column 1 is that cluster's
 * smallest core row; in any other workspace -- zero-filled at least in its first 256 bytes --
 * column 1 is -1.  Everything else depends on points and labels alone.  max_clusters < 0 (or
 * n_max < 0): DP_ERR_SHAPE.
 */
int dp_cluster_table(const double* points, const int32_t* labels, const int32_t* n_dev, int32_t n_max,
                     const int32_t* n_clusters_dev, int32_t max_clusters, double* table_out, uint32_t* order_out,
                     int32_t* offsets_out, void* workspace, int64_t workspace_bytes, dp_stream_t stream);

/*
 * ---- Cluster shapes (ABI 18, csrc/dp_shapes.hip) ---------------------------------------------------
 * The rest of the reference's floor-plan step: per cluster the convex hull, the minimum-area
 * rectangle, the least-squares circle and the circle-or-rectangle decision of fit_shapes_to_clusters
 * (simple_pointcloud_viewer.py:332-412, fit_circle :12-42, is_better_fit_as_circle :44-77), from the
 * order / offsets / cluster count of a dp_cluster_table call.  The ground, clean and cluster
 * sections' conventions hold: fp64 points [n_max][3], n_dev a device int32 (NULL: n_max; clamped to
 * [0, n_max]), n_max = 0, *n_dev = 0 and zero clusters valid, everything on the caller's stream with
 * no synchronisation and no host read-back, each fp64 product, sum and difference rounded on its own
 * (no FMA), argument errors returned as DP_ERR_* before any launch.
 *   workspace  >= dp_shapes_workspace_size(n_max, max_clusters) bytes of device memory, 8-byte
 *              aligned, owned by the call until the stream has passed it (content need not be
 *              initialised).  About 28 bytes per point and 40 per cluster.
 *
 * Frame.  Shapes are fitted in the reference's top-down frame u = -x, v = z
 * (simple_pointcloud_viewer.py / pointcloud_pipeline.py:111-118).  The negation is exact; it makes
 * centres and angles the reference's numbers (the cluster stage, which only measures distances, did
 * not need it).
 *
 * Specification.  For each cluster c < K = min(*n_clusters_dev, max_clusters), members
 * order[offsets[c] : offsets[c + 1]] (ascending rows), N of them:
 *   1. N < 5: skipped, as the reference does (:362).  kind 0, count N, every other column 0.
 *   2. Convex hull.  o(a, b, c) = (bu - au) * (cv - av) - (bv - av) * (cu - au), every operation
 *      rounded on its own.  The hull's vertices are the members that are strict corners (o > 0 taken
 *      counter-clockwise): collinear and duplicate points are not vertices; among coincident members
 *      the smallest row is the vertex.  They are listed counter-clockwise from the lexicographically
 *      smallest (u, v): the monotone chain over the members sorted by (u, v, row) with one member per
 *      distinct (u, v), a point leaving the stack unless o(second from top, top, new) > 0; lower
 *      hull left to right, then upper hull right to left.  One distinct point gives one vertex, two
 *      (or any exactly collinear set) two.  hull_area = (sum over i = 1 .. h - 2 of
 *      o(p_0, p_i, p_i+1)) / 2: the shoelace sum taken from the first vertex, where every term is
 *      positive (summation order unspecified).
 *   3. Minimum-area rectangle (rotating calipers), h >= 2.  For every hull edge i, p_i -> p_i+1
 *      (the last back to p_0), in list order: d = p_i+1 - p_i, len = sqrt(du*du + dv*dv),
 *      e = (du / len, dv / len), n = (-e_v, e_u); over ALL hull vertices p = u*e_u + v*e_v and
 *      q = v*e_u - u*e_v; width = max p - min p, height = max q - min q, area = width * height.  The
 *      smallest area wins, ties go to the smallest i.  With pc = (min p + max p) / 2 and
 *      qc = (min q + max q) / 2: centre = (e_u*pc - e_v*qc, e_v*pc + e_u*qc),
 *      angle = atan2(e_v, e_u) * 57.29577951308232 degrees, folded into [0, 90):
 *      k = floor(angle / 90), angle -= 90 * k, and if that rounds to 90 (a tiny negative angle)
 *      angle = 0, k += 1; odd k swaps width and height.  h = 1 (N coincident points): a 0 x 0
 *      rectangle at that point, angle 0, area 0.
 *      Stated differences from the reference: cv2.minAreaRect works on a float32 copy of the points
 *      and its angle convention depends on the OpenCV version; this fit is in fp64 on the fp64 points
 *      and its convention is the one above.
 *   4. Circle: the reference's fit_circle minimises sum (R_i - mean R)^2 over the centre with
 *      scipy.optimize.leastsq from the members' mean.  Here the same residuals and start, by a damped
 *      Gauss-Newton (Levenberg-Marquardt) iteration.  At a centre (x, y): R_i = sqrt((u_i - x)^2 +
 *      (v_i - y)^2), a_i = (u_i - x) / R_i, b_i = (v_i - y) / R_i (both 0 where R_i = 0); the sums
 *      SR, Sa, Sb, Saa, Sab, Sbb, SaR, SbR, SRR of R, a, b, a a, a b, b b, a R, b R, R R (summation
 *      order unspecified); Rm = SR / N, A11 = Saa - Sa*Sa/N, A12 = Sab - Sa*Sb/N,
 *      A22 = Sbb - Sb*Sb/N, g1 = SaR - Sa*Rm, g2 = SbR - Sb*Rm, cost = SRR - SR*Rm.
 *      Start: (x, y) = (sum u / N, sum v / N), lambda = 1e-3.  At most 50 times:
 *        M11 = A11 (1 + lambda), M22 = A22 (1 + lambda), det = M11*M22 - A12*A12; stop unless det > 0;
 *        dx = (M22*g1 - A12*g2) / det, dy = (M11*g2 - A12*g1) / det; evaluate the sums at
 *        (x + dx, y + dy);
 *        if its cost <= cost: move there, lambda /= 10, and stop if sqrt(dx*dx + dy*dy) <= 1e-13 * its Rm;
 *        else lambda *= 10, and stop if lambda > 1e10.
 *      xc, yc = the final centre, r = its Rm, fit_error = (sum (R_i - r)^2 / N) / (r*r).
 *   5. Decision (is_better_fit_as_circle): circle_area = pi * (r*r); h < 3 or hull_area not > 0: a
 *      rectangle with circ = 0 (where the reference's qhull call raises, and its fallback rule cannot
 *      say "circle" for a zero rectangle area).  Otherwise circ = hull_area / circle_area,
 *      circ = min(circ, 1 / circ), and the cluster is a circle iff circ > circularity_threshold and
 *      fit_error < 0.15 and |circle_area - area| / max(circle_area, area) < 0.3 (area: the
 *      rectangle's), every comparison false on NaN.
 *   6. Row c of shapes_out, fp64 [max_clusters][16], rows c < K written: kind (0 skipped, 1 rectangle,
 *      2 circle), count, rectangle centre u, centre v, width, height, angle, area, circle xc, yc, r,
 *      fit_error, hull_area, hull vertex count, circ, error flag.
 *   hull_rows_out     int32 [n_max]: the hulls' vertices as row numbers, cluster after cluster
 *   hull_offsets_out  int32 [max_clusters + 1], entries c <= K written: cluster c's vertices are
 *                     hull_rows_out[hull_offsets_out[c] : hull_offsets_out[c + 1]]
 *
 * Method.  (u, v) is gathered once into cluster order.  Hulls by exact reduction (the hull of a union
 * is the hull of the hulls): a cluster's members are cut into chunks of DP_SHAPES_H_MAX; a workgroup
 * sorts its chunk in LDS by (u, v, row rank) (bitonic), runs the chain (lower and upper hull on two
 * waves) and writes the survivors back; rounds repeat until the cluster is one chunk, whose hull is
 * the cluster's; that workgroup then takes the area and the calipers (one lane per edge over the
 * vertices in LDS, min-reduction with the index tie-break).  Chunk lists are built on the device by
 * one-workgroup scans.  Circle: one workgroup per cluster streams the gathered members once per
 * evaluation (wave reductions of the nine sums).
 * Bounds this implementation keeps:
 *   - no kernel waits on another workgroup;
 *   - no thread loops over a whole cluster: the chain's two serial loops run over one chunk
 *     (<= DP_SHAPES_H_MAX members), the circle's loops over 1/256 of a cluster per evaluation;
 *   - at most 6 hull rounds, and at most DP_SHAPES_H_MAX hull vertices per cluster.  A cluster that
 *     is not down to one chunk by then (its hull has more vertices, or shrinks too slowly) gets error
 *     flag 1, kind 0, an empty hull range and every other column but the count 0: nothing is fitted
 *     from a truncated hull.  Other clusters of the call are not affected.
 * The last step of fit_shapes_to_clusters, detect_and_split_l_shapes (:79-282), works on the rectangle
 * list produced here: "L-shape split" (additive to ABI 20) below.
 * circularity_threshold NaN, max_clusters < 0 or n_max < 0: DP_ERR_SHAPE.
 */
#define DP_SHAPES_H_MAX 2048
int64_t dp_shapes_workspace_size(int64_t n_max, int64_t max_clusters);
int dp_cluster_shapes(const double* points, const int32_t* n_dev, int32_t n_max, const uint32_t* order,
                      const int32_t* offsets, const int32_t* n_clusters_dev, int32_t max_clusters,
                      double circularity_threshold, double* shapes_out, int32_t* hull_rows_out,
                      int32_t* hull_offsets_out, void* workspace, int64_t workspace_bytes, dp_stream_t stream);

/*
 * ---- Oriented mesh points (ABI 19, csrc/dp_normals.hip) --------------------------------------------
 * The per-point start of the reference's fourth pipeline step, create_mesh_from_pointcloud
 * (pointcloud_to_mesh.py:313-395).  Every meshing method there begins with the same three Open3D calls
 * on the cleaned cloud: voxel_down_sample(voxel_size), estimate_normals(KDTreeSearchParamHybrid(radius =
 * 2 * voxel_size, max_nn = 30)) and orient_normals_towards_camera_location([0, 0, 0]).  (Its first
 * estimate_normals, on the full cloud, is overwritten by the one after down-sampling and is skipped
 * here.)  Their product, an oriented point set, is what a surface reconstructor takes as input; Poisson
 * and ball-pivoting reconstruction and the non-manifold clean-up are out of scope (the reference's third
 * method is the "Triangle mesh" section below).  The ground, clean and
 * cluster sections' conventions hold: fp64 points [n_max][3], n_dev a device int32 (NULL: n_max;
 * clamped to [0, n_max]), n_max = 0 and *n_dev = 0 valid, everything on the caller's stream with no
 * synchronisation and no host read-back, each fp64 product, sum and difference rounded on its own (no
 * FMA), argument errors returned as DP_ERR_* before any launch.  Rows at or beyond the live count are
 * neither read nor written.
 *   workspace  >= dp_normals_workspace_size(n_max) bytes of device memory, 8-byte aligned, owned by the
 *              call until the stream has passed it (content need not be initialised).  About 90 bytes
 *              per point (the sort's workspace included).
 *   stats_out  fp64 [8], one layout for the three calls: finite rows, non-finite rows, [2] voxels
 *              (dp_voxel_downsample) or finite rows with fewer than 3 neighbours (the other two),
 *              rows whose list was truncated to max_nn (dp_knn_search), flipped normals
 *              (dp_estimate_normals), error flag, 0, 0.  A call leaves the entries of the others 0.
 * Open3D was not available to check against, so, as for dp_clean_stray, the sentences below are the
 * specification (restated in tests/normals_numpy.py, which is pinned to scipy's cKDTree and
 * numpy.linalg.eigh).
 *
 * Voxel grid (dp_voxel_downsample).  Per axis origin = (minimum over the finite live rows) -
 * voxel_size / 2 and index = floor((v - origin) / voxel_size), clamped to [0, 2^21 - 2].  A voxel is
 * the set of finite rows with one index triple; its key is (ix << 42) | (iy << 21) | iz.
 *   points_out    fp64 [n_max][3]: voxel v's point = the mean of its members' coordinates (fp64 sums in
 *                 an unspecified but fixed order, then one division by the member count)
 *   colors_out    uint8 [n_max][3] (colors != NULL): per channel (2 * sum + m) / (2 * m) in integers,
 *                 m the member count: the mean rounded half up
 *   count_out     int32 [n_max]: voxel v's member count
 *   voxel_of_out  int32 [n_max]: the voxel of every live row, -1 for a non-finite row
 *   n_out_dev     device int32: the number of voxels; rows at or beyond it of the three arrays above
 *                 are not written
 * Voxels come in ascending key order.  Stated difference: Open3D's order is that of a hash map.
 * Error flag (device side): an axis would need more than 2^21 - 2 voxels ((max - origin) / voxel_size).
 * Then *n_out_dev = 0 and voxel_of_out is -1 throughout.  voxel_size not finite or <= 0: DP_ERR_SHAPE.
 * Method: the cell keys go through dp_sort_pairs with the row as payload (stable, so a voxel's run is in
 * row order); run heads are flagged and scanned (voxel numbers, *n_out_dev), and one wave per voxel sums
 * its run.
 *
 * Hybrid search (dp_knn_search).  Participants are the finite live rows.  Row j is a neighbour of row i
 * iff d2 = (dx*dx + dy*dy) + dz*dz < radius*radius -- the expression and strictness of dp_clean_stray;
 * row i is its own neighbour.  Of more than max_nn neighbours the max_nn smallest by (d2, row) are kept.
 *   nbr_out        int32 [n_max][max_nn]: row i's neighbours in ascending (d2, row) order, then -1
 *   nbr_count_out  int32 [n_max]: their number, min(neighbours, max_nn); 0 for a non-finite row
 * max_nn in [1, 64], radius finite and > 0 (else DP_ERR_SHAPE).
 * Error flag (device side): an axis would need more than 2^21 - 2 cells of edge radius.  Then every
 * count is 0 (and every list -1): nothing is listed from a wrong neighbourhood.
 * Method: the stray stage's grid (cells of edge radius * (1 + 2^-20), dp_sort_pairs, coordinates
 * gathered into cell order, each of the 9 (x, y) cell rows around a point one key range found by binary
 * search).  One wave per query: the lanes stride a range's candidates 64 at a time; a batch holding a
 * candidate below the current max_nn-th smallest is sorted across the lanes (bitonic network on
 * shuffles) and merged into the running best, kept one entry per lane in ascending order.  No scratch,
 * no per-thread arrays.
 *
 * Normals (dp_estimate_normals), from the lists of a dp_knn_search call (same points, same max_nn).
 * A finite row with m = nbr_count < 3 listed neighbours gets (0, 0, 1).  Otherwise, over the listed
 * neighbours in list order: mean = (sum p) / m, then C = (sum (p - mean)(p - mean)^T) / m, two passes,
 * fp64; the normal is the unit eigenvector of C's smallest eigenvalue (cyclic Jacobi on the 3 x 3 until
 * the off-diagonal sum no longer changes the diagonal sum, then the column of the smallest diagonal
 * entry divided by its length).  A zero or non-finite vector becomes (0, 0, 1).  Stated difference:
 * Open3D accumulates the uncentred moments in one pass and uses a closed-form solver; the eigenvector
 * is the same up to rounding wherever the two smallest eigenvalues are apart, its sign is arbitrary in
 * both.  With orient != 0 the normal (the (0, 0, 1) default included, as in Open3D) is negated when
 * (nx * (cx - px) + ny * (cy - py)) + nz * (cz - pz) < 0 with c = camera (HOST pointer, fp64 [3],
 * finite).  A non-finite row gets (0, 0, 0).  An entry of a list outside [0, live count) ends the list.
 *   normals_out  fp64 [n_max][3]
 * One thread per row; both passes gather the neighbours' coordinates, everything else is in registers.
 */
int64_t dp_normals_workspace_size(int64_t n_max);
int dp_voxel_downsample(const double* points, const uint8_t* colors, const int32_t* n_dev, int32_t n_max,
                        double voxel_size, double* points_out, uint8_t* colors_out, int32_t* count_out,
                        int32_t* voxel_of_out, int32_t* n_out_dev, double* stats_out, void* workspace,
                        int64_t workspace_bytes, dp_stream_t stream);
int dp_knn_search(const double* points, const int32_t* n_dev, int32_t n_max, double radius, int32_t max_nn,
                  int32_t* nbr_out, int32_t* nbr_count_out, double* stats_out, void* workspace,
                  int64_t workspace_bytes, dp_stream_t stream);
int dp_estimate_normals(const double* points, const int32_t* n_dev, int32_t n_max, const int32_t* nbr,
                        const int32_t* nbr_count, int32_t max_nn, const double* camera, int32_t orient,
                        double* normals_out, double* stats_out, dp_stream_t stream);

/*
 * ---- Occupancy floor plan (ABI 20, csrc/dp_floorplan.hip) ------------------------------------------
 * The reference's second floor-plan output, cleaned_pointcloud_to_floorplan.py, up to the contour
 * tracing: the top-down density grid (create_density_grid_from_points :172-212, create_direct_floorplan
 * :676-886), the morphological closing and opening of process_height_slice (:245-311: closing 7 x 7
 * twice, opening 3 x 3), the connected regions the reference then outlines, and a picture.  The ground,
 * clean and cluster sections' conventions hold: fp64 points [n_max][3], n_dev a device int32 (NULL:
 * n_max; clamped to [0, n_max]), everything on the caller's stream with no synchronisation and no host
 * read-back, each fp64 product, sum and difference rounded on its own (no FMA), argument errors returned
 * as DP_ERR_* before any launch.
 * The grid's size is only known on the device.  Grid buffers have the caller's capacity max_cells (in
 * [0, 2^31 - 1]); dims is a device int32 [2] = (H, W), written by dp_occupancy_grid and read ON THE DEVICE
 * by every later stage -- it is their live count, as n_dev is the raster's.  A dims outside [0,
 * DP_FLOOR_MAX_DIM] or with H * W > max_cells is read as (0, 0).  Grids are row-major, cell = gz * W + gx,
 * row 0 = smallest z; cells at or beyond H * W are neither read nor written.
 *   workspace  >= dp_floorplan_workspace_size(max_cells, max_regions) bytes of device memory, 8-byte
 *              aligned, owned by the call until the stream has passed it (content need not be
 *              initialised).  About 13.3 bytes per cell and 96 per region.  dp_occupancy_grid and
 *              dp_grid_morphology need dp_floorplan_workspace_size(max_cells, 0) only.
 * OpenCV is not available to check against; the rules below are the specification (restated in
 * tests/floorplan_numpy.py, which is pinned to scipy.ndimage).
 *
 * Raster (dp_occupancy_grid).
 *   1. Participants: the finite live rows with y >= height_threshold; a NaN threshold takes every finite
 *      row (an infinite one: DP_ERR_SHAPE).
 *   2. Coordinates are x and z as stored.  The picture does NOT take the x flip (u = -x) of the shapes
 *      stage: it is the reference's imshow of its own grid, which has none.
 *   3. min_x = (minimum of x over the participants) - padding, max_x = (maximum) + padding, the same for
 *      z.  W = (int)ceil((max_x - min_x) / resolution), H from z (create_density_grid_from_points).
 *      origin_out, fp64 [2] on the device = (min_x, min_z).
 *   4. A participant's cell: gx = (int)((x - min_x) / resolution), gz likewise.  A row with gx >= W or
 *      gz >= H is dropped and counted (with padding = 0 the row on the maximum is: the reference drops
 *      it too).
 *   5. Per cell:  density_out  uint32: the number of its members;
 *                 height_out   float32: the largest (float)y of its members, 0 in an empty cell (-0.0
 *                              counts as +0.0);
 *                 color_out    uint8 [3] (colors != NULL): the colour of the member with the largest
 *                              (float)y, among equal heights the smallest row; not written in an empty
 *                              cell;
 *                 occupied_out uint8: density > 0.
 *   6. stats_out fp64 [8]: participants, non-finite rows, finite rows below the threshold, dropped rows,
 *      occupied cells, H, W, error.  Error 1: no participants.  Error 2: W or H exceeds
 *      DP_FLOOR_MAX_DIM, or W * H > max_cells.  Under either dims = (0, 0) and no cell is written
 *      (origin is 0, 0 under error 1).
 *   Stated differences: the reference's loop never colours a cell whose heights are all <= 0 and takes
 *   the first of equal heights in its (randomly thinned) order; here every occupied cell has an owner and
 *   ties go to the smallest row.  The reference thins the cloud at random in its fast mode; this uses
 *   every participant.
 *   Method: one pass for the minimum / maximum, one for the cells: a 64-bit atomicMax on (ordered float32
 *   bits of y) << 32 | ~row gives height and colour owner at once, beside an atomicAdd on the density; a
 *   wave first joins the rows that share a cell (they mostly do: the cloud is in image order), so a dense
 *   cell takes one atomic pair per wave, not per row.
 *   resolution not finite or <= 0, padding not finite or < 0: DP_ERR_SHAPE.
 *
 * Morphology (dp_grid_morphology): cv2.morphologyEx on the binary grid (non-zero = set; the output is 0 / 1).
 *   7. close_iters times: a dilation, then an erosion, by a close_size x close_size square of ones; then
 *      once: an erosion, then a dilation, by open_size x open_size.  Sizes are odd and in [1,
 *      DP_FLOOR_MAX_KERNEL] (else DP_ERR_SHAPE); size 1, or 0 iterations, is the identity.
 *   8. Border (OpenCV's default): a dilation reads the cells outside the grid as 0, an erosion reads them
 *      as 1: scipy.ndimage.binary_dilation(border_value=0) and binary_erosion(border_value=1) with the
 *      same structure.  (ndimage.binary_closing itself erodes with border 0 and is not the same.)
 *   grid_out may be grid.
 *   Method: rows packed 64 cells to a word by a wave's ballot; a square of ones is separable: the row pass
 *   is shifts of a word and its two neighbours ORed / ANDed, the column pass ORs / ANDs k row words.  No LDS.
 *
 * Regions (dp_grid_regions): the 8-connected components of a uint8 grid (non-zero = set) and their table.
 *   9. labels_out int32 [max_cells]: 0 on background; components numbered from 1 in row-major order of
 *      their first cell -- scipy.ndimage.label(structure = ones((3, 3))).
 *  10. n_regions_dev, device int32: the number of regions.  table_out fp64 [max_regions]
 *      [DP_FLOOR_COLUMNS], rows r < min(regions, max_regions) written, row r for label r + 1:
 *        0 cells; 1 area in m^2 = cells * (resolution * resolution); 2..5 bounding box gx0, gz0, gx1, gz1
 *        (inclusive); 6, 7 centroid in cells: (sum of gx) / cells, (sum of gz) / cells, the sums exact
 *        (64-bit integers), one division each; 8, 9 centroid in world coordinates origin + (c + 0.5) *
 *        resolution; 10 points: the sum of density over the region; 11 the largest height over the
 *        region's cells with density > 0 (0 if none); 12 the mean of height over those cells (0 if none):
 *        an fp64 sum in an unspecified order, divided by their number.
 *      A region past max_regions keeps its label but has no row.
 *  11. stats_out fp64 [8]: set cells, regions, rows written, overflow flag (regions > max_regions), H, W,
 *      0, 0.
 *   density and height are the raster's (or any arrays of that layout); origin is its origin_out.
 *   Method: union-find over the cell index (dp_points.h: hook the larger root under the smaller, path
 *   halving), each cell joined to its west, north-west, north and north-east neighbours; the root of a
 *   region is then its first cell, and a scan of the root flags numbers them.  The table is accumulated
 *   with 64-bit integer atomics (one fp64 atomic for the height sum).
 *   Bounds: no kernel waits on another workgroup; a find walks at most the chain to its root, which
 *   halving keeps short but which is not bounded below the region's size.
 *   Stated difference: the reference measures a region by cv2.contourArea of its traced outline and
 *   drops those of 5 or less; here the area is the cell count.  findContours, approxPolyDP and the polygons
 *   file are the next section, "Floor-plan polygons", which does measure a region by its traced outline
 *   (detect_and_split_l_shapes belongs to the shapes stage: "L-shape split" below).
 *
 * Picture (dp_floorplan_image): image_out uint8 [max_cells][3], RGB, H x W as the grids (row 0 = smallest z).
 *  12. White background.  A cell whose label has a table row with area >= min_area is filled; the cells
 *      of every other region (too small, or past max_regions) are background.
 *  13. Fill colour, with color_by_height: h = min(1, mean / max_height) from the row's mean height,
 *      r = (int)(255 h), g = (int)(255 (1 - |2h - 1|)), b = (int)(255 (1 - h)), each saturated to [0, 255]
 *      (as OpenCV does with a colour tuple; only a negative mean needs it).  Without: grey 180.
 *  14. A filled cell with a 4-neighbour outside the grid or of another label is black (the outline).
 *  15. The reference's 1 m scale bar with its non-fast sizes: L = (int)(1 / resolution), x0 = min(W - 50 - L,
 *      W - 10), z0 = min(H - 50, H - 10); if x0 > 0, z0 > 0, z0 < H and x0 + L < W the cells
 *      [z0, z0 + 20) x [x0, x0 + L) inside the grid are black.  The Hershey title and "1m" text are not drawn.
 *   min_area finite and >= 0, max_height and resolution finite and > 0 (else DP_ERR_SHAPE).
 */
#define DP_FLOOR_MAX_DIM 8192
#define DP_FLOOR_MAX_KERNEL 15
#define DP_FLOOR_COLUMNS 13
int64_t dp_floorplan_workspace_size(int64_t max_cells, int64_t max_regions);
int dp_occupancy_grid(const double* points, const uint8_t* colors, const int32_t* n_dev, int32_t n_max,
                      double height_threshold, double resolution, double padding, int32_t max_cells,
                      uint32_t* density_out, float* height_out, uint8_t* color_out, uint8_t* occupied_out,
                      int32_t* dims_out, double* origin_out, double* stats_out, void* workspace,
                      int64_t workspace_bytes, dp_stream_t stream);
int dp_grid_morphology(const uint8_t* grid, const int32_t* dims, int32_t max_cells, int32_t close_size,
                       int32_t close_iters, int32_t open_size, uint8_t* grid_out, void* workspace,
                       int64_t workspace_bytes, dp_stream_t stream);
int dp_grid_regions(const uint8_t* grid, const uint32_t* density, const float* height, const int32_t* dims,
                    const double* origin, int32_t max_cells, double resolution, int32_t max_regions,
                    int32_t* labels_out, int32_t* n_regions_dev, double* table_out, double* stats_out,
                    void* workspace, int64_t workspace_bytes, dp_stream_t stream);
int dp_floorplan_image(const int32_t* labels, const int32_t* dims, int32_t max_cells, const double* table,
                       const int32_t* n_regions_dev, int32_t max_regions, double resolution, double min_area,
                       double max_height, int32_t color_by_height, uint8_t* image_out, dp_stream_t stream);

/*
 * ---- Floor-plan polygons (additive to ABI 20, csrc/dp_outline.hip) ----------------------------------
 * The rest of the reference's cleaned_pointcloud_to_floorplan.py behind the regions: the outline of each
 * region (cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE), process_height_slice :309), its
 * simplification (approximate_contour :314-387: contourArea, arcLength, approxPolyDP, Polygon.is_valid, the
 * rectangle snap) and the mean height that labels the polygons file (create_height_slices :143).  The
 * floor-plan section's conventions hold: dims and n_regions are read ON THE DEVICE, buffers have the
 * caller's capacity, everything runs on the caller's stream with no synchronisation and no host read-back,
 * argument errors are returned as DP_ERR_* before any launch, no kernel waits on another workgroup, and
 * every loop is bounded by a count known at its start.  The block is additive: no existing entry point or
 * layout changes, and DP_ABI_VERSION stays 20.  Vertices are (x, y) = (gx, gz) in grid units.
 * OpenCV, skimage and shapely are not available to check against; the rules below are the specification
 * (restated sequentially in tests/outline_numpy.py, pinned to scipy where scipy can pin them).
 *   workspace  >= dp_outline_workspace_size(max_cells, max_regions, max_vertices) bytes of device memory,
 *              8-byte aligned, owned by the call until the stream has passed it (content need not be
 *              initialised): about 20 bytes per vertex and 100 per region, nothing per cell.  Both calls
 *              take the same size; dp_simplify_outlines must get the max_regions and max_vertices of the
 *              outlines it reads.
 *
 * Outline (dp_region_outlines), for each region with a table row, r < R = min(*n_regions, max_regions),
 * label r + 1, read from `labels` as dp_grid_regions wrote them:
 *   O1. Start.  s = the region's first cell in row-major order (the cell that gives it its label).
 *   O2. Border following (Suzuki-Abe's outer border as OpenCV runs it).  Directions are numbered
 *       counter-clockwise on the screen with z down: 0 E, 1 NE, 2 N, 3 NW, 4 W, 5 SW, 6 S, 7 SE.  From s
 *       look clockwise beginning at W (W, NW, N, NE, E, SE, S, SW) for the first cell of the region, i1.
 *       None: the outline is the single vertex s.  Otherwise i2 = i1, i3 = s, and repeat: look
 *       counter-clockwise around i3, beginning one step after the direction of i2, for the first cell i4
 *       of the region (i2 itself is the eighth candidate); emit i3; stop if i4 == s and i3 == i1;
 *       otherwise i2 = i3, i3 = i4.  A cell on a one-cell-wide part is emitted once per pass.  Cells outside
 *       the grid are no cells of the region.  Holes are never entered: the walk keeps the outside on its
 *       searching side.
 *   O3. CHAIN_APPROX_SIMPLE.  An emitted cell is a vertex iff the step leaving it differs from the step
 *       that arrived at it, taken cyclically (the start's arriving step is the last step of the walk).  The
 *       start is always a vertex: it arrives by W, NE, N or NW and leaves by E, SE, S or SW.
 *   O4. columns_out int64 [max_regions][DP_OUTLINE_INT_COLUMNS], row r: 0 vertices; 1 emitted (border)
 *       cells; 2 the signed shoelace sum  sum_i (x_i * y_i+1 - x_i+1 * y_i)  over the vertices, last to
 *       first included, exact; 3 the start cell gz * W + gx (-1: the label has no cell, all columns 0).
 *       measures_out fp64 [max_regions][DP_OUTLINE_REAL_COLUMNS], row r: 0 area = |sum| / 2
 *       (cv2.contourArea); 1 perimeter (cv2.arcLength, closed): over consecutive vertices, last to first
 *       included, the float32 square root of dx * dx + dy * dy -- dx, dy converted to float32, both products
 *       and their sum rounded to float32 -- summed in fp64 in vertex order (the sum is exact below 2^29,
 *       so the order cannot show).
 *   O5. offsets_out int32 [max_regions + 1], vertices_out int32 [max_vertices][2].  Region r's vertices are
 *       written, in the order of O2 from s, at offsets[r] .. offsets[r + 1] iff the vertex counts of
 *       regions 0 .. r together are <= max_vertices; otherwise it keeps its columns, writes no vertices
 *       (offsets[r + 1] = offsets[r]) and raises the overflow flag.  So the first region that does not fit
 *       and every later one are left out, and nothing is written at or past max_vertices.  A region past
 *       max_regions is skipped.
 *       stats_out fp64 [8]: regions, rows R, vertices of all rows, vertices written, vertex overflow flag,
 *       region overflow flag (regions > max_regions), H, W.
 *   Method: a workgroup (one wave) per region walks its cycle.  The successor in O2 is a function of (cell,
 *   direction of the previous cell), so the border states form disjoint cycles and the walk is bounded by
 *   8 * (cells of the region), counted beforehand.  Lane k looks at the k-th candidate of a search and a
 *   ballot takes the first, so a step is one round of loads.  The walk runs twice: once for the columns,
 *   and, after one workgroup has scanned the counts into offsets, once more to write.
 *
 * Simplification (dp_simplify_outlines), for each row r in turn; the reference runs in height-threshold
 * mode, so its own halvings apply (the default mode without a threshold, with the halvings undone, is
 * dp_simplify_outlines_with and the section "Height-sliced floor plan" below).  polygons_out fp64 [max_regions][DP_POLYGON_COLUMNS] has one row per
 * region whether it keeps a polygon or not.
 *   S1. Area filter.  area * (resolution * resolution) < min_area / 4: no polygon (drop reason 1).  The
 *       reference divides min_area by 4 twice; the caller's min_area is after the first division.
 *   S2. epsilon = 0.005 * perimeter (alpha 0.01 halved).
 *   S3. Closed Douglas-Peucker on the integer vertices (cv2.approxPolyDP, closed).  Anchors: start at vertex
 *       0; three times, move to the vertex farthest from the current one (largest squared distance, first
 *       of equals in ring order starting after the current one).  The last two vertices visited are the
 *       anchors A (visited second) and B (visited last).  Early exit: if the last largest squared distance
 *       is <= epsilon * epsilon the result is the single vertex A, and S4 drops it.  Otherwise the ring is
 *       split into the chains A..B and B..A.  A chain keeps its interior vertex with the largest |cross| to
 *       the chord if cross^2 > epsilon^2 * |chord|^2 -- the cross product an exact integer, (double)cross *
 *       (double)cross against (epsilon * epsilon) * (double)(dx * dx + dy * dy) in fp64, the first of equal
 *       maxima in ring order -- and is split there, recursively.  The result is the kept vertices in ring
 *       order beginning at A, which is where OpenCV's output begins.
 *       Stated difference: approxPolyDP ends with a clean-up pass over nearly collinear neighbours.  It is
 *       NOT built: its exact form could not be stated with certainty, and neither it nor the rest of S3 can
 *       be checked against OpenCV where this library is built and tested.
 *   S4. Fewer than 3 vertices: no polygon (drop reason 2).
 *   S5. Polygon.is_valid and area > 0, exact in integers.  No polygon (drop reason 3) if two vertices of the
 *       ring coincide, two non-adjacent edges share a point (touching included), two adjacent edges overlap
 *       (a spike: collinear and folding back), or the ring's shoelace sum is 0.
 *   S6. Rectangle snap.  With 4 to 6 vertices: the ring's convex hull and the hull's minimum-area rectangle
 *       by rules 2 and 3 of "Cluster shapes" (hull, calipers, ties to the smallest edge, angle folded into
 *       [0, 90)), in fp64.  ring_area = |shoelace sum| / 2, rect_area = width * height.  If |rect_area -
 *       ring_area| / ring_area < 0.2 the polygon is the four corners cv2.boxPoints gives for (centre,
 *       (width, height), angle): with b = cos(angle) / 2, a = sin(angle) / 2:
 *         p0 = (cx - a h - b w, cy + b h - a w), p1 = (cx + a h - b w, cy - b h - a w), p2 = 2 c - p0,
 *         p3 = 2 c - p1, flag 1 (snapped).  Otherwise the polygon is the ring.
 *       Stated difference: the reference runs cv2.minAreaRect on float32 points with its own angle
 *       convention and measures the float32 box; sin and cos here are the device's.
 *   S7. polygons_out row r: 0 label r + 1; 1 vertices of the polygon (0 without one); 2 flags (1 =
 *       snapped); 3 area in cells (the ring's, or the rectangle's when snapped; 0 without a polygon);
 *       4 that area * (resolution * resolution); 5 epsilon; 6 drop reason: 0 kept, 1 too small, 2 fewer than
 *       3 vertices, 3 invalid, 4 overflow (the outline's vertices were not written, or the polygon's do not
 *       fit); 7 vertices of the outline.  polygon_offsets_out int32 [max_regions + 1],
 *       polygon_vertices_out fp64 [max_polygon_vertices][2]: as O5, a polygon is written iff the polygons
 *       of rows 0 .. r together fit max_polygon_vertices.
 *       stats_out fp64 [8]: rows, polygons kept, their vertices, vertices written, rows dropped for
 *       overflow, too small, fewer than 3, invalid.
 *   Method: one workgroup per region.  S3 runs level by level: every undecided vertex carries the two ends
 *   of its chain, a chain takes its arg-max with one 64-bit atomicMax of (|cross| << 32 | ~position) at its
 *   start, the vertices on either side of a kept one take it as their new end, and rounds repeat until
 *   none splits (at most as many as vertices).  A scan of the keep flags (dp_points.h) lists the ring.
 *   S5 is all pairs of edges.  S6 is the LDS sort, chain and calipers that dp_cluster_shapes runs.
 *   resolution not finite or <= 0, min_area not finite or < 0, a negative capacity: DP_ERR_SHAPE.
 *
 * Mean height (dp_floor_mean_height): mean_out fp64 [2] on the device = (the mean y of the raster's
 * participants, rule 1 of "Occupancy floor plan"; their number).  No participants: height_threshold, as the
 * reference.  One fp64 sum in an unspecified order, one division.
 *
 * The polygons file (Python: export_floorplan_text) holds the reference's world coordinates:
 * shapely.affinity.scale with its default origin scales about the centre of the polygon's bounding box and
 * the translation adds the grid origin, X = cx + (x - cx) * resolution + min_x with cx the bounding-box
 * centre IN GRID UNITS, and likewise Z.  That is the reference's behaviour and is reproduced as it is; the
 * plain origin + x * resolution coordinates are in the JSON beside it.
 */
#define DP_OUTLINE_INT_COLUMNS 4
#define DP_OUTLINE_REAL_COLUMNS 2
#define DP_POLYGON_COLUMNS 8
int64_t dp_outline_workspace_size(int64_t max_cells, int64_t max_regions, int64_t max_vertices);
int dp_region_outlines(const int32_t* labels, const int32_t* dims, int32_t max_cells, const int32_t* n_regions_dev,
                       int32_t max_regions, int32_t max_vertices, int32_t* offsets_out, int32_t* vertices_out,
                       int64_t* columns_out, double* measures_out, double* stats_out, void* workspace,
                       int64_t workspace_bytes, dp_stream_t stream);
int dp_simplify_outlines(const int32_t* offsets, const int32_t* vertices, const int64_t* columns, const double* measures,
                         const int32_t* n_regions_dev, int32_t max_regions, int32_t max_vertices, double resolution,
                         double min_area, int32_t max_polygon_vertices, int32_t* polygon_offsets_out,
                         double* polygon_vertices_out, double* polygons_out, double* stats_out, void* workspace,
                         int64_t workspace_bytes, dp_stream_t stream);
int dp_floor_mean_height(const double* points, const int32_t* n_dev, int32_t n_max, double height_threshold,
                         double* mean_out, dp_stream_t stream);

/*
 * ---- Height-sliced floor plan (additive to ABI 20, csrc/dp_slices.hip, csrc/dp_outline.hip) ----------
 * The default mode of the reference's cleaned_pointcloud_to_floorplan.py, the one its CLI runs without
 * --height_threshold: create_height_slices (:149-170) cuts the levelled cloud into num_slices bands,
 * process_height_slice (:245-312) rasters each band at 0.05 m, closes it ONCE with a kernel whose size
 * get_optimal_closing_kernel_size (:214-243) derives from the raw grid, opens it 3 x 3, and
 * approximate_contour runs with alpha and min_area undivided.  The floor-plan sections' conventions hold:
 * fp64 points [n_max][3] with a device count n_dev (NULL: n_max; clamped to [0, n_max]), everything on the
 * caller's stream with no synchronisation and no host read-back, each fp64 operation rounded on its own (no
 * FMA), argument errors returned as DP_ERR_* before any launch, no kernel waits on another workgroup,
 * every loop is bounded by a count known when it starts, buffers have the caller's capacity and nothing is
 * written past it.  The block is additive: no existing entry point, layout or output changes, and
 * DP_ABI_VERSION stays 20.
 * Layout.  S = num_slices in [1, DP_SLICE_MAX].  Every per-cell buffer is [S][max_cells], max_cells the
 * capacity PER SLICE, S * max_cells <= 2^31 - 1 (else DP_ERR_SHAPE): slice s begins at the host-known
 * offset s * max_cells.  Its live size is dims[s] = (H, W), a device int32 [S][2]; its origin is
 * origin[s], a device fp64 [S][2].  So the stages behind the morphology are the existing entry points
 * (dp_grid_regions, dp_region_outlines, dp_simplify_outlines_with) called per slice on offset pointers.
 *   workspace  >= dp_slices_workspace_size(num_slices, max_cells) bytes of device memory, 8-byte aligned,
 *              owned by the call until the stream has passed it (content need not be initialised): about
 *              4.3 bytes per cell of all slices.  The three calls take the same size.
 *
 * Slice raster (dp_slice_grids): the grids of all S slices in two passes over the cloud.
 *   R1. Bounds, in fp64, as the reference writes them: h = (height_max - height_min) / S,
 *       lo_s = height_min + s * h, hi_s = lo_s + h, mid_s = (lo_s + hi_s) / 2.  bounds_out fp64 [S][3] =
 *       (lo_s, hi_s, mid_s).  height_min and height_max finite, height_max > height_min (else DP_ERR_SHAPE).
 *   R2. The participants of slice s are the finite live rows with y >= lo_s && y < hi_s, each slice's
 *       pair of comparisons evaluated on its own.  hi_s and lo_{s+1} may differ in the last bit, so a row
 *       may belong to two adjacent slices or to none, as in the reference; membership is never derived
 *       from one division.
 *   R3. Per slice, rules 2 to 5 of "Occupancy floor plan" with that slice's participants: minimum and
 *       maximum of x and z, padding, W and H by ceil, the cell by truncation, a row with gx >= W or gz >= H
 *       dropped and counted.  density_out uint32, height_out float32 (the largest (float)y of a cell's
 *       members, 0 in an empty cell, -0.0 counts as +0.0), occupied_out uint8; no colour output.
 *   R4. stats_out fp64 [S][8]: participants, dropped rows, occupied cells, H, W, status, 0, 0.  Status 1:
 *       fewer than min_points participants (the reference: 10), or none at all; the slice is skipped and
 *       its origin is (0, 0).  Status 2: W or H exceeds DP_FLOOR_MAX_DIM, or W * H > max_cells.  Under
 *       either status dims[s] = (0, 0) and no cell of that slice is written; the other slices are
 *       unaffected.  min_points < 0, resolution not finite or <= 0, padding not finite or < 0: DP_ERR_SHAPE.
 *   Method: pass 1 takes a row per lane and, for each slice with a row in the wave, reduces the keys of
 *   those rows over the wave (wave_minmax of dp_points.h); one lane adds the result to the workgroup's copy
 *   in LDS and the workgroup issues one set of global atomics per slice it has seen.  One thread per slice
 *   writes origin and dims.  Pass 2 is the raster's joining loop with the key (slice, cell): the slices
 *   present in a wave are taken one after the other, so two rows with the same x and z in different slices
 *   are never joined, and a row of two slices is rastered into both.  Without a colour there is no owner
 *   row, so the cell's key is the 32 ordered bits of (float)y, kept in height_out between pass 2 and the
 *   kernel that turns keys into heights.
 *
 * Closing sizes (dp_slice_closing_sizes), from the RAW binary grids (occupied_out, or any uint8 grids of
 * this layout, non-zero = set):
 *   C1. cells_s = the number of set cells of slice s; comps_s = the number of its 8-connected components
 *       (what skimage.measure.label counts by default on a 2-D array; scipy.ndimage.label with a 3 x 3
 *       structure of ones).  counts_out int64 [S][2] = (cells_s, comps_s).
 *   C2. close_size_out int32 [S]:  3 if comps_s == 0 or cells_s < 400 * comps_s, else 5 if cells_s <
 *       900 * comps_s, else 7 if cells_s < 1600 * comps_s, else 9 if cells_s < 2500 * comps_s, else 11.
 *       This is the reference's max(3, min(11, int(sqrt(mean) / 5))), made odd by adding 1, in exact 64-bit
 *       integers: int(sqrt(a) / 5) >= m holds exactly when cells >= 25 m^2 comps, and the mean's distance
 *       from such a threshold is 0 or at least 1 / comps, far above fp64's rounding, so no device sqrt is
 *       involved and nothing is within a tolerance (tests/test_slices.py pins the equivalence).
 *   Method: the union-find of dp_points.h over the stacked cell index s * max_cells + c, each set cell joined
 *   to its west, north-west, north and north-east neighbours inside its slice's dims; after the last union a
 *   cell is a root iff it is its own parent, and the roots are counted with one ballot and one atomic per
 *   wave (a wave's cells share their slice).  No table is built.
 *
 * Morphology with device sizes (dp_slice_morphology): rules 7 and 8 of "Occupancy floor plan" for all S
 * slices in one call.
 *   M1. The closing size of slice s is read ON THE DEVICE from close_size[s] (dp_slice_closing_sizes'
 *       output); a value that is not odd or not in [1, DP_FLOOR_MAX_KERNEL] is read as 1 (the identity).
 *   M2. close_iters (>= 0) and open_size (odd, in [1, DP_FLOOR_MAX_KERNEL]) are host values, else
 *       DP_ERR_SHAPE; the reference uses 1 and 3.  grid_out may be grid.
 *   Method: dp_grid_morphology's packed row and column passes with the slice in the launch grid's second
 *   dimension and the radius looked up per slice.  dp_grid_morphology itself is unchanged.
 *
 * Simplification parameters (dp_simplify_outlines_with, csrc/dp_outline.hip): dp_simplify_outlines, rule for
 * rule, with S1 and S2 taking their constants from the caller:
 *   S1'. area * (resolution * resolution) < area_floor: no polygon (drop reason 1).
 *   S2'. epsilon = alpha * perimeter.
 *   area_floor and alpha finite and >= 0 (else DP_ERR_SHAPE).  dp_simplify_outlines(min_area) is
 *   dp_simplify_outlines_with(min_area / 4, 0.005), bit for bit (a division by 4 is exact).  The default
 *   mode passes the reference's (0.1, 0.01).
 *
 * The polygons file of all slices (Python: export_sliced_floorplan_text) is save_floorplan_data's: one line
 * per kept polygon labelled with its slice's mid_s, slices in ascending height (the reference's sort is
 * stable and the slices arrive in ascending order), within a slice descending label (OpenCV lists contours
 * last-found first), coordinates as "Floor-plan polygons" states them.
 * Not built: plot_floorplan, its viridis colours and the combined background grid (they feed only the
 * plot); the reference's RANSAC floor plane (the cloud is already levelled by the ground stage); OpenCV's
 * final clean-up pass inside approxPolyDP (still unstated: S3's stated difference); random thinning;
 * batching the per-slice region, outline and simplify launches into one launch each (DESIGN.md section 19
 * has what the per-slice launches cost).
 */
#define DP_SLICE_MAX 32
int64_t dp_slices_workspace_size(int64_t num_slices, int64_t max_cells);
int dp_slice_grids(const double* points, const int32_t* n_dev, int32_t n_max, double height_min, double height_max,
                   int32_t num_slices, double resolution, double padding, int32_t min_points, int32_t max_cells,
                   uint32_t* density_out, float* height_out, uint8_t* occupied_out, int32_t* dims_out,
                   double* origin_out, double* bounds_out, double* stats_out, void* workspace,
                   int64_t workspace_bytes, dp_stream_t stream);
int dp_slice_closing_sizes(const uint8_t* grid, const int32_t* dims, int32_t num_slices, int32_t max_cells,
                           int32_t* close_size_out, int64_t* counts_out, void* workspace, int64_t workspace_bytes,
                           dp_stream_t stream);
int dp_slice_morphology(const uint8_t* grid, const int32_t* dims, int32_t num_slices, int32_t max_cells,
                        const int32_t* close_size, int32_t close_iters, int32_t open_size, uint8_t* grid_out,
                        void* workspace, int64_t workspace_bytes, dp_stream_t stream);
int dp_simplify_outlines_with(const int32_t* offsets, const int32_t* vertices, const int64_t* columns,
                              const double* measures, const int32_t* n_regions_dev, int32_t max_regions,
                              int32_t max_vertices, double resolution, double area_floor, double alpha,
                              int32_t max_polygon_vertices, int32_t* polygon_offsets_out, double* polygon_vertices_out,
                              double* polygons_out, double* stats_out, void* workspace, int64_t workspace_bytes,
                              dp_stream_t stream);

/*
 * ---- L-shape split (additive to ABI 20, csrc/dp_lshape.hip) -----------------------------------------
 * The end of the reference's fit_shapes_to_clusters: the rectangle list it builds from the cluster
 * shapes (the forced halving of a very large rectangle, split_large_rectangle :284-330, :387-396) and
 * `rectangles = detect_and_split_l_shapes(rectangles, points_2d)` (simple_pointcloud_viewer.py:79-282,
 * :410), which replaces a large rectangle that holds separate occupied parts by one rectangle per part.
 * The point-cloud sections' conventions hold: fp64 points [n_max][3], n_dev a device int32 (NULL: n_max;
 * clamped to [0, n_max]), n_max = 0, *n_dev = 0 and zero rectangles valid, everything on the caller's
 * stream with no synchronisation and no host read-back, each fp64 product, sum and difference rounded on
 * its own (no FMA), argument errors returned as DP_ERR_* before any launch.  sin and cos are the device's.
 * The block is additive: no existing entry point or layout changes, and DP_ABI_VERSION stays 20.
 * A rectangle row is fp64 [8]: centre u, centre v, width, height, angle in degrees, cluster, flags, 0,
 * in the frame u = -x, v = z of "Cluster shapes".  flags: 1 = a half of a forced split, + 2 = a part of an
 * L-shape split.
 *
 * Rectangle list (dp_shape_rectangles).  Reads shapes, the [max_clusters][16] table of dp_cluster_shapes,
 * rows c < K = min(*n_clusters_dev, max_clusters).  Each kind == 1 row, in cluster order, becomes one
 * rectangle (centre, width, height, angle of its columns 2..6, flags 0).  A row with width * height > 100
 * and count > 1000 becomes two, flags 1, with a = angle * pi / 180:
 *   width > height: d = width / 4:  (cu - d*cos a, cv - d*sin a, width / 2, height, angle), then
 *                                   (cu + d*cos a, cv + d*sin a, width / 2, height, angle);
 *   otherwise:      d = height / 4: (cu - d*sin a, cv + d*cos a, width, height / 2, angle), then
 *                                   (cu + d*sin a, cv - d*cos a, width, height / 2, angle).
 *   rects_out    fp64 [2 * max_clusters][8], the rows below *n_rects_dev written
 *   n_rects_dev  device int32: the number of rectangles
 *
 * Split (dp_lshape_split).  Input: the points, labels int32 [n_max] as dp_cluster_dbscan wrote them, a
 * rectangle list rects [max_rects][8] with its device count (clamped to [0, max_rects]).  The points that
 * take part are the reference's points_2d: the live rows with label >= -1 -- every DBSCAN participant,
 * noise and the members of other clusters included, not the rectangle's own cluster alone -- at u = -x,
 * v = z.  For each rectangle r = (cu, cv, w, h, angle, ...) of the list, in list order, with the
 * reference's constants:
 *   1. w * h < 10: kept (status 1).
 *   2. a = -angle * pi / 180, c = cos a, s = sin a.  A point is at x' = du*c - dv*s, y' = du*s + dv*c with
 *      du = u - cu, dv = v - cv (the reference's np.dot(centered, R.T)), and inside iff -w/2 < x' < w/2
 *      and -h/2 < y' < h/2: strict, as Polygon.contains is.
 *      Stated difference: the reference tests against cv2.boxPoints corners rounded to float32; this
 *      tests in the rectangle's own frame in fp64.
 *   3. Fewer than 50 points inside: kept (status 2).
 *   4. gw = (int)(w / 0.2) + 1, gh = (int)(h / 0.2) + 1 (saturated at 2^31 - 1).  gw <= 2 or gh <= 2: kept
 *      (status 3).  A side above DP_LSHAPE_MAX_SIDE: kept, error flag 1 (status 9).  Grids take their
 *      gw * gh cells from the capacity max_cells in list order, for every rectangle that passed rule 1 and
 *      the two side tests (whatever rule 3 says of it): once the grids up to and including r need more
 *      than max_cells, r and every later such rectangle is kept with error flag 1 (status 9).  Nothing is
 *      split from a truncated grid.
 *   5. An inside point sets cell gx = (int)((x' + w/2) / 0.2), gy = (int)((y' + h/2) / 0.2) when
 *      0 <= gx < gw and 0 <= gy < gh.  b = the set cells.
 *   6. Dilation by 2 x 2 ones with OpenCV's default anchor (1, 1):
 *      d[y][x] = b[y][x] | b[y][x-1] | b[y-1][x] | b[y-1][x-1], cells outside the grid reading 0.
 *   7. empty = !d.  Its 4-connected components with at least 6 cells form empty_mask.  None: kept
 *      (status 4).  ratio = (cells of empty_mask) / (gw * gh), one fp64 division; ratio < 0.2 or
 *      ratio > 0.6: kept (status 5).
 *   8. occupied = !empty_mask (smaller holes count as occupied, as in the reference).  Fewer than 2
 *      4-connected components of it: kept (status 6).
 *   9. Each occupied component with at least 6 cells, in row-major order of its first cell
 *      (scipy.ndimage.label's numbering; cv2.connectedComponents' own is not documented, and it only
 *      fixes the order of the output rows): its points are (x * 0.2 - w/2, y * 0.2 - h/2) over its cells;
 *      (sx, sy), sub_w, sub_h, sub_angle = their minimum-area rectangle by rules 2 and 3 of "Cluster
 *      shapes" (hull, calipers, ties to the smallest edge, angle folded into [0, 90)).
 *      Stated difference: cv2.minAreaRect works on float32 points with its own angle convention.
 *      The centre goes back as the reference writes it: ocx = (sx*c - sy*s) + cu, ocy = (sx*s + sy*c) + cv
 *      with the c and s of rule 2 -- np.dot(centre, rotation_matrix.T), the reference's
 *      rotation_matrix_inv taken literally, which turns by -angle a second time instead of turning back.
 *      angle' = fmod(sub_angle + angle, 180).  The part is listed iff sub_w * sub_h > 1.0.
 *  10. With L parts listed and S = the sum of their sub_w * sub_h in listed order: L < 2: kept (status 7);
 *      not 0.4 < S / (w * h) < 1.3: kept (status 8); otherwise the parts replace r (status 0), each
 *      (ocx, ocy, sub_w, sub_h, angle', r's cluster, r's flags + 2, 0).
 *   The reference's "largest empty region" loop (:201-208) computes a value nothing reads; it is left out.
 *   rects_out  fp64 [max_out][8]: the list in order, a replaced rectangle's parts in its place; a kept
 *              rectangle's row is copied as it came.  Offsets from a device scan of the per-rectangle counts.
 *   n_out_dev  device int32 [2]: rows written = min(rows, max_out); error word: 1 when rows > max_out (the
 *              rows past max_out are dropped), else 0.
 *   info_out   fp64 [max_rects][8], row r: status, points inside (0 under status 1), gw, gh (0 under
 *              status 1), cells of empty_mask (0 under status 1, 2, 3, 9), occupied components (0 under
 *              those and 4, 5), parts listed (0 unless status 0, 7, 8), error flag.
 *   workspace  >= dp_lshape_workspace_size(max_rects, max_cells) bytes of device memory, 8-byte aligned,
 *              owned by the call until the stream has passed it (content need not be initialised).  About
 *              29 bytes per cell and 130 per rectangle.
 *   n_max, max_rects, max_out or max_cells < 0: DP_ERR_SHAPE.
 *
 * Method.  One workgroup lists the candidates (rule 1) and scans the grid sizes into cell offsets: all
 * grids are ranges of one byte-per-cell array.  One pass over points x candidates: a workgroup keeps 64
 * candidates in LDS, rejects by the bounding circle before the rotation, counts the inside points by
 * wave ballots and stores the cell's byte.  Per-cell kernels over all grids at once do the dilation and
 * the two labellings with the union-find of dp_points.h (west and north links; a root is its component's
 * first cell), sizes by one atomic per cell.  The roots to fit are numbered by the flag scan of
 * dp_points.h.  One workgroup per component: a wave per grid row finds the row's leftmost and rightmost
 * member by ballots; the hull of those (at most 2 * DP_LSHAPE_MAX_SIDE = DP_SHAPES_H_MAX points) is the
 * component's, so one LDS chunk of the sort, chain and calipers that dp_cluster_shapes runs does it.
 * Bounds: no kernel waits on another workgroup; no thread loops over the points or over a grid (a wave
 * walks rows 64 cells at a time; the last kernel's threads walk their rectangles' parts).
 */
#define DP_LSHAPE_MAX_SIDE 1024
int dp_shape_rectangles(const double* shapes, const int32_t* n_clusters_dev, int32_t max_clusters,
                        double* rects_out, int32_t* n_rects_dev, dp_stream_t stream);
int64_t dp_lshape_workspace_size(int64_t max_rects, int64_t max_cells);
int dp_lshape_split(const double* points, const int32_t* labels, const int32_t* n_dev, int32_t n_max,
                    const double* rects, const int32_t* n_rects_dev, int32_t max_rects, int32_t max_out,
                    int32_t max_cells, double* rects_out, int32_t* n_out_dev, double* info_out, void* workspace,
                    int64_t workspace_bytes, dp_stream_t stream);

/* ---- Scale-invariant boundary metric (additive to ABI 20, csrc/dp_boundary.hip) ---------------------
 *
 * The edge counts behind SI_boundary_F1 and SI_boundary_Recall of the reference's
 * depth_pro/eval/boundary_metrics.py, and the edge maps themselves.  The counts are integers, so they
 * equal the reference's exactly; the scores are made from them on the host (depth_pro/eval).  fp32 with
 * IEEE division and denormals (no fast-math), no host synchronisation, no allocation, argument errors
 * returned as DP_ERR_* before any launch.
 *
 *   1. Input: pred is a float32 H x W depth with a row stride of ld_pred elements.  The target is a
 *      float32 depth (DP_BOUNDARY_DEPTH, the F1 case) or a uint8 0 / non-zero mask (DP_BOUNDARY_MASK, the
 *      recall case), ld_target in elements of its own type.
 *   2. Inverse depth: inv = 1.0f / (d < 1e-6f ? 1e-6f : d).  A NaN depth stays NaN (numpy's clip), +inf
 *      gives 0; -inf, 0 and negatives give 1e6.  With DP_BOUNDARY_INVERSE ORed into target_kind, pred and
 *      a depth target are inverse depths already and are used as they are (the reference's boundary_f1 and
 *      edge_recall_matting take those).
 *   3. Ratios, in the reference's return order (left, top, right, bottom): left = inv[y,x] / inv[y,x+1] and
 *      right = inv[y,x+1] / inv[y,x], both H x (W-1); top = inv[y,x] / inv[y+1,x] and bottom =
 *      inv[y+1,x] / inv[y,x], both (H-1) x W.  fp32 divisions: x / 0 is inf (an edge), 0 / 0 and anything
 *      with a NaN is no edge.
 *   4. Plain edge (fgbg_depth): (double)ratio > t, t a double.  The kernels compare ratio > f in fp32 with
 *      f the largest float32 <= t, which is the same predicate for every float32 ratio (dp_boundary.hip).
 *   5. Thinned edge (fgbg_depth_thinned): within each row of a horizontal map, of every maximal run of
 *      consecutive cells with ratio > t one cell stays, the first of the largest values; within each column
 *      of a vertical map the same, going down, the topmost of equal maxima.  Runs do not continue from one
 *      line into the next, a NaN ends a run, and of two infs in a run the first stays.
 *   6. Mask edges (fgbg_binary_mask) of a 0 / 1 mask m: left = m[y,x] & ~m[y,x+1], right = m[y,x+1] & ~m[y,x],
 *      top = m[y,x] & ~m[y+1,x], bottom = m[y+1,x] & ~m[y,x].
 *   7. counts[k][dir][0..2] = cells that are an edge of both images, of the target, of the prediction, for
 *      threshold k and direction dir.  DP_BOUNDARY_DEPTH: plain edges of both.  DP_BOUNDARY_MASK: thinned
 *      edges of the prediction, mask edges of the target (the same number for every k).
 *   8. The reference's edge_recall_matting compares ratio > np.float32(t) (a weak Python scalar), its
 *      boundary_f1 (double)ratio > t (an np.float64 scalar).  This library always does the second: the
 *      recall's caller passes (double)(float)t.
 *
 * dp_boundary_counts: all n_t thresholds (host array) in one call; counts (device, n_t * 12 uint64) is written
 *   whole.  dp_boundary_edges: maps = 4 planes of H * W bytes in the order of 3., map cell (y, x) at y * W + x,
 *   0 / 1, 0 outside each map's extent (the last column of left / right, the last row of top / bottom); plain
 *   edges, or thinned ones with thinned != 0.
 *   H, W in [1, DP_BOUNDARY_MAX_DIM] (1 x 1: every count is 0), n_t in [1, DP_BOUNDARY_MAX_T], ld >= W (else
 *   DP_ERR_SHAPE).  A null pointer, a threshold that is not finite, a target_kind other than the two kinds with
 *   or without the flag, a workspace below dp_boundary_workspace_size(H, W, n_t) (edges: n_t = 1) or not 4-byte
 *   aligned, counts not 8-byte aligned: DP_ERR_ARG.  The thinned passes cut every line into segments of
 *   DP_BOUNDARY_SEGMENT cells; the workspace holds two runs per segment, threshold and direction.
 */
#define DP_BOUNDARY_MAX_DIM 16384
#define DP_BOUNDARY_MAX_T   32
#define DP_BOUNDARY_DIRS    4     /* left, top, right, bottom */
#define DP_BOUNDARY_COUNTS  3     /* both, target, predicted */
#define DP_BOUNDARY_DEPTH   0     /* target: float32 depth, plain edges on both sides */
#define DP_BOUNDARY_MASK    1     /* target: uint8 0/1, prediction thinned */
#define DP_BOUNDARY_INVERSE 2     /* flag: the depths are inverse depths already */
#define DP_BOUNDARY_SEGMENT 64
int64_t dp_boundary_workspace_size(int32_t H, int32_t W, int32_t n_t);
int dp_boundary_counts(const float* pred, int64_t ld_pred, const void* target, int64_t ld_target, int32_t target_kind,
                       int32_t H, int32_t W, const double* thresholds /* host */, int32_t n_t,
                       uint64_t* counts /* device, [n_t][4][3], written whole */, void* ws, int64_t ws_bytes,
                       dp_stream_t stream);
int dp_boundary_edges(const float* depth, int64_t ld, int32_t H, int32_t W, double t, int32_t thinned,
                      uint8_t* maps /* device, 4 planes of H*W bytes, 0 outside each map's extent */, void* ws,
                      int64_t ws_bytes, dp_stream_t stream);

/*
 * ---- Triangle mesh (additive to ABI 20, csrc/dp_mesh.hip) -------------------------------------------
 * The reference's third meshing method, `--mesh_method simple` (create_simple_triangulated_mesh,
 * pointcloud_to_mesh.py:423-465), and the search under it: for every point of the down-sampled cloud the 6
 * nearest other points, the 5 triangles (i, n_j, n_j+1) over them, then remove_degenerate_triangles and
 * remove_duplicated_triangles.  The same search with k = 20 is get_average_point_distance (:397-421), from
 * which ball pivoting takes its radii.  The block is additive: no existing entry point or layout changes,
 * and DP_ABI_VERSION stays 20.  The point-cloud sections' conventions hold: fp64 points [n_max][3], n_dev a
 * device int32 (NULL: n_max; clamped to [0, n_max]), n_max = 0 and *n_dev = 0 valid, everything on the
 * caller's stream with no synchronisation and no host read-back, each fp64 product, sum and difference
 * rounded on its own (no FMA), argument errors returned as DP_ERR_* before any launch.  Rows at or beyond the
 * live count are neither read nor written.
 *   workspace  >= dp_mesh_workspace_size(n_max, t_max) bytes of device memory, 8-byte aligned, owned by the
 *              call until the stream has passed it (content need not be initialised).  A call on points
 *              needs (its n_max, 0), dp_mesh_clean_triangles (0, its t_max); a buffer sized for both serves
 *              every call.  About 85 bytes per point or 61 per triangle, whichever is more (the sort's
 *              workspace included).
 *   stats_out  fp64 [8], per call as listed below.
 * Open3D was not available to check against, so, as for dp_clean_stray and the oriented mesh points, the
 * numbered rules below are the specification (restated in tests/mesh_numpy.py, which is pinned to scipy's
 * cKDTree).
 * Not built: Poisson and ball-pivoting reconstruction (Open3D internals: their results depend on its octree
 * and on the order of its front), remove_duplicated_vertices (a no-op on a voxel grid's output) and
 * remove_non_manifold_edges (it removes triangles in the iteration order of an Open3D hash map, which cannot
 * be specified).
 *
 * Exact k nearest (dp_knn_exact).
 *   1. Participants are the finite live rows.  For row i the list holds the k participants j != i that are
 *      smallest by (d2, j), d2 = (dx*dx + dy*dy) + dz*dz -- the expression of dp_clean_stray and
 *      dp_knn_search.  k in [1, 64] (else DP_ERR_SHAPE).
 *   2. nbr_out        int32 [n_max][k]: row i's neighbours in ascending (d2, row) order, then -1
 *      nbr_count_out  int32 [n_max]: their number, min(k, participants - 1); 0 for a non-finite row
 *      d2_out         fp64 [n_max][k], may be NULL: the listed d2; entries past the count are not written
 *   3. cell_edge (finite and > 0, else DP_ERR_SHAPE) is the search grid's cell size: a speed parameter that
 *      never changes a list or a count.  The grid: per axis origin = the minimum over the participants, cell =
 *      floor((v - origin) / g) with g = cell_edge * (1 + 2^-20), clamped to [0, 2^21 - 2].
 *   4. The ring of row i is the smallest r >= 0 such that its list is full (k entries) and its largest d2 is
 *      strictly below (r * cell_edge) * (r * cell_edge) (fp64, r exact), or such that the cube of cells within
 *      Chebyshev distance r of row i's cell covers every participant's cell, whichever r is smaller.  It is
 *      the number of cell rings a walk outward from the row's cell has to take: with g above cell_edge, a
 *      cell further than r cells away holds no point that near.
 *   5. stats_out: finite rows, non-finite rows, finite rows with fewer than k neighbours, the largest ring
 *      of any finite row, error flag, 0, 0, 0.
 *   6. Error flag (device side): an axis would need more than 2^21 - 2 cells ((max - origin) / g).  Then every
 *      count is 0, every list -1, the third entry of stats_out the number of finite rows and the ring 0.
 *   7. Stated difference: Open3D's search_knn_vector_3d(p, k + 1) lists the query itself at position 0, which
 *      the reference drops; here the query is excluded by identity.  The two differ only for exact duplicate
 *      points, which a voxel grid never produces.  Open3D's order among equal distances is unspecified; here
 *      it is by row.
 * Method: dp_knn_search's grid (dp_sort_pairs on (cell, row), coordinates gathered into cell order, a run of
 * z-adjacent cells of one (x, y) cell row is one key range found by binary search).  One wave per query.
 * Ring r is the shell of cells at Chebyshev distance exactly r: the 8 r cell rows on the square's rim with
 * 2 r + 1 cells each, and two single cells for each of the (2 r - 1)^2 rows inside; the lanes take one range's
 * pair of binary searches each, the ranges' candidates are numbered by a prefix sum over the lanes and go 64
 * at a time through dp_knn_search's bitonic merge into a running best of one entry per lane.  The loop is
 * wave-uniform and ends after ring r by rule 4.  No scratch, no per-thread arrays, no LDS.
 * Bound: a query whose k-th neighbour lies R cells away visits O(R^2) cell rows (O(R^3) ranges) up to
 * R = 8; a query still open after ring 8 starts again over every participant in sorted order (n / 64 batches,
 * nearly all rejected by one comparison), so the work is bounded whatever the cloud and cell_edge are, and a
 * cell_edge far below the point spacing costs O(n^2 / 64).
 *
 * Mean neighbour distance (dp_mesh_mean_distance), from d2_out and nbr_count_out of a dp_knn_exact call.
 *   1. Per row with m > 0 listed neighbours: (sqrt(d2[0]) + sqrt(d2[1]) + ... + sqrt(d2[m-1])) / m, summed in
 *      list order.
 *   2. mean_out[0] = the sum of those over the rows with m > 0, divided by their number (0 without any);
 *      mean_out[1] = their number.  Order of the sum: 256 partial sums, partial t taking rows t, t + 256, ...
 *      in turn; within each group of 64 partials the butterfly v[l] += v[l ^ o] for o = 32, 16, ..., 1; the
 *      four groups' sums added in group order.
 *   3. Stated difference: get_average_point_distance averages over 1000 randomly sampled rows; this is its
 *      deterministic form over all of them.
 *
 * Fan (dp_mesh_fan), the reference's loop at :448-457, from the lists of a dp_knn_exact call.
 *   1. Row i with m = min(nbr_count[i], k) listed neighbours gives the triangles (i, nbr[i][j], nbr[i][j+1])
 *      for j = 0 .. m - 2, at slot i * (k - 1) + j of tri_out, int32 [n_max * (k - 1)][3]; the other slots
 *      of a live row are (-1, -1, -1).
 *   2. n_max * (k - 1) must be below 2^31 / 3 (else DP_ERR_SHAPE); k = 1 has no slots.
 *
 * Triangle clean-up (dp_mesh_clean_triangles): remove_degenerate_triangles, then remove_duplicated_triangles,
 * on a plain list tri_in int32 [t_max][3] with live count t_dev over n_vertices vertices.
 *   1. A triangle with an index outside [0, n_vertices) is dropped (`invalid`: how the fan's empty slots
 *      leave); of the others, one with two equal indices is dropped (`degenerate`).
 *   2. The canonical form of a triangle is its cyclic rotation with the smallest index first: (a, b, c),
 *      (b, c, a) and (c, a, b) are one triangle, (a, c, b) is another (the orientation is kept).
 *   3. Of the triangles sharing a canonical form the one at the smallest input position is kept, as it came
 *      (not rotated); the others count as `duplicated`.
 *   4. tri_out int32 [t_max][3] (not tri_in): the kept triangles in ascending input position; *t_out_dev their
 *      number; rows at or beyond it are not written.
 *   5. stats_out: input, invalid, degenerate, duplicated, kept, error flag (always 0: nothing can go wrong
 *      on the device), 0, 0.  Any n_vertices in [0, 2^31) works.
 * Method: three indices do not fit one 64-bit key above 2^21 vertices, so two stable passes of dp_sort_pairs
 * with the input position as payload: by the canonical third index, then by (first << 32) | second; dropped
 * triangles sort last.  A run's head is then its smallest position; the heads are flagged by position,
 * scanned (dp_points.h) and compacted.
 */
int64_t dp_mesh_workspace_size(int64_t n_max, int64_t t_max);
int dp_knn_exact(const double* points, const int32_t* n_dev, int32_t n_max, int32_t k, double cell_edge,
                 int32_t* nbr_out, int32_t* nbr_count_out, double* d2_out, double* stats_out, void* workspace,
                 int64_t workspace_bytes, dp_stream_t stream);
int dp_mesh_mean_distance(const double* d2, const int32_t* nbr_count, const int32_t* n_dev, int32_t n_max, int32_t k,
                          double* mean_out /* device, fp64 [2] */, void* workspace, int64_t workspace_bytes,
                          dp_stream_t stream);
int dp_mesh_fan(const int32_t* nbr, const int32_t* nbr_count, const int32_t* n_dev, int32_t n_max, int32_t k,
                int32_t* tri_out, dp_stream_t stream);
int dp_mesh_clean_triangles(const int32_t* tri_in, const int32_t* t_dev, int32_t t_max, int32_t n_vertices,
                            int32_t* tri_out, int32_t* t_out_dev, double* stats_out, void* workspace,
                            int64_t workspace_bytes, dp_stream_t stream);

/*
 * ---- Depth-warped views (ABI 20, additive; csrc/dp_effects.hip) ----------------------------------------------
 * The "3D effects" of the reference's OLD_SCRIPTS/depth_video_effect.py (3D_EFFECTS_README.md): the frames of its
 * parallax video (:10-111) and its red-cyan anaglyph (:113-183), from an RGB image and its depth map, both on the
 * device.  Everything on the caller's stream with no synchronisation and no host read-back; argument errors are
 * returned as DP_ERR_* before any launch (a null pointer, an unknown kind, a workspace that is too small or not
 * 4-byte aligned, bad_out not 8-byte aligned: DP_ERR_ARG; H or W outside [1, 16384], n_views outside
 * [1, DP_WARP_MAX_VIEWS]: DP_ERR_SHAPE).
 *   image      uint8 [H][W][3]          depth   float32 [H][W]
 *   workspace  >= dp_effects_workspace_size() bytes of device memory, 4-byte aligned, owned by the call until the
 *              stream has passed it (content need not be initialised)
 * The device does only IEEE add, subtract, multiply, divide and conversions, every one rounded on its own (no FMA),
 * so the bytes are those of NumPy >= 2 promotion (a Python float is weak, an np.float64 scalar is not):
 *   1. dn = (depth - min) / (max - min), every step in float32; min and max over the whole map.
 *   2. Maps, with x, y the integer pixel coordinates (per view descriptor {kind, a, b}, three doubles):
 *      DP_WARP_SHIFT      map_x = double(x) + a * double(1f - dn), map_y = double(y) + b * double(1f - dn), in fp64
 *                         (parallax `circle`: a = amplitude W cos t, b = amplitude H sin t; `swing`: a = amplitude W
 *                         sin t, b = 0; t = 2 pi frame / total_frames; cos and sin stay on the host, in numpy)
 *      DP_WARP_SHIFT_F32  map_x = double(x) + double(float32(a) * (1f - dn)), the product in float32; map_y = y; b is
 *                         not looked at (the anaglyph's views: a = +separation W for the left, - for the right)
 *      DP_WARP_ZOOM       map_x = double(x) + a * (double(x) - W / 2), map_y = double(y) + a * (double(y) - H / 2), in
 *                         fp64, a = 1 - zoom_factor = 1 - (1.0 + amplitude sin t); the depth is not read
 *      then clip(map_x, 0, W - 1), clip(map_y, 0, H - 1) and a cast to float32.
 *   3. Sampling: cv2.remap(INTER_LINEAR) on 8-bit pixels with float32 maps, OpenCV 4.x's published fixed-point rule:
 *      sx = rint_half_even(map_x * 32), ix = sx >> 5, fx = sx & 31, the same for y; the four weights
 *      32 (32 - fx | fx) (32 - fy | fy) sum to 32768; the result is (sum of w p + 16384) >> 15.  A tap outside the image
 *      counts as 0; after the clip it always has weight 0.  No cv2 binary was available to run against, so, as for
 *      dp_resize_u8_cv, parity with a cv2 binary is unpinned: tests/effects_numpy.py restates these rules and is
 *      checked against scipy.ndimage.map_coordinates.
 *   4. Anaglyph: channel 0 of the left view, channels 1 and 2 of the right view.
 * Stated differences from the reference:
 *   a. out[y][x] = sample(image, map_x[y][x], map_y[y][x]).  The reference passes map_x.T, map_y.T to cv2.remap; what
 *      it gets is the transpose of this image (and its video writer silently fails on a non-square frame).
 *   b. Non-finite depth is undefined in the reference.  Here min and max are taken over the finite depths, and a pixel
 *      whose map_x or map_y is not finite before the clip (NaN or inf depth; max == min, where dn = 0 / 0) is written
 *      as (0, 0, 0) and counted in bad_out.  DP_WARP_ZOOM has no such pixels.
 * dp_warp_views: views is a HOST array fp64 [n_views][3] (read during the call), out uint8 [n_views][H][W][3], bad_out
 * device int64 [n_views].  The depth is read once per pixel for all views.
 * dp_anaglyph: dx = separation * W (rounded to float32 here), out uint8 [H][W][3], bad_out device int64 [1]; one
 * fused pass, no intermediate views.
 */
#define DP_WARP_MAX_VIEWS 32
#define DP_WARP_SHIFT     0
#define DP_WARP_SHIFT_F32 1
#define DP_WARP_ZOOM      2
int64_t dp_effects_workspace_size(void);
int dp_warp_views(const uint8_t* image, const float* depth, int32_t H, int32_t W, const double* views, int32_t n_views,
                  uint8_t* out, int64_t* bad_out, void* workspace, int64_t workspace_bytes, dp_stream_t stream);
int dp_anaglyph(const uint8_t* image, const float* depth, int32_t H, int32_t W, double dx, uint8_t* out,
                int64_t* bad_out, void* workspace, int64_t workspace_bytes, dp_stream_t stream);

/*
 * ---- Depth shadows (ABI 20, additive; csrc/dp_shadows.hip) ---------------------------------------------------
 * The image-space depth-shadow tools of the reference's OLD_SCRIPTS/mesh_from_depth.py: find_depth_shadows (:1110-1170)
 * and the ground-plane fill of remove_depth_shadows (:1857-1944).  A depth map has no true value at a silhouette; the
 * pixels between foreground and background back-project to a sheet of points behind every object.  Everything runs on
 * the caller's stream as separate launches, with no synchronisation and no read-back.  Every entry point returns
 * DP_ERR_ARG before any launch for: a null pointer (depth_out of dp_depth_shadows alone may be null), h or w < 1,
 * h * w >= 2^31, a threshold_factor that is not finite, min_region_size < 0, a workspace that is null, not 8-byte
 * aligned or shorter than dp_shadows_workspace_size(h, w) (which returns 0 for a size it refuses).
 *   depth      float32 [h][w]      masks   uint8 [h][w] (0 / 1)      workspace   device memory, owned by the call until
 *   the stream has passed it, content need not be initialised
 *   stats_out  device fp64 [DP_SHADOW_STATS], written by every call (entries a call does not compute are 0):
 *     EDGE         pixels that are not free (dp_depth_edges, dp_depth_shadows: edge pixels)
 *     SHADOW       pixels of the output mask that are 1
 *     COMPONENTS   4-connected free components        KEPT      those with >= min_region_size pixels
 *     LARGEST      pixels of the largest component    GMAX      the gradient's maximum
 *     NONFINITE    depth pixels that are NaN or inf   ERROR     1 when NONFINITE > 0, else 0
 *     NONPOSITIVE  shadow pixels whose depth is <= 0 (dp_depth_shadows; the only pixels for which the reference goes on
 *                  to its cKDTree nearest-valid fill, which is not built)
 * dp_depth_gradient: np.sqrt(sobel(d, 1)**2 + sobel(d, 0)**2) with scipy.ndimage.sobel, bit for bit.  sobel on float32
 *   is two 1-D passes with mode='reflect' (the sample beyond an edge is the edge sample; a length-1 axis sees itself
 *   three times): the derivative [-1, 0, 1] along the axis, rounded to float32, then the smoothing [1, 2, 1] along the
 *   other axis, rounded to float32.  Each pass accumulates in fp64 in scipy's order: centre * weight first, then
 *   (left - right) * -1, or (left + right) * 1, added to it.  Then dx * dx, dy * dy, their sum and the square root in
 *   float32, each rounded on its own (no FMA, correctly rounded square root).  gmax_out: device float32 [1], the
 *   maximum over the frame (an atomicMax per workgroup on the bit pattern: non-negative floats order as integers).
 * dp_depth_edges: edge = (gmax > 0 ? g / gmax : g) > float32(threshold_factor), division and comparison in float32,
 *   the division correctly rounded (NumPy >= 2 compares a float32 array with a Python float in float32).  The reference's
 *   depth_threshold = threshold_factor * depth_map.mean() is dead code and is not computed; its Canny branch (image is
 *   not None) is not built, remove_depth_shadows never passes the image.
 *   Non-finite depth is outside the contract and defined: it is counted (NONFINITE), and such a frame has no edges,
 *   every pixel is free.  Nothing faults on it.
 * dp_region_filter: free_mask is any uint8 [h][w] (non-zero = free).  mask_out is 1 where the pixel is not free or its
 *   4-connected (scipy.ndimage.label's default cross, not the 3 x 3 square) free component has fewer than
 *   min_region_size pixels: the reference's ~np.isin(labels, valid_regions).  No numbering is produced.
 * dp_depth_shadows: the chain gradient, edges, region filter on ~edge.  depth_out, when not null, receives the depth
 *   with the shadow pixels set to NaN (dp_depth_to_points drops those: its valid test is d == d && d > 0).  Dropping
 *   them is this project's use of the mask; the reference fills them.
 * dp_fill_ground_shadows: the reference's fill for shadow pixels (shadow != 0) in the rows >= int(ground_rows * h)
 *   (the reference: 0.7), all in fp64 in the reference's evaluation order, stored rounded to float32; every other
 *   pixel is copied.  plane is a HOST array fp64 [4] = {n0, n1, n2, d} of n . p + d = 0, in the frame the formula
 *   assumes (camera axes, y down, unit normal; documented, not converted); cx = w / 2, cy = h / 2, f = max(w, h) are
 *   the reference's choices here, not the camera's.
 *     |n2| > 1e-6:                z = (-n0 x - n1 y - d) / n2 with x = (xi - cx) * 1.0 / f, y = (yi - cy) * 1.0 / f
 *     else |n0| > 1e-6:           DP_ERR_ARG (the reference's 100-step depth search is not built)
 *     else (horizontal plane):    z = (-d / n1) * f / den, den = yi - cy, replaced by 1e-6 where |den| < 1e-6
 *     z = max(z, 0.1).  filled_out: device int64 [1] (8-byte aligned), the pixels filled.  A plane or ground_rows that
 *     is not finite is DP_ERR_ARG.  No workspace.
 * Not built: detect_ground_plane / optimize_ground_plane (RANSAC, scipy's optimiser) and the cKDTree fill.
 */
#define DP_SHADOW_STATS            9
#define DP_SHADOW_STAT_EDGE        0
#define DP_SHADOW_STAT_SHADOW      1
#define DP_SHADOW_STAT_COMPONENTS  2
#define DP_SHADOW_STAT_KEPT        3
#define DP_SHADOW_STAT_LARGEST     4
#define DP_SHADOW_STAT_GMAX        5
#define DP_SHADOW_STAT_NONFINITE   6
#define DP_SHADOW_STAT_ERROR       7
#define DP_SHADOW_STAT_NONPOSITIVE 8
int64_t dp_shadows_workspace_size(int32_t h, int32_t w);
int dp_depth_gradient(const float* depth, int32_t h, int32_t w, float* grad_out, float* gmax_out, double* stats_out,
                      void* workspace, int64_t workspace_bytes, dp_stream_t stream);
int dp_depth_edges(const float* depth, int32_t h, int32_t w, double threshold_factor, uint8_t* edge_out,
                   double* stats_out, void* workspace, int64_t workspace_bytes, dp_stream_t stream);
int dp_region_filter(const uint8_t* free_mask, int32_t h, int32_t w, int32_t min_region_size, uint8_t* mask_out,
                     double* stats_out, void* workspace, int64_t workspace_bytes, dp_stream_t stream);
int dp_depth_shadows(const float* depth, int32_t h, int32_t w, double threshold_factor, int32_t min_region_size,
                     uint8_t* mask_out, float* depth_out, double* stats_out, void* workspace, int64_t workspace_bytes,
                     dp_stream_t stream);
int dp_fill_ground_shadows(const float* depth, const uint8_t* shadow, int32_t h, int32_t w, const double* plane,
                           double ground_rows, float* depth_out, int64_t* filled_out, dp_stream_t stream);

/*
 * ---- Point-cloud views (ABI 20, additive; csrc/dp_render.hip) -------------------------------------------------
 * Pictures of a cloud on the device: z-buffered square splats from up to DP_RENDER_MAX_VIEWS perspective cameras (the
 * reference's Open3D presets front / top / side / isometric of render_point_cloud_to_image and visualize_pointcloud)
 * and the orthographic top-down `plan` of pointcloud_pipeline.py's in_memory_pointcloud_visualization.  Everything runs
 * on the caller's stream as separate launches, with no synchronisation and no read-back.  The rule is DESIGN.md
 * section 22, restated in tests/render_numpy.py; all arithmetic is fp64 in the order written there, without FMA.
 *   points     fp64 [n][3]; the first *count rows are live (count: device int32, null = n); a row with a non-finite
 *              coordinate is counted and takes no part          colors   uint8 [n][3] or null (128, 128, 128)
 *   views      HOST fp64 [n_views][7] = front (3), up (3), zoom; read during the call
 *   plan       0: no plan view; 1: the plan of every finite row; 2: of the rows with y >= min_height.  The plan is the
 *              last view of the call.
 *   size       the splat's side in pixels, odd, 1 .. DP_RENDER_MAX_SIZE
 *   background HOST uint8 [6]: the perspective views' background, then the plan's
 *   tan_half_fov  tan(30 degrees) for the reference's 60 degree field of view, as the caller's libm gives it
 *   image_out  uint8 [n_views + (plan != 0)][H][W][3]; with sheet != 0 (exactly 4 views, no plan) uint8 [2H][2W][3]
 *              with view 0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right
 *   cameras_out  device fp64 [views][DP_RENDER_CAMERA_DOUBLES]: kind (0 perspective, 1 plan), degenerate, then for a
 *              perspective view eye [2..4], s [5..7], u [8..10], F [11..13], near, far, dist, extent, centre [18..20],
 *              t * (W / H), t; for the plan centre x', centre z, scale, y_top, min_height (NaN: none), (W - 1) / 2,
 *              (H - 1) / 2.  A degenerate view (no finite row, or an extent that is not > 0; the plan: no shown row) is
 *              all background.
 *   stats_out  device fp64 [DP_RENDER_STATS]: LIVE, NONFINITE, DEGENERATE, ERROR (1 when NONFINITE > 0), then per view
 *              at DP_RENDER_STAT_VIEWS + 4 v: drawn, clipped (the plan: below min_height), outside, covered pixels
 *   workspace  >= dp_render_workspace_size(W, H, size, views) bytes (0 for arguments it refuses), 8-byte aligned, owned
 *              by the call until the stream has passed it; dp_render_cameras uses the first 256 bytes only
 * DP_ERR_ARG before any launch: a null pointer (colors and count may be null; views when n_views = 0), n < 0, W or
 * H < 1, W * H >= 2^31, size even or outside 1 .. 15, n_views > 4 or no view at all, a front, up or zoom that is zero
 * or not finite, a zoom < 0, up parallel to front, a min_height (plan = 2) or tan_half_fov that is not finite, a sheet
 * without exactly four views, a workspace that is null, short or misaligned.
 */
#define DP_RENDER_MAX_VIEWS       4
#define DP_RENDER_MAX_SIZE        15
#define DP_RENDER_CAMERA_DOUBLES  24
#define DP_RENDER_STATS           24
#define DP_RENDER_STAT_LIVE       0
#define DP_RENDER_STAT_NONFINITE  1
#define DP_RENDER_STAT_DEGENERATE 2
#define DP_RENDER_STAT_ERROR      3
#define DP_RENDER_STAT_VIEWS      4
int64_t dp_render_workspace_size(int32_t W, int32_t H, int32_t size, int32_t n_views);
int dp_render_cameras(const double* points, const int32_t* count, int32_t n, const double* views, int32_t n_views,
                      int32_t plan, double min_height, int32_t W, int32_t H, double tan_half_fov, double* cameras_out,
                      double* stats_out, void* workspace, int64_t workspace_bytes, dp_stream_t stream);
int dp_render_points(const double* points, const uint8_t* colors, const int32_t* count, int32_t n, const double* views,
                     int32_t n_views, int32_t plan, double min_height, int32_t W, int32_t H, int32_t size,
                     const uint8_t* background, double tan_half_fov, int32_t sheet, uint8_t* image_out,
                     double* cameras_out, double* stats_out, void* workspace, int64_t workspace_bytes,
                     dp_stream_t stream);

/*
 * ---- Shape overlays on the plan view (ABI 20, additive; csrc/dp_overlay.hip) ----------------------------------
 * The last step of pointcloud_pipeline.py's in_memory_pointcloud_visualization (:172-230): the fitted rectangles and
 * circles stroked on the plan picture of dp_render_points, each with its number.  Strokes and labels are drawn on the
 * device from the tables that are already there; everything runs on the caller's stream as separate launches, with
 * no synchronisation and no read-back.  matplotlib's anti-aliased rasteriser is not the target: the rule below
 * defines the picture (restated in tests/overlay_numpy.py).  All arithmetic is fp64 in the
 * order written, every operation rounded on its own (no FMA), square root and division correctly rounded; sin and
 * cos are the device's, taken once per shape, and the records they go into are an output of the call.
 *
 * The rule.
 *   1. Frame.  Shapes live in the top-down frame u = -x, v = z of "Cluster shapes", the plan view's own x', z.  The
 *      camera is a plan record of dp_render_points (kind 1): cx = [2], cz = [3], scale = [4], hw = [7] = (W - 1) / 2,
 *      hh = [8] = (H - 1) / 2.  A point (u, v) is at X = (u - cx) * scale + hw, Y = hh - (v - cz) * scale; pixel (i, j)
 *      (column i, row j) is the point (i, j).  A camera whose kind is not 1, whose degenerate word is not 0, or with
 *      one of the five values not finite, is degenerate: nothing is listed, nothing is drawn, the error word is 2.
 *   2. The list.  nr = min(*n_rects_dev, max_rects) rectangles (rows of dp_shape_rectangles / dp_lshape_split, fp64
 *      [8]: cu, cv, w, h, angle in degrees, ...) in list order, then the nc rows of the shapes table (fp64 [16], rows
 *      below min(*n_clusters_dev, max_clusters)) whose kind [0] == 2, in table order, as circles (xc, yc, r) =
 *      columns 8..10.  A null count reads as the capacity, a negative one as 0; rows past the count are not read.
 *      Rectangle i is record i, carries the number i + 1 and the colour i mod 8 of the rectangle palette; the k-th
 *      circle is record nr + k, carries nr + k + 1 and the colour k mod 8 of the circle palette (palette entries
 *      8..15).
 *   3. Skipped.  A shape with a non-finite column among those five (three), or w, h or r < 0, or whose X, Y, a, b
 *      (R) or box half sides ex, ey below are not finite, is skipped: flags 8, every field but kind, colour and number 0, both boxes empty.
 *   4. Rectangle.  a = w * scale / 2, b = h * scale / 2, t = stroke / 2, c = cos(angle * pi / 180), s = sin(same)
 *      (pi = 3.14159265358979323846).  The rectangle is w x h, centred, turned by angle counter-clockwise in (u, v),
 *      which is clockwise in pixels.  For a pixel, dx = i - X, dy = j - Y, x' = dx * c - dy * s, y' = dx * s + dy * c:
 *      it is on the stroke iff |x'| <= a + t and |y'| <= b + t and not (|x'| < a - t and |y'| < b - t): mitred
 *      corners.  Stroke box: ex = |c| * (a + t) + |s| * (b + t), ey = |s| * (a + t) + |c| * (b + t),
 *      x0 = floor(X - ex), x1 = ceil(X + ex), y0 = floor(Y - ey), y1 = ceil(Y + ey).
 *   5. Circle.  R = r * scale, d2 = dx * dx + dy * dy, lo = max(R - t, 0): on the stroke iff lo * lo <= d2 and
 *      d2 <= (R + t) * (R + t).  Stroke box: x0 = floor(X - (R + t)), x1 = ceil(X + (R + t)), the same in y.
 *      A pixel outside a shape's stroke box is not on its stroke (the box is what the tiles are culled by).
 *   6. Blending.  A stroke pixel becomes out = (A * c + (255 - A) * p + 127) / 255 per channel, integer division.
 *      Per pixel: the rectangles in list order, then the circles; every covering shape blends in turn.
 *   7. Labels, after all strokes, in the same order.  label_scale = L = 0: none.  A number above 9999 has no label
 *      and is counted (flags 4).  Otherwise, with n digits: the block is (6 n - 1) L wide and 7 L high, its corner at
 *      lx = floor(X + 0.5) - ((6 n - 1) L) / 2, ly = floor(Y + 0.5) - (7 L) / 2 (integer division); the label box is
 *      the block grown by L on every side.  Every pixel of the box is blended with white at A = 179; then the pixel
 *      (lx + ox, ly + oy) of the block with column q = ox / L, digit q / 6 (most significant first), q % 6 = 5 being
 *      the gap, is set to the shape's colour where bit 4 - q % 6 of row oy / L of the digit's 5 x 7 bitmap
 *      (DP_OVERLAY_FONT) is set.
 *   8. A shape whose stroke box and label box both miss the picture [0, W - 1] x [0, H - 1] is off-screen: counted,
 *      never drawn.  flags: 1 the stroke box meets the picture, 2 the label box does, 4 label dropped, 8 skipped.
 *   records_out  device fp64 [max_rects + max_circles][DP_OVERLAY_RECORD_DOUBLES], the first nr + nc rows written:
 *                kind (1 rectangle, 2 circle), flags, X, Y, a (circle: R), b (0), c (1), s (0), colour r + 256 g +
 *                65536 b, number, stroke box x0 y0 x1 y1, label box x0 y0 x1 y1, digits, 0.  An empty box is 0 0 -1 -1.
 *   stats_out    device fp64 [DP_OVERLAY_STATS]: rectangles drawn, circles drawn (flags 1 or 2), skipped, off-screen,
 *                labels dropped, pixels painted (covered by a stroke or a label box), error word (1: a shape was
 *                skipped, 2: degenerate camera), 0.  The first four add up to nr + nc.
 *   image        uint8 [H][W][3], read and written in place; a 64 x 16 tile that no record touches is not written
 *   palette      HOST uint8 [16][3], read during the call      workspace  >= dp_overlay_workspace_size(max_rects,
 *                max_circles) bytes (0 for negative capacities), 8-byte aligned, owned by the call until the stream
 *                has passed it
 * Either list may be null with a capacity of 0 (max_circles = max_clusters).  DP_ERR_ARG before any launch: a null
 * image, camera, palette, records_out, stats_out or workspace, a null list with a capacity > 0, a double array that
 * is not 8-byte aligned or a count that is not 4-byte aligned, W or H < 1, W * H >= 2^31, stroke not finite or not
 * > 0, alpha outside 0..255, label_scale outside 0..DP_OVERLAY_MAX_LABEL_SCALE, a negative capacity, capacities
 * that add up to 2^31 or more, a workspace that is short or misaligned.
 */
#define DP_OVERLAY_RECORD_DOUBLES   20
#define DP_OVERLAY_STATS            8
#define DP_OVERLAY_MAX_LABEL_SCALE  8
#define DP_OVERLAY_LABEL_ALPHA      179
/* the ten digits, 5 x 7, row by row from the top, bit 4 = the leftmost column */
#define DP_OVERLAY_FONT {{14, 17, 19, 21, 25, 17, 14}, {4, 12, 4, 4, 4, 4, 14}, {14, 17, 1, 2, 4, 8, 31}, \
                         {31, 2, 4, 2, 1, 17, 14}, {2, 6, 10, 18, 31, 2, 2}, {31, 16, 30, 1, 1, 17, 14}, \
                         {6, 8, 16, 30, 17, 17, 14}, {31, 1, 2, 4, 8, 8, 8}, {14, 17, 17, 14, 17, 17, 14}, \
                         {14, 17, 17, 15, 1, 2, 12}}
int64_t dp_overlay_workspace_size(int64_t max_rects, int64_t max_circles);
int dp_overlay_shapes(uint8_t* image, int32_t W, int32_t H, const double* camera_dev, const double* rects,
                      const int32_t* n_rects_dev, int32_t max_rects, const double* shapes, const int32_t* n_clusters_dev,
                      int32_t max_clusters, const uint8_t* palette, double stroke, int32_t alpha, int32_t label_scale,
                      double* records_out, double* stats_out, void* workspace, int64_t workspace_bytes,
                      dp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DP_MI355X_H */
