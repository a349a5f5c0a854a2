"""The folded-LayerNorm path of dp_gemm (dp_gemm_args.ln_*) and dp_layernorm_stats at their documented
contract (include/dp_mi355x.h) edges, against fp64 -- the companion of test_gemm_contract.py, whose
constants and conventions (header-derived expected_rc, per-element bound, canaries, CPU self-check
with seeded mutations) it takes over.

Operations and their references (fp64 over the exact upcast of every 16-bit / fp32 operand):

  producer      x' = (A . B^T + bias) * gamma + x, x = the fp32 C (fp32 producer) or hi + q 2^(e - S)
                (split producer).  |x' - ref| <= 2^-23 |ref| + (K + 16) 2^-24 S, S the same formula on
                absolute values (test_gemm_contract's bound).  With an fp32 C present the 16-bit rows
                are exactly its rounding and the int8 low part exactly ops.split_residual of it; with
                C = NULL merge_residual(hi', lo') meets the bound plus half a step 2^(e' - S) (1.5
                steps where q' = 127, the clamped tie; 2^-25 for a subnormal f16 hi', whose step is
                finer than its rounding error) and is a fixed point of split(merge(.)) -- but for
                q' = -128 under an odd hi', which decodes to an exact 16-bit tie and re-encodes from
                the even neighbour, at most one step away (a property of the encoding, not of a kernel).
                part is then compared with the statistics of merge(hi', lo'), q = that error away
                from the x' they were taken of: + q on the mean, + 128 (2 Dm q + q^2) on M2.
  part          (mean, M2) of each 128-column chunk of the STORED rows, vs fp64.  u = 2^-24,
                D = max |x - x_first| over the chunk, first = the chunk's first column (the shift):
                  GEMM epilogue (one pass, shifted): d_i = x_i - shift (1 rounding), s1 = sum d_i
                  and s2 = sum d_i^2 over 32 sequential adds and 2 cross-lane ones (depth 34),
                  mean = shift + s1 / 128, M2 = s2 - s1 * (s1 / 128):
                    |mean err| <= u |mean| + (1 + 34 + 1) u D                    = u |mean| + 36 u D
                    |M2 err|   <= (3 + 34) u 128 D^2 [s2] + 2 * 35 u 128 D^2 [s1^2 / 128]
                                  + 2 u 128 D^2 [the product and the difference]  = 109 * 128 u D^2
                  dp_layernorm_stats (two passes): sum over a depth-7 tree (3 in the lane, 4 across),
                  mean = s / 128, M2 = sum (x_i - mean)^2 over the same tree, X = max |x|,
                  Dm = max |x - mean|:
                    |mean err| <= 7 u X
                    |M2 err|   <= (3 + 7) u 128 Dm^2 + 128 (7 u X)^2
                (both times 1.01 for the second-order terms).
  rs            (rstd, -rstd * mean) vs fp64 from the `part` values the same launch wrote (as data):
                mean = sum of 8 / 8 (depth 3): dmean = 3 u max |mean_c|; d_c = mean_c - mean;
                M2 = sum (M2_c + 128 d_c^2): dM2 = 256 dmean sum |d_c| + 1024 dmean^2 + 10 u M2;
                var = M2 / 1024 + eps: dvar = dM2 / 1024 + u (var + eps);
                |rstd err| <= rstd (dvar / (2 (var + eps)) + u + RSQRT_ALLOWANCE), and for the product
                |mean| * that + rstd dmean + u |rstd mean|.
  consumer      v = rstd * acc - rstd * mean * colsum[n] + bias[n], act(v), 16-bit store; (mean, rstd)
                merged in fp64 from the part values handed to the kernel (or the rs values, as data):
                  |out - ref| <= u_out |ref| + L (rstd (K + 16) 2^-24 (|xb| |B|^T + |mean| |colsum|)
                                 + |bias| 2^-23 + |rstd err| |acc - mean colsum| + rstd dmean |colsum|)
                L = 1.13 with GELU (its Lipschitz constant) else 1, plus LN_GELU_ALLOWANCE with GELU.

No element is left out of a comparison.  Canaries: 64 elements before and after every output, the
[N, ld) padding and two rows past M, on C, xb / hi, xl, part and rs; all bit-identical after the call.

The CPU self-check shows that an fp32 restatement of the header's formulas meets every bound with
both allowances at 0, and that each seeded mutation of it fails at least one case.
"""

import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gemm_contract as gc
from depth_pro import _lib, ops
from depth_pro._lib import DP_ACT_GELU, DP_ACT_NONE, DP_ACT_RELU

DTYPES = gc.DTYPES
DT_IDS = ["bf16", "f16"]
OK, ERR_ARG, ERR_SHAPE, ERR_ALIGN, ERR_DTYPE = gc.OK, gc.ERR_ARG, gc.ERR_SHAPE, gc.ERR_ALIGN, 1003
MARGIN, PAT16, U_OUT, N_TILES = gc.MARGIN, gc.PAT16, gc.U_OUT, gc.N_TILES
PAT8 = 0x5A
U32 = 2.0 ** -24
EPS = float(np.float32(1e-6))              # the value the kernels see
S_OF = {torch.bfloat16: 16, torch.float16: 19}
T_8PH320, T_P8PH = _lib.DP_TILE_8PH_320x256, _lib.DP_TILE_P8PH_256x256
WS_RS_OFFSET = 4096                        # the persistent consumer's merged statistics: the workspace's first partial slot

# rsqrtf is a hardware approximation (v_rsq_f32) whose error cannot be derived from the format.  Measured on
# MI355X over every rs this module checks (ln_rs_out of the split producers and the pre-pass of the persistent
# consumers, both dtypes): the largest value of (|rstd - ref| - bound) / ref with the allowance at 0 was -8.8e-8
# (split_256x1024x1024_noC_rs), i.e. no rstd exceeds the derived bound and the measured excess is 0.
RSQRT_EXCESS_MEASURED = 0.0
RSQRT_ALLOWANCE = 2.0 * RSQRT_EXCESS_MEASURED
# gelu_erf (x * sigmoid(odd polynomial)) behind the folded consumer: the largest |out - ref| - bound over the
# GELU consumers of this module with the allowance at 0, same machine: 1.088e-5 (f16, c_641x512_gelu, on the
# all-zero rows, where v = bias[n] and the derived bound is little more than the f16 rounding of the result; within
# gelu_erf's stated 2.6e-5).  bf16: -2.5e-7 (none over the bound).  Without GELU: -1.1e-7 (f16), -9.6e-7 (bf16).
LN_GELU_EXCESS_MEASURED = 1.088e-5
LN_GELU_ALLOWANCE = 2.0 * LN_GELU_EXCESS_MEASURED


# ============================================================================ 1. return codes (host)
def _lc(name, *presets, **kw):
    c = dict(name=name, M=320, N=1024, K=1024, lda=None, ldc=None, act=DP_ACT_NONE, acc=False, c32=False,
             c_null=False, gamma=False, part_out=False, xb_out=False, xl=False, rs_out=False, part_in=False,
             rs_in=False, colsum=False, eps=1e-6, ws=False)
    for p in presets:
        c.update(p)
    c.update(kw)
    return c


P32 = dict(part_out=True, xb_out=True, acc=True, c32=True)          # the fp32 producer
SPL = dict(xl=True, xb_out=True, acc=True, c32=True)                # the split producer
RSO = dict(SPL, part_out=True, rs_out=True, ws=True)                # ... with merged row statistics
CON = dict(part_in=True, colsum=True)                               # a consumer
CRS = dict(rs_in=True, colsum=True)


def _rc_cases():
    cs = [_lc("p32_ok", P32), _lc("split_ok", SPL), _lc("split_ok_cnull_part", SPL, c_null=True, part_out=True),
          _lc("rso_ok", RSO), _lc("con_ok", CON), _lc("con_ok_ws", CON, ws=True), _lc("con_rs_ok", CRS),
          _lc("con_gelu_ok", CON, act=DP_ACT_GELU),
          # each missing or extra producer field
          _lc("p32_no_part", P32, part_out=False), _lc("p32_no_xb", P32, xb_out=False),
          _lc("p32_c_null", P32, c_null=True), _lc("split_no_xb", SPL, xb_out=False),
          _lc("rs_out_alone", acc=True, c32=True, rs_out=True, ws=True),
          # a producer together with a consumer
          _lc("p32_and_consumer", P32, CON), _lc("split_and_colsum", SPL, colsum=True),
          _lc("consumer_and_xb", CON, xb_out=True),
          # producers with an activation, without accumulate, with a 16-bit C
          _lc("p32_relu", P32, act=DP_ACT_RELU), _lc("p32_gelu", P32, act=DP_ACT_GELU),
          _lc("split_relu", SPL, act=DP_ACT_RELU), _lc("p32_no_acc", P32, acc=False),
          _lc("split_no_acc", SPL, acc=False), _lc("p32_c16", P32, c32=False), _lc("split_c16", SPL, c32=False),
          _lc("p32_c16_no_acc", P32, c32=False, acc=False), _lc("split_c16_no_acc", SPL, c32=False, acc=False),
          # split producer: ldc, the extent limit on both sides (M = 1: ldc alone sets M * ldc * 4)
          _lc("split_ldc_4", SPL, ldc=1028), _lc("split_ldc_8", SPL, ldc=1032),
          _lc("split_extent_below", SPL, M=1, ldc=2 ** 30 - 72), _lc("split_extent_at", SPL, M=1, ldc=2 ** 30 - 64),
          # consumer
          _lc("con_both_stats", CON, rs_in=True), _lc("con_no_stats", colsum=True),
          _lc("con_no_colsum", part_in=True), _lc("con_rs_no_colsum", rs_in=True), _lc("con_gamma", CON, gamma=True),
          _lc("con_relu", CON, act=DP_ACT_RELU), _lc("con_c32", CON, c32=True),
          _lc("con_c32_acc", CON, c32=True, acc=True), _lc("con_eps_0", CON, eps=0.0),
          _lc("con_eps_neg", CON, eps=-1e-6), _lc("con_eps_nan", CON, eps=float("nan")),
          _lc("con_rs_eps_0", CRS, eps=0.0), _lc("con_ldc_4", CON, N=256, ldc=260),
          _lc("con_p8_32768", CON, ws=True, M=32768, N=256), _lc("con_p8_32769", CON, ws=True, M=32769, N=256),
          # ln_rs_out
          _lc("rso_no_xl", P32, rs_out=True, ws=True), _lc("rso_no_part", RSO, part_out=False),
          _lc("rso_no_ws", RSO, ws=False), _lc("rso_eps_0", RSO, eps=0.0),
          _lc("rso_M_163520", RSO, M=163520, K=64), _lc("rso_M_163521", RSO, M=163521, K=64)]
    for N in (128, 256, 384, 1024):
        cs += [_lc(f"p32_N{N}", P32, N=N, K=64), _lc(f"split_N{N}", SPL, N=N, K=64), _lc(f"con_N{N}", CON, N=N)]
    for N in (256, 512, 2048):
        cs.append(_lc(f"rso_N{N}", RSO, N=N, K=64))
    for K in (512, 1024, 2048):
        cs += [_lc(f"con_K{K}", CON, K=K, N=256), _lc(f"con_rs_K{K}", CRS, K=K, N=256)]
    return cs


RC_CASES = _rc_cases()


def expected_ln_rc(c, tile):
    """(return code, planned tile or None) of dp_gemm_plan for an ln_* launch, from include/dp_mi355x.h:
    the general checks, 'What a launch with an ln_* field must meet', the ABI-13 paragraph, the 8-column rules."""
    M, N, K = c["M"], c["N"], c["K"]
    lda, ldc = c["lda"] or K, c["ldc"] or N
    c16 = not c["c32"]
    # the general checks
    if K % 64 or N % 4:
        return ERR_SHAPE, None
    if lda % 8 or ldc % 4:
        return ERR_ALIGN, None
    if c["c_null"] and not c["xl"]:
        return ERR_ARG, None
    if c["acc"] and c16:
        return ERR_DTYPE, None
    prod = c["part_out"] or c["xb_out"] or c["xl"] or c["rs_out"]
    cons = c["part_in"] or c["colsum"] or c["rs_in"]
    eps_ok = c["eps"] > 0                                   # False for NaN
    ws_ok = c["ws"]
    if prod and cons:
        return ERR_ARG, None
    if prod and not c["xl"] and not (c["part_out"] and c["xb_out"] and c["acc"] and c["c32"] and not c["c_null"]
                                     and c["act"] == DP_ACT_NONE):
        return ERR_ARG, None
    if c["xl"] and not (c["xb_out"] and c["acc"] and c["c32"] and c["act"] == DP_ACT_NONE and ldc % 8 == 0
                        and M * ldc * 4 < 2 ** 32 - 256):
        return ERR_ARG, None
    if cons and not (c["colsum"] and (c["part_in"] != c["rs_in"]) and K == 1024 and eps_ok and not c["gamma"]
                     and c["act"] in (DP_ACT_NONE, DP_ACT_GELU) and c16 and not c["acc"]):
        return ERR_ARG, None
    if c["rs_out"] and not (c["xl"] and c["part_out"] and N == 1024 and eps_ok and ws_ok and -(-M // 320) <= 511):
        return ERR_ARG, None
    if N % 256:                                             # every ln_* launch: what DP_TILE_8PH_320x256 takes
        return ERR_ARG, None
    if c["rs_in"] and tile not in (0, T_P8PH):
        return ERR_ARG, None
    if tile not in (0, T_8PH320) and not (cons and tile == T_P8PH):
        return ERR_ARG, None
    if c16 and ldc % 8:                                     # the 8-column rules, whatever the hint
        return ERR_ALIGN, None
    if c["rs_in"]:
        return OK, T_P8PH
    if tile == T_P8PH:                                      # a part_in consumer: rerouted without a place for rs
        return OK, T_P8PH if (ws_ok and M <= 32768) else T_8PH320
    if tile == T_8PH320 or prod:
        return OK, T_8PH320
    return OK, None                                         # a part_in consumer under AUTO: either engine


_DUMMY = torch.zeros(64, dtype=torch.float32)               # an aligned address the planner never dereferences


def ln_args(c, tile):
    dt = torch.bfloat16
    A = torch.empty(8, dtype=dt)
    C = torch.empty(8, dtype=torch.float32 if c["c32"] else dt)
    a = ops._gemm_args(A, A, C, M=c["M"], N=c["N"], K=c["K"], lda=c["lda"], ldc=c["ldc"], act=c["act"],
                       accumulate=c["acc"], gamma=_DUMMY if c["gamma"] else None, tile=tile)
    p = _DUMMY.data_ptr()
    if c["c_null"]:
        a.C = None
    for key in ("part_out", "xb_out", "xl", "rs_out", "part_in", "rs_in", "colsum"):
        if c[key]:
            setattr(a, "ln_" + key, p)
    a.ln_eps = c["eps"]
    if c["ws"]:
        a.workspace, a.workspace_bytes = p, int(_lib.load().dp_gemm_workspace_size())
    return a


@pytest.mark.parametrize("ci", range(len(RC_CASES)), ids=[c["name"] for c in RC_CASES])
def test_plan_rejects_exactly_what_the_header_says(ci):
    """Host only: dp_gemm_plan's code for every (ln_* case, hint 0..23) == the header-derived predicate."""
    c = RC_CASES[ci]
    for tile in range(N_TILES):
        a = ln_args(c, tile)
        t, g = ctypes.c_int32(-1), ctypes.c_int32(-1)
        rc = _lib.load().dp_gemm_plan(ctypes.byref(a), ctypes.byref(t), ctypes.byref(g))
        want, want_tile = expected_ln_rc(c, tile)
        assert rc == want, f"{c['name']} tile {tile}: plan {rc}, header {want}"
        if rc == OK and want_tile is not None:
            assert t.value == want_tile, f"{c['name']} tile {tile}: planned on {t.value}, header says {want_tile}"
        if rc == OK:
            assert t.value in (T_8PH320, T_P8PH)
    assert c["name"].split("_")[-1] != "ok" or expected_ln_rc(c, 0)[0] == OK


def test_rc_table_covers_both_sides():
    """The table holds accepted and rejected launches of each kind (a predicate that always says ARG passes nothing)."""
    codes = {expected_ln_rc(c, 0)[0] for c in RC_CASES}
    assert codes == {OK, ERR_ARG, ERR_ALIGN, ERR_DTYPE}
    by = {c["name"]: expected_ln_rc(c, 0)[0] for c in RC_CASES}
    assert by["split_extent_below"] == OK and by["split_extent_at"] == ERR_ARG
    assert by["rso_M_163520"] == OK and by["rso_M_163521"] == ERR_ARG
    assert by["p32_N128"] == ERR_ARG and by["p32_N256"] == OK and by["split_N384"] == ERR_ARG
    assert by["con_K512"] == ERR_ARG and by["con_K1024"] == OK and by["con_rs_K2048"] == ERR_ARG
    assert expected_ln_rc(RC_CASES[[c["name"] for c in RC_CASES].index("con_p8_32769")], T_P8PH) == (OK, T_8PH320)


def _stats_rc_cases():
    """(name, kwargs overriding a valid call, expected code) for dp_layernorm_stats, from its header paragraph."""
    cs = [(f"cols_{n}", dict(cols=n), ERR_SHAPE) for n in (128, 256, 768, 1536, 4096)]
    cs += [("rows_0", dict(rows=0), ERR_SHAPE), ("ldx_mod4", dict(ldx=1026), ERR_ALIGN),
           ("ldxb_mod8", dict(ldxb=1028), ERR_ALIGN), ("x_misaligned", dict(x=4), ERR_ALIGN),
           ("xb_misaligned", dict(xb=2), ERR_ALIGN), ("xl_misaligned", dict(xl=1), ERR_ALIGN),
           ("part_misaligned", dict(part=4), ERR_ALIGN), ("dtype_f32", dict(dtype=2), ERR_DTYPE),
           ("x_null", dict(x=None), ERR_ARG), ("xb_null", dict(xb=None), ERR_ARG), ("part_null", dict(part=None), ERR_ARG)]
    return cs


def _stats_call(base, kw):
    """dp_layernorm_stats with `base` as every pointer, byte offsets / NULLs / sizes from kw."""
    ptr = lambda k: None if (k in kw and kw[k] is None) else base + kw.get(k, 0)   # noqa: E731
    cols = kw.get("cols", 1024)
    return _lib.load().dp_layernorm_stats(ptr("x"), kw.get("ldx", cols), kw.get("rows", 4), cols, ptr("xb"),
                                          kw.get("ldxb", cols), ptr("xl"), ptr("part"), kw.get("dtype", 0), None)


@pytest.mark.parametrize("case", _stats_rc_cases(), ids=[c[0] for c in _stats_rc_cases()])
def test_layernorm_stats_rejections(case):
    """Host only: every documented rejection of dp_layernorm_stats comes before any launch (dummy pointers)."""
    _, kw, want = case
    assert _stats_call(_DUMMY.data_ptr(), kw) == want


# ===================================================================== 2. inputs, model, references
FAMILIES = ["generic", "out7", "out0", "out128", "outN128", "chunkconst", "const", "mean100", "zero"]
CHUNK_VALUES = [-8.0, 3.0, 0.5, 12.0, -1.0, 6.0, -4.0, 2.0]      # exact in bf16 and f16; far apart


def family_rows(M, W, g, dev):
    """[M][W] fp32 rows, row r of family FAMILIES[r % 9].  `dev`: the deviation of the mean-100 rows, 100 +- dev
    alternating by column (every chunk's mean is exactly 100).  16 bits hold 100 +- dev exactly for dev = 2^-3 in
    f16 (spacing 2^-4 in [64, 128)) but not in bf16 (spacing 2^-1): rows that become 16-bit operands take dev = 2^-1
    for bf16; fp32 / split streams take 2^-3 (hi = 100, 64 steps of 2^-9 in bf16)."""
    x = torch.randn(M, W, generator=g) * 2 + torch.randn(M, 1, generator=g)
    fam = [FAMILIES[r % len(FAMILIES)] for r in range(M)]
    col = torch.arange(W)
    for r, f in enumerate(fam):
        if f == "out7":
            x[r, 7] += 40.0
        elif f == "out0":
            x[r, 0] += 40.0
        elif f == "out128":
            x[r, 128] += 40.0
        elif f == "outN128":
            x[r, W - 128] += 40.0
        elif f == "chunkconst":
            x[r] = torch.tensor(CHUNK_VALUES)[(col // 128 + r) % 8]
        elif f == "const":
            x[r] = 3.25
        elif f == "mean100":
            x[r] = 100.0 + dev * (1.0 - 2.0 * (col % 2))
        elif f == "zero":
            x[r] = 0.0
    return x, fam


def split_host(x, dt, mut=None):
    """ops.split_residual, restated so that it can be mutated."""
    s = S_OF[dt] + (1 if mut == "s_off_by_one" else 0)
    hi = x.to(dt)
    hf = hi.float()
    e = torch.frexp(x if mut == "exp_from_x" else hf).exponent
    q = torch.nan_to_num(torch.round(torch.ldexp(x - hf, (s - e).float())), nan=0.0, posinf=1e9, neginf=-1e9)
    q = torch.remainder(q + 128, 256) - 128 if mut == "q_not_clamped" else q.clamp(-128, 127)     # (an int8 wrap)
    return hi, q.to(torch.int8)


def chunk_stats64(x):
    c = x.double().reshape(x.shape[0], -1, 128)
    mu = c.mean(-1)
    return torch.stack((mu, ((c - mu[..., None]) ** 2).sum(-1)), -1)          # [M][nch][2]


def part_bounds(x, impl):
    """Per-chunk (mean, M2) error bounds for the stored fp32 rows x (module docstring)."""
    c = x.double().reshape(x.shape[0], -1, 128)
    mu = c.mean(-1)
    if impl == "gemm":
        D = (c - c[..., :1]).abs().amax(-1)
        bm, bq = U32 * mu.abs() + 36 * U32 * D, 109 * 128 * U32 * D * D
    else:
        X, Dm = c.abs().amax(-1), (c - mu[..., None]).abs().amax(-1)
        bm, bq = 7 * U32 * X, 10 * 128 * U32 * Dm * Dm + 128 * (7 * U32 * X) ** 2
    return torch.stack((bm, bq), -1) * 1.01


def rs_reference(part, allowance=RSQRT_ALLOWANCE):
    """fp64 (rstd, -rstd * mean) from fp32 part [M][8][2] as data, their bounds, and (mean, dmean)."""
    p = part.double()
    mc, qc = p[..., 0], p[..., 1]
    mean = mc.mean(1)
    d = mc - mean[:, None]
    M2 = (qc + 128 * d * d).sum(1)
    var = M2 / 1024
    rstd = (var + EPS) ** -0.5
    dmean = 3 * U32 * mc.abs().amax(1)
    dM2 = 256 * dmean * d.abs().sum(1) + 1024 * dmean ** 2 + 10 * U32 * M2
    dvar = dM2 / 1024 + U32 * (var + EPS)
    b_rstd = rstd * (0.5 * dvar / (var + EPS) + U32 + allowance)
    b_nm = mean.abs() * b_rstd + rstd * dmean + U32 * (rstd * mean).abs()
    return dict(rstd=rstd, nm=-rstd * mean, b_rstd=b_rstd, b_nm=b_nm, mean=mean, dmean=dmean)


def merge_model(part, mut=None):
    """The header's Chan merge in fp32: [M][2] (rstd, -rstd * mean)."""
    mc, qc = part[..., 0], part[..., 1]
    mean = mc.sum(1) * 0.125
    d = mc - mean[:, None]
    M2 = qc.sum(1) if mut == "merge_no_between_term" else (qc + 128.0 * d * d).sum(1)
    var = M2 / (1023.0 if mut == "var_over_1023" else 1024.0)
    rstd = torch.rsqrt(var + (0.0 if mut == "eps_omitted" else np.float32(1e-6)))
    return torch.stack((rstd, -rstd * mean), 1)


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.int8}[t.element_size()])


class Region:
    """[rows][cols] inside a flat allocation: MARGIN + off elements before, rows of ld, two rows past, MARGIN after."""

    def __init__(self, rows, cols, ld, off, dtype):
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        self.base = MARGIN + off
        self.numel = self.base + (rows + 2) * ld + MARGIN
        self.idx = (self.base + torch.arange(rows)[:, None] * ld + torch.arange(cols)[None, :]).reshape(-1)

    def fresh(self, body=None):
        if self.dtype == torch.float32:
            buf = torch.full((self.numel,), float("nan"), dtype=torch.float32)
        elif self.dtype == torch.int8:
            buf = torch.full((self.numel,), PAT8, dtype=torch.int8)
        else:
            buf = torch.full((self.numel,), PAT16, dtype=torch.int16).view(self.dtype)
        if body is not None:
            buf[self.idx] = body.reshape(-1).to(self.dtype)
        return buf

    def body(self, buf):
        return buf[self.idx].reshape(self.rows, self.cols)

    def canaries_changed(self, buf):
        keep = torch.ones(self.numel, dtype=torch.bool)
        keep[self.idx] = False
        return int((_bits(buf)[keep] != _bits(self.fresh())[keep]).sum())


# ------------------------------------------------------------------------------------- producers
def _pc(name, kind, M, N, K, **kw):
    c = dict(name=name, kind=kind, M=M, N=N, K=K, bias=True, gamma=True, C=True, part=True, rs=False, strides=False,
             edges=None)
    c.update(kw)
    return c


PCASES = [
    _pc("p32_1x256x64", "p32", 1, 256, 64),
    _pc("p32_319x512x128_nobias", "p32", 319, 512, 128, bias=False),
    _pc("p32_321x256x192", "p32", 321, 256, 192),
    _pc("p32_257x1024x64_nobias", "p32", 257, 1024, 64, bias=False, gamma=False),
    _pc("p32_320x256x128_strides", "p32", 320, 256, 128, strides=True),
    _pc("split_2x256x64_edges", "split", 2, 256, 64, gamma=False, edges="all"),
    _pc("split_15x512x128_noC_edges", "split", 15, 512, 128, gamma=False, C=False, edges="no_overflow"),
    _pc("split_255x256x192_nopart", "split", 255, 256, 192, part=False),
    _pc("split_256x1024x1024_noC_rs", "split", 256, 1024, 1024, bias=False, C=False, rs=True),
    _pc("split_320x512x64_strides", "split", 320, 512, 64, strides=True),
    _pc("split_1x1024x128_rs", "split", 1, 1024, 128, rs=True),
    _pc("split_321x1024x64_noC_rs", "split", 321, 1024, 64, C=False, rs=True),
    _pc("split_641x1024x64_rs_nobias", "split", 641, 1024, 64, bias=False, rs=True),
    _pc("split_257x1024x64_noC_nopart", "split", 257, 1024, 64, C=False, part=False),
]
PCASE_IDS = [c["name"] for c in PCASES]


def edge_elements(dt):
    """(hi, q, bias) per element for the split-residual edges; x' = bias + (hi + q step) exactly (A = 0, gamma 1).
    U = ulp of the 16-bit type in [1, 2)."""
    U = 2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -10
    return [
        (1.0, 0, U / 2),             # exact tie: hi' = 1 (even), x' - hi' = +128 steps -> q' clamped to 127
        (-1.0, 0, -U / 2),           # its mirror: hi' = -1, q' = -128 (representable: not clamped)
        (1.0, 0, 1.5 * U),           # tie between 1 + U (odd) and 1 + 2U: hi' = 1 + 2U, q' = -128
        (1.0, 0, -1.0),              # hi' = 0, q' = 0
        (1.0, 0, 1.0 - U / 8),       # x' = 2 - U/8 -> hi' = 2 from below: e' = 2 where frexp(x') gives 1; q' = -16
        (1.0, 0, 1.0 + U / 4),       # x' = 2 + U/4 -> hi' = 2 from above; q' = 32
        (1.5, 37, 1.0),              # hi' in the next binade up from hi
        (1.5, -90, -0.75),           # hi' in the next binade down
        (1.0, 127, U / 2),           # an old low part carried into the sum
        (0.0, 0, 3.25 * 2.0 ** -24), # f16: a subnormal hi' = 3 * 2^-24 whose step 2^-41 saturates q' at 127
        (0.0, 0, -2.0 ** -20),       # f16: a subnormal hi' hit exactly (q' = 0)
        (32768.0, 0, 32752.0),       # x' = 65520: the f16 tie that rounds to +inf (bf16: 65536 - 16, q' = -8)
    ]


OVERFLOW_COL = 11                   # index of the last edge element


class PProblem:
    pass


@functools.lru_cache(maxsize=None)
def pproblem(ci, dt):
    c = PCASES[ci]
    g = torch.Generator().manual_seed(7000 + ci)
    M, N, K = c["M"], c["N"], c["K"]
    P = PProblem()
    P.c, P.dt, P.M, P.N, P.K = c, dt, M, N, K
    x, fam = family_rows(M, N, g, 2.0 ** -3)
    A = torch.randn(M, K, generator=g)
    for r, f in enumerate(fam):
        if f in ("chunkconst", "const", "mean100", "zero"):
            A[r] = 0.0                                  # x' = bias * gamma + x there (= x without a bias)
    P.B = (torch.randn(N, K, generator=g) * K ** -0.5).to(dt)
    P.bias = torch.randn(N, generator=g) if c["bias"] else None
    P.gamma = (0.1 + 0.05 * torch.randn(N, generator=g)) * (1 - 2 * (torch.arange(N) % 3 == 0).float()) if c["gamma"] else None
    P.edge_row = None
    if c["edges"]:
        el = edge_elements(dt)
        n_el = len(el) - (1 if c["edges"] == "no_overflow" else 0)
        P.edge_row, P.edge_n = M - 1, n_el
        A[M - 1] = 0.0
        k = torch.arange(N) % n_el
        P.bias = torch.tensor([e[2] for e in el], dtype=torch.float32)[k]
        P.edge_hi = torch.tensor([e[0] for e in el], dtype=torch.float32)[k].to(dt)
        P.edge_q = torch.tensor([e[1] for e in el], dtype=torch.int8)[k]
    P.A = A.to(dt)
    if c["kind"] == "split":
        P.hi0, P.lo0 = split_host(x, dt)
        if c["edges"]:
            P.hi0[M - 1], P.lo0[M - 1] = P.edge_hi, P.edge_q
        P.x = ops.merge_residual(P.hi0, P.lo0)          # exactly what the kernel reads
    else:
        P.x = x
    s = 8 if c["strides"] else 0
    P.lda, P.ldb, P.ldc, P.off = K + s, K + 2 * s, N + s, s
    nch = N // 128
    P.rC = Region(M, N, P.ldc, P.off, torch.float32) if c["C"] else None
    P.rhi = Region(M, N, P.ldc, P.off, dt)
    P.rlo = Region(M, N, P.ldc, P.off, torch.int8) if c["kind"] == "split" else None
    P.rpart = Region(M, 2 * nch, 2 * nch, 0, torch.float32) if c["part"] else None
    P.rrs = Region(M, 2, 2, 0, torch.float32) if c["rs"] else None
    return P


def p_prefill(P):
    """The output allocations before the call."""
    o = {}
    if P.rC is not None:
        o["C"] = P.rC.fresh(P.x if P.c["kind"] == "p32" else None)     # the split producer never reads C
    o["hi"] = P.rhi.fresh(P.hi0 if P.c["kind"] == "split" else None)
    if P.rlo is not None:
        o["lo"] = P.rlo.fresh(P.lo0)
    if P.rpart is not None:
        o["part"] = P.rpart.fresh()
    if P.rrs is not None:
        o["rs"] = P.rrs.fresh()
    return o


@functools.lru_cache(maxsize=None)
def p_reference(ci, dt):
    """fp64 x' and its accumulation bound."""
    P = pproblem(ci, dt)
    A, B = P.A.double(), P.B.double()
    v, S = A @ B.t(), A.abs() @ B.abs().t()
    if P.bias is not None:
        v, S = v + P.bias.double(), S + P.bias.double().abs()
    if P.gamma is not None:
        v, S = v * P.gamma.double(), S * P.gamma.double().abs()
    ref, S = v + P.x.double(), S + P.x.double().abs()
    return ref, (P.K + 16) * U32 * S


def p_model(P, mut=None):
    """An fp32 evaluation of the header's producer formulas (or a seeded mutation): the allocations after the call."""
    c, dt = P.c, P.dt
    o = p_prefill(P)
    v = P.A.float() @ P.B.float().t()
    if P.bias is not None:
        v = v + P.bias
    if P.gamma is not None:
        v = v * P.gamma
    xn = v + P.x
    if P.rC is not None:
        o["C"][P.rC.idx] = xn.reshape(-1)
    if c["kind"] == "split":
        hi, lo = split_host(xn, dt, mut)
        if mut != "hi_not_updated":
            o["hi"][P.rhi.idx] = hi.reshape(-1)
        o["lo"][P.rlo.idx] = lo.reshape(-1)
        stored = xn if P.rC is not None else ops.merge_residual(hi, lo)
    else:
        o["hi"][P.rhi.idx] = xn.to(dt).reshape(-1)
        stored = xn
    part = None
    if P.rpart is not None:
        ch = xn.reshape(P.M, -1, 128)                 # one pass, shifted by the chunk's first value
        d = ch - ch[..., :1]
        s1, s2 = d.sum(-1), (d * d).sum(-1)
        part = torch.stack((ch[..., 0] + s1 * (1.0 / 128), s2 - s1 * (s1 * (1.0 / 128))), -1)
        if mut == "part_chunk_off_by_one":
            part = part.roll(1, 1)
        o["part"][P.rpart.idx] = part.reshape(-1)
    if P.rrs is not None:
        o["rs"][P.rrs.idx] = merge_model(part, mut).reshape(-1)
    return o, stored


def p_verify(P, ci, o, rsq_allow=RSQRT_ALLOWANCE):
    """Failures (strings) and figures of a producer's allocations `o` after the call."""
    c, dt = P.c, P.dt
    ref, b_acc = p_reference(ci, dt)
    fails, fig = [], {}
    split = c["kind"] == "split"
    hi = P.rhi.body(o["hi"])
    lo = P.rlo.body(o["lo"]) if split else None
    fin16 = torch.isfinite(hi.float())               # False only at the f16 overflow edge
    if P.rC is not None:
        Cn = P.rC.body(o["C"])
        ex = (Cn.double() - ref).abs() - (2.0 ** -23 * ref.abs() + b_acc)
        fig["x_new excess"] = float(torch.nan_to_num(ex, nan=float("inf")).max())
        if not bool((ex <= 0).all()):
            fails.append(f"C: {int((~(ex <= 0)).sum())} elements over the bound, excess {fig['x_new excess']:.3e}")
        if not torch.equal(_bits(hi), _bits(Cn.to(dt))):
            fails.append(f"xb != the 16-bit rounding of the stored C at {int((_bits(hi) != _bits(Cn.to(dt))).sum())} elements")
        if split:
            want = ops.split_residual(Cn, dt)[1]
            same = (lo == want) | ~fin16
            if not bool(same.all()):
                fails.append(f"xl != split_residual(stored C) at {int((~same).sum())} elements")
        stored, q_chunk = Cn, None
    else:
        merged = ops.merge_residual(hi, lo)
        e = torch.frexp(hi.float()).exponent
        step = torch.ldexp(torch.ones_like(merged), (e - S_OF[dt]).float()).double()
        q_err = torch.where(lo == 127, 1.5, 0.5) * step
        if dt == torch.float16:                      # a subnormal hi': the 16-bit rounding error itself
            q_err = torch.where(hi.float().abs() < 2.0 ** -14, torch.full_like(q_err, 2.0 ** -25), q_err)
        ex = (merged.double() - ref).abs() - (2.0 ** -23 * ref.abs() + b_acc + q_err)
        fig["x_new excess"] = float(torch.nan_to_num(ex, nan=float("inf")).max())
        if not bool((ex <= 0).all()):
            fails.append(f"merge(hi', lo'): {int((~(ex <= 0)).sum())} elements over the bound, excess {fig['x_new excess']:.3e}")
        # a fixed point of split(merge(.)) -- except that q' = -128 under an odd hi' (x' - hi' within half a step
        # of -ulp / 2, not a tie) decodes to the exact tie between hi' and its neighbour, which re-encodes from
        # the even neighbour (127 steps back, or 64 doubled ones across a binade): the same number to one step
        h2, l2 = ops.split_residual(merged, dt)
        same = (_bits(h2) == _bits(hi)) & (l2 == lo)
        near = (lo == -128) & ((ops.merge_residual(h2, l2).double() - merged.double()).abs() <= step)
        if not bool((same | near).all()):
            fails.append(f"(hi', lo') is not a fixed point of split_residual(merge_residual(.)) at {int((~(same | near)).sum())} elements")
        stored, q_chunk = merged, q_err.reshape(P.M, -1, 128).amax(-1)
    if P.edge_row is not None:                       # x' = bias + x exactly: the encoding bit for bit
        r = P.edge_row
        xe = P.bias + P.x[r]
        he, le = ops.split_residual(xe, dt)
        ok = torch.equal(_bits(hi[r]), _bits(he)) and bool(((lo[r] == le) | ~fin16[r]).all())
        if not ok:
            bad = ((_bits(hi[r]) != _bits(he)) | ((lo[r] != le) & fin16[r])).nonzero().reshape(-1)[:6].tolist()
            fails.append(f"edge row: (hi', lo') != the encoding of bias + x at columns {bad}")
        if dt == torch.float16 and c["edges"] == "all":      # pinned: the f16 overflow edge
            k = torch.arange(P.N) % P.edge_n == OVERFLOW_COL
            if not (bool((hi[r][k].float() == float("inf")).all()) and bool((lo[r][k] == -128).all())):
                fails.append("f16 overflow edge: expected hi' = +inf with q' = -128")
        elif not bool(fin16.all()):
            fails.append("a non-finite 16-bit value outside the f16 overflow edge")
    elif not bool(fin16.all()):
        fails.append("a non-finite 16-bit value")
    part = None
    if P.rpart is not None:
        part = P.rpart.body(o["part"]).reshape(P.M, -1, 2)
        b_part = part_bounds(stored, "gemm")
        if q_chunk is not None:      # the statistics are of x', the stored rows are its encoding: |x' - stored| <= q
            cs = stored.double().reshape(P.M, -1, 128)
            Dm = (cs - cs.mean(-1, keepdim=True)).abs().amax(-1)
            b_part = b_part + torch.stack((q_chunk, 128 * (2 * Dm * q_chunk + q_chunk ** 2)), -1)
        ex = (part.double() - chunk_stats64(stored)).abs() - b_part
        fig["part excess"] = float(torch.nan_to_num(ex, nan=float("inf")).max())
        if not bool((ex <= 0).all()):
            fails.append(f"part: {int((~(ex <= 0)).sum())} values over the bound, excess {fig['part excess']:.3e}")
    if P.rrs is not None:
        rs = P.rrs.body(o["rs"])
        fails += rs_check(rs, part, fig, rsq_allow)
    for k, reg in (("C", P.rC), ("hi", P.rhi), ("lo", P.rlo), ("part", P.rpart), ("rs", P.rrs)):
        if reg is not None and reg.canaries_changed(o[k]):
            fails.append(f"{k}: {reg.canaries_changed(o[k])} canaries changed")
    return fails, fig


def rs_check(rs, part, fig, rsq_allow=RSQRT_ALLOWANCE):
    """rs [M][2] against fp64 from the part [M][8][2] of the same launch; fig gets the allowance-free relative excess."""
    R = rs_reference(part, 0.0)
    e0 = ((rs[:, 0].double() - R["rstd"]).abs() - R["b_rstd"]) / R["rstd"]
    fig["rstd relative excess"] = max(fig.get("rstd relative excess", float("-inf")),
                                      float(torch.nan_to_num(e0, nan=float("inf")).max()))
    R = rs_reference(part, rsq_allow)
    bad0 = ~((rs[:, 0].double() - R["rstd"]).abs() <= R["b_rstd"])
    bad1 = ~((rs[:, 1].double() - R["nm"]).abs() <= R["b_nm"])
    if bool(bad0.any()) or bool(bad1.any()):
        return [f"rs: {int(bad0.sum())} rstd and {int(bad1.sum())} -rstd*mean over the bound "
                f"(rstd relative excess without allowance {fig['rstd relative excess']:.3e})"]
    return []


# ------------------------------------------------------------------------------------- consumers
def _cc(name, M, N, act, strides=False):
    return dict(name=name, M=M, N=N, K=1024, act=act, strides=strides)


CCASES = [_cc("c_15x256_none", 15, 256, DP_ACT_NONE), _cc("c_1x256_gelu", 1, 256, DP_ACT_GELU),
          _cc("c_2x512_none", 2, 512, DP_ACT_NONE), _cc("c_255x256_gelu", 255, 256, DP_ACT_GELU),
          _cc("c_256x256_none", 256, 256, DP_ACT_NONE), _cc("c_257x512_gelu", 257, 512, DP_ACT_GELU),
          _cc("c_319x256_none", 319, 256, DP_ACT_NONE), _cc("c_320x256_gelu", 320, 256, DP_ACT_GELU),
          _cc("c_321x256_none_strides", 321, 256, DP_ACT_NONE, True), _cc("c_641x512_gelu", 641, 512, DP_ACT_GELU)]
CCASE_IDS = [c["name"] for c in CCASES]


class CProblem:
    pass


@functools.lru_cache(maxsize=None)
def cproblem(ci, dt):
    c = CCASES[ci]
    g = torch.Generator().manual_seed(9000 + ci)
    M, N, K = c["M"], c["N"], c["K"]
    P = CProblem()
    P.c, P.dt, P.M, P.N, P.K = c, dt, M, N, K
    x, P.fam = family_rows(M, K, g, 0.5 if dt == torch.bfloat16 else 2.0 ** -3)
    P.xb = x.to(dt)                                          # the un-normalised 16-bit rows (A)
    P.part = chunk_stats64(P.xb).float()                     # handed to the kernel: data
    w = torch.randn(N, K, generator=g) * K ** -0.5
    P.B = w.to(dt)
    # the fp32 master weights sit 0.24 ulp above their 16-bit rounding, all on one side: a colsum summed
    # over them instead of over B is off by 0.24 sum ulp(B)
    Bf = P.B.float()
    ulp = torch.ldexp(torch.ones_like(Bf), (torch.frexp(Bf).exponent - (8 if dt == torch.bfloat16 else 11)).float())
    P.w32 = Bf + 0.24 * ulp * (Bf != 0)                                  # (0.48 of the finer ulp just below a power of two)
    assert torch.equal(P.w32.to(dt), P.B)
    P.colsum = P.B.double().sum(1).float()
    P.bias = torch.randn(N, generator=g) * 0.5
    s = 8 if c["strides"] else 0
    P.lda, P.ldb, P.ldc, P.off = K + s, K + 2 * s, N + s, s
    P.rC = Region(M, N, P.ldc, P.off, dt)
    return P


def c_products(P):
    """fp64 xb . B^T and |xb| . |B|^T, computed once per problem."""
    if not hasattr(P, "_prod"):
        xb, B = P.xb.double(), P.B.double()
        P._prod = (xb @ B.t(), xb.abs() @ B.abs().t())
    return P._prod


def c_reference(P, rs=None, rsq_allow=RSQRT_ALLOWANCE):
    """(ref, bound) in fp64; rs: [M][2] fp32 statistics handed over as data
    (else merged in fp64 from P.part)."""
    acc, absacc = c_products(P)
    cs, bias = P.colsum.double(), P.bias.double()
    kf = (P.K + 16) * U32
    if rs is None:
        R = rs_reference(P.part, rsq_allow)
        rstd, mean = R["rstd"][:, None], R["mean"][:, None]
        v = rstd * (acc - mean * cs) + bias
        pre = rstd * kf * (absacc + mean.abs() * cs.abs()) + bias.abs() * 2.0 ** -23 + \
            R["b_rstd"][:, None] * (acc - mean * cs).abs() + rstd * R["dmean"][:, None] * cs.abs()
    else:
        r0, r1 = rs[:, :1].double(), rs[:, 1:2].double()
        v = r0 * acc + r1 * cs + bias
        pre = kf * (r0.abs() * absacc + r1.abs() * cs.abs()) + bias.abs() * 2.0 ** -23
    gelu = P.c["act"] == DP_ACT_GELU
    ref = F.gelu(v) if gelu else v
    return ref, U_OUT[P.dt] * ref.abs() + (1.13 if gelu else 1.0) * pre


def c_model(P, mut=None, rs=None):
    """An fp32 evaluation of the header's consumer formula (or a seeded mutation): the C allocation after the call."""
    part = P.part
    if mut == "consumer_chunk_off_by_one":           # chunks 1 .. 8 of the flat array instead of 0 .. 7
        flat = part.reshape(-1, 2)
        part = torch.cat((flat[1:], flat[-1:])).reshape(part.shape)
    if mut == "stats_of_neighbour_row":              # row min(m + 1, M - 1)'s statistics
        part = part[torch.clamp(torch.arange(P.M) + 1, max=P.M - 1)]
    r = merge_model(part, mut) if rs is None else rs
    colsum = P.w32.double().sum(1).float() if mut == "colsum_unrounded" else P.colsum
    acc = P.xb.float() @ P.B.float().t()
    nm = -r[:, 1:2] if mut == "mean_sign_flipped" else r[:, 1:2]
    v = r[:, :1] * acc + (nm * colsum + P.bias)
    if P.c["act"] == DP_ACT_GELU:
        v = F.gelu(v)
    buf = P.rC.fresh()
    buf[P.rC.idx] = v.to(P.dt).reshape(-1)
    return buf


def c_verify(P, buf, rs=None, gelu_allow=LN_GELU_ALLOWANCE, rsq_allow=RSQRT_ALLOWANCE):
    ref, bound = c_reference(P, rs, rsq_allow)
    out = P.rC.body(buf).double()
    ex = (out - ref).abs() - bound
    worst = float(torch.nan_to_num(ex, nan=float("inf")).max())
    lim = gelu_allow if P.c["act"] == DP_ACT_GELU else 0.0
    fails = []
    if not bool((ex <= lim).all()):
        rows = sorted({P.fam[r] for r in (~(ex <= lim)).any(1).nonzero().reshape(-1).tolist()})
        fails.append(f"C: {int((~(ex <= lim)).sum())} elements over the bound, excess {worst:.3e}, row families {rows}")
    if P.rC.canaries_changed(buf):
        fails.append(f"C: {P.rC.canaries_changed(buf)} canaries changed")
    return fails, worst


# ------------------------------------------------------------------------- dp_layernorm_stats cases
SCASES = [dict(name="s_c512_r7_xl", cols=512, rows=7, xl=True, pad=False), dict(name="s_c512_r9", cols=512, rows=9, xl=False, pad=False),
          dict(name="s_c2048_r5_xl", cols=2048, rows=5, xl=True, pad=False), dict(name="s_c2048_r10", cols=2048, rows=10, xl=False, pad=False),
          dict(name="s_c1024_r13_xl_ld", cols=1024, rows=13, xl=True, pad=True), dict(name="s_c512_r1_ld", cols=512, rows=1, xl=False, pad=True)]


class SProblem:
    pass


@functools.lru_cache(maxsize=None)
def sproblem(ci, dt):
    c = SCASES[ci]
    g = torch.Generator().manual_seed(8000 + ci)
    P = SProblem()
    P.c, P.dt, P.M, P.N = c, dt, c["rows"], c["cols"]
    P.x, _ = family_rows(P.M, P.N, g, 2.0 ** -3)
    if P.M > 1:                                              # the encoding's edges as fp32 inputs
        U = 2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -10
        P.x[1, :8] = torch.tensor([1 + U / 2, -1 - U / 2, 1 + 1.5 * U, 2 - U / 8, 2 + U / 4, 3.25 * 2.0 ** -24, 0.0, -2.0 ** -20])
    pad = c["pad"]
    P.ldx, P.ldxb = P.N + (4 if pad else 0), P.N + (8 if pad else 0)
    nch = P.N // 128
    P.rx = Region(P.M, P.N, P.ldx, 4 if pad else 0, torch.float32)
    P.rhi = Region(P.M, P.N, P.ldxb, 8 if pad else 0, dt)
    P.rlo = Region(P.M, P.N, P.ldxb, 8 if pad else 0, torch.int8) if c["xl"] else None
    P.rpart = Region(P.M, 2 * nch, 2 * nch, 0, torch.float32)
    return P


def s_model(P, mut=None):
    o = {"hi": P.rhi.fresh(), "part": P.rpart.fresh()}
    hi, lo = split_host(P.x, P.dt, mut)
    o["hi"][P.rhi.idx] = hi.reshape(-1)
    if P.rlo is not None:
        o["lo"] = P.rlo.fresh(lo)
    ch = P.x.reshape(P.M, -1, 128)                           # two passes
    mean = ch.sum(-1) * (1.0 / 128)
    part = torch.stack((mean, ((ch - mean[..., None]) ** 2).sum(-1)), -1)
    if mut == "part_chunk_off_by_one":
        part = part.roll(1, 1)
    o["part"][P.rpart.idx] = part.reshape(-1)
    return o


def s_verify(P, o):
    fails, fig = [], {}
    hi = P.rhi.body(o["hi"])
    he, le = ops.split_residual(P.x, P.dt)
    if not torch.equal(_bits(hi), _bits(he)):
        fails.append("xb != x in 16 bits")
    if P.rlo is not None and not torch.equal(P.rlo.body(o["lo"]), le):
        fails.append(f"xl != split_residual(x) at {int((P.rlo.body(o['lo']) != le).sum())} elements")
    part = P.rpart.body(o["part"]).reshape(P.M, -1, 2)
    ex = (part.double() - chunk_stats64(P.x)).abs() - part_bounds(P.x, "stats")
    fig["part excess"] = float(torch.nan_to_num(ex, nan=float("inf")).max())
    if not bool((ex <= 0).all()):
        fails.append(f"part: {int((~(ex <= 0)).sum())} values over the bound, excess {fig['part excess']:.3e}")
    for k, reg in (("hi", P.rhi), ("lo", P.rlo), ("part", P.rpart)):
        if reg is not None and reg.canaries_changed(o[k]):
            fails.append(f"{k}: {reg.canaries_changed(o[k])} canaries changed")
    return fails, fig


# ================================================================================== the self-check
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_selfcheck_fp32_model_passes_every_case(dt):
    """(a) no bound is tighter than a correct fp32 evaluation can meet: both measured allowances at 0."""
    for ci, c in enumerate(PCASES):
        P = pproblem(ci, dt)
        fails, _ = p_verify(P, ci, p_model(P)[0], rsq_allow=0.0)
        assert not fails, f"{c['name']}: {fails}"
    for ci, c in enumerate(CCASES):
        P = cproblem(ci, dt)
        fails, _ = c_verify(P, c_model(P), gelu_allow=0.0, rsq_allow=0.0)
        assert not fails, f"{c['name']}: {fails}"
        rs = merge_model(P.part)                             # statistics handed over as data
        fails, _ = c_verify(P, c_model(P, rs=rs), rs=rs, gelu_allow=0.0)
        assert not fails, f"{c['name']} (rs as data): {fails}"
    for ci, c in enumerate(SCASES):
        P = sproblem(ci, dt)
        fails, _ = s_verify(P, s_model(P))
        assert not fails, f"{c['name']}: {fails}"


MUTATIONS = ["merge_no_between_term", "var_over_1023", "eps_omitted", "mean_sign_flipped", "colsum_unrounded",
             "part_chunk_off_by_one", "consumer_chunk_off_by_one", "stats_of_neighbour_row", "exp_from_x",
             "s_off_by_one", "q_not_clamped", "hi_not_updated"]
_SPLIT_MUTS = ("exp_from_x", "s_off_by_one", "q_not_clamped", "hi_not_updated")


@pytest.mark.parametrize("mut", MUTATIONS)
def test_selfcheck_mutation_is_caught(mut):
    """(b) a subtly wrong kernel fails at least one case (the measured allowances at their shipped values)."""
    caught = []
    for dt in DTYPES:
        for ci, c in enumerate(PCASES):
            if c["M"] > 64 and not (c["rs"] and c["M"] <= 256):      # the small cases and one with rs are enough
                continue
            P = pproblem(ci, dt)
            if p_verify(P, ci, p_model(P, mut)[0])[0]:
                caught.append(c["name"])
        if mut not in _SPLIT_MUTS and mut != "part_chunk_off_by_one":
            for ci, c in enumerate(CCASES[:4]):
                P = cproblem(ci, dt)
                if c_verify(P, c_model(P, mut))[0]:
                    caught.append(c["name"])
        if mut in _SPLIT_MUTS[:3] + ("part_chunk_off_by_one",):
            for ci, c in enumerate(SCASES):
                P = sproblem(ci, dt)
                if s_verify(P, s_model(P, mut))[0]:
                    caught.append(c["name"])
    assert caught, f"mutation {mut} passes every case"


def test_selfcheck_edges_are_what_they_claim():
    """The split-residual edge elements hit the encodings their comments name (host restatement)."""
    for dt in DTYPES:
        U = 2.0 ** -7 if dt == torch.bfloat16 else 2.0 ** -10
        el = edge_elements(dt)
        hi = torch.tensor([e[0] for e in el]).to(dt)
        q = torch.tensor([e[1] for e in el], dtype=torch.int8)
        xn = torch.tensor([e[2] for e in el], dtype=torch.float32) + ops.merge_residual(hi, q)
        assert torch.equal(xn.double(), torch.tensor([e[2] for e in el]).double() + ops.merge_residual(hi, q).double())
        h, l = ops.split_residual(xn, dt)
        hf = h.float().tolist()
        assert hf[:6] == [1.0, -1.0, 1 + 2 * U, 0.0, 2.0, 2.0]
        assert l.tolist()[:6] == [127, -128, -128, 0, -16, 32]
        assert 2.0 <= hf[6] < 4.0 and 0.5 <= hf[7] < 1.0
        raw = torch.round(torch.ldexp(xn - h.float(), (S_OF[dt] - torch.frexp(h.float()).exponent).float()))
        assert raw[0] == 128                                  # the clamp is what makes it 127
        if dt == torch.float16:
            assert hf[9] == 3 * 2.0 ** -24 and l[9] == 127 and raw[9] > 127 and hf[10] == -2.0 ** -20 and l[10] == 0
            assert hf[11] == float("inf") and float(xn[11]) == 65520.0 and l[11] == -128
        else:
            assert hf[11] == 65536.0 and l[11] == -8


# ====================================================================================== 3. the GPU
_STATE = {}


@pytest.fixture(scope="module")
def workspace(cuda):
    ws = ops.gemm_workspace(cuda)
    _STATE["ws"] = ws
    return ws


def _dev(region, buf, cuda):
    """(device allocation, the view dp_gemm gets: from the region's first element)."""
    d = buf.to(cuda)
    return d, d[region.base:]


def launch_producer(P, cuda, ws=None):
    """Run producer P on the GPU: the allocations after the call (CPU), planned tile."""
    c = P.c
    pre = p_prefill(P)
    dev = {k: v.to(cuda) for k, v in pre.items()}
    A = gc._embed(P.A, P.lda, P.off, cuda)
    B = gc._embed(P.B, P.ldb, 2 * P.off, cuda)
    view = lambda k, reg: dev[k][reg.base:]      # noqa: E731
    kw = dict(M=P.M, N=P.N, K=P.K, lda=P.lda, A_off=MARGIN + P.off, ldb=P.ldb, B_off=MARGIN + 2 * P.off, ldc=P.ldc,
              bias=None if P.bias is None else P.bias.to(cuda), gamma=None if P.gamma is None else P.gamma.to(cuda),
              accumulate=True, ln_out=(view("hi", P.rhi), view("part", P.rpart) if P.rpart is not None else None))
    if c["kind"] == "split":
        kw.update(ln_xl=view("lo", P.rlo))
    if P.rrs is not None:
        kw.update(ln_rs_out=view("rs", P.rrs), ln_eps=1e-6, workspace=ws)
    Cv = view("C", P.rC) if P.rC is not None else None
    tile, _ = ops.gemm(A, B, Cv, plan_only=True, **kw)
    ops.gemm(A, B, Cv, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in dev.items()}, tile


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("ci", range(len(PCASES)), ids=PCASE_IDS)
def test_producer(cuda, workspace, record, ci, dt):
    P = pproblem(ci, dt)
    o, tile = launch_producer(P, cuda, workspace)
    assert tile == T_8PH320
    fails, fig = p_verify(P, ci, o)
    for k, v in fig.items():
        record(k, v)
    print(f"{P.c['name']} {dt}: " + ", ".join(f"{k} {v:.3e}" for k, v in fig.items()))
    assert not fails, f"{P.c['name']} {dt}:\n" + "\n".join(fails)


def launch_consumer(P, cuda, tile, ws=None, rs=None):
    """Run consumer P: C allocation after the call (CPU), planned tile.  rs: a device [M rounded up to even][2]."""
    A = gc._embed(P.xb, P.lda, P.off, cuda)
    B = gc._embed(P.B, P.ldb, 2 * P.off, cuda)
    C = P.rC.fresh().to(cuda)
    kw = dict(M=P.M, N=P.N, K=P.K, lda=P.lda, A_off=MARGIN + P.off, ldb=P.ldb, B_off=MARGIN + 2 * P.off, ldc=P.ldc,
              bias=P.bias.to(cuda), act=P.c["act"], tile=tile, workspace=ws, ln_eps=1e-6,
              ln_in=(P.part.to(cuda) if rs is None else None, P.colsum.to(cuda)), ln_rs_in=rs)
    planned, _ = ops.gemm(A, B, C[P.rC.base:], plan_only=True, **kw)
    ops.gemm(A, B, C[P.rC.base:], **kw)
    torch.cuda.synchronize()
    return C.cpu(), planned


def rs_padded(rs, cuda):
    """[M][2] statistics in a device buffer of M rounded up to even rows, the pad row NaN (never used, the header says)."""
    M = rs.shape[0]
    buf = torch.full((M + (M & 1), 2), float("nan"), dtype=torch.float32)
    buf[:M] = rs
    return buf.to(cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("ci", range(len(CCASES)), ids=CCASE_IDS)
def test_consumer_on_both_engines(cuda, workspace, record, ci, dt):
    """The 320 x 256 engine with ln_part_in; the persistent engine with ln_part_in + a workspace (its pre-pass
    statistics, read back from the workspace, checked on their own) and with those statistics as ln_rs_in
    (pad row NaN): the two persistent runs bit-identical."""
    P = cproblem(ci, dt)
    fails, fig = [], {}
    C1, t1 = launch_consumer(P, cuda, 0)
    assert t1 == T_8PH320
    f, worst = c_verify(P, C1)
    fails += [f"320 x 256: {s}" for s in f]
    workspace[WS_RS_OFFSET:WS_RS_OFFSET + 8 * P.M].fill_(0xFF)            # NaNs where the pre-pass must write
    C2, t2 = launch_consumer(P, cuda, T_P8PH, ws=workspace)
    assert t2 == T_P8PH
    rs = workspace[WS_RS_OFFSET:WS_RS_OFFSET + 8 * P.M].view(torch.float32).reshape(P.M, 2).cpu()
    fails += [f"pre-pass {s}" for s in rs_check(rs, P.part, fig)]
    f, w2 = c_verify(P, C2)
    fails += [f"persistent, part: {s}" for s in f]
    C3, t3 = launch_consumer(P, cuda, 0, rs=rs_padded(rs, cuda))
    assert t3 == T_P8PH
    f, w3 = c_verify(P, C3, rs=rs)
    fails += [f"persistent, rs as data: {s}" for s in f]
    if not torch.equal(_bits(C2), _bits(C3)):
        fails.append("persistent: ln_part_in + workspace and ln_rs_in differ")
    if bool(torch.isnan(P.rC.body(C3).float()).any()):
        fails.append("NaN in the output (the ln_rs_in pad row leaked)")
    worst = max(worst, w2, w3)
    record("consumer largest excess over the allowance-free bound", worst)
    record("rstd relative excess", fig["rstd relative excess"])
    print(f"{P.c['name']} {dt}: consumer excess {worst:.3e}, rstd relative excess {fig['rstd relative excess']:.3e}")
    assert not fails, f"{P.c['name']} {dt}:\n" + "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("pname", ["split_1x1024x128_rs", "split_321x1024x64_noC_rs"])
def test_producer_statistics_feed_the_persistent_consumer(cuda, workspace, record, pname, dt):
    """A split producer's ln_rs_out (checked on its own) as the persistent consumer's ln_rs_in: bit-identical to the
    consumer that merges the producer's part in its pre-pass, and within the bound of the fp64 reference over the
    producer's hi' rows with those statistics as data."""
    pi = PCASE_IDS.index(pname)
    P = pproblem(pi, dt)
    o, _ = launch_producer(P, cuda, workspace)
    fails, fig = p_verify(P, pi, o)
    M, K, N = P.M, 1024, 256
    C = CProblem()
    C.c, C.dt, C.M, C.N, C.K = dict(name=pname + "_consumer", act=DP_ACT_GELU), dt, M, N, K
    C.fam = ["producer row"] * M
    C.xb = P.rhi.body(o["hi"]).clone()
    C.part = P.rpart.body(o["part"]).reshape(M, 8, 2).clone()
    g = torch.Generator().manual_seed(77)
    C.B = (torch.randn(N, K, generator=g) * K ** -0.5).to(dt)
    C.colsum = C.B.double().sum(1).float()
    C.bias = torch.randn(N, generator=g) * 0.5
    C.lda, C.ldb, C.ldc, C.off = K, K, N, 0
    C.rC = Region(M, N, N, 0, dt)
    rs = P.rrs.body(o["rs"])
    C1, t1 = launch_consumer(C, cuda, T_P8PH, ws=workspace)
    C2, t2 = launch_consumer(C, cuda, 0, rs=rs_padded(rs, cuda))
    assert t1 == T_P8PH and t2 == T_P8PH
    f, worst = c_verify(C, C2, rs=rs)
    fails += f
    if not torch.equal(_bits(C1), _bits(C2)):
        fails.append("ln_rs_in from the producer and the pre-pass over its part differ")
    if bool(torch.isnan(C.rC.body(C2).float()).any()):
        fails.append("NaN in the output")
    record("consumer largest excess over the allowance-free bound", worst)
    assert not fails, f"{pname} {dt}:\n" + "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_row_tile_counters_reset_between_launches(cuda, workspace, record, dt):
    """Two ln_rs_out producers back to back on one workspace (M = 321: 2 row tiles, then M = 641: 3): the second
    launch's statistics are within bound too, and the counters (workspace words 512 .. 1022) are zero after each."""
    for name in ("split_321x1024x64_noC_rs", "split_641x1024x64_rs_nobias"):
        ci = PCASE_IDS.index(name)
        P = pproblem(ci, dt)
        o, _ = launch_producer(P, cuda, workspace)
        fails, fig = p_verify(P, ci, o)
        record("rstd relative excess", fig["rstd relative excess"])
        assert not fails, f"{name} {dt}:\n" + "\n".join(fails)
        assert int(workspace[2048:4092].view(torch.int32).abs().sum()) == 0, "row-tile counters not reset"


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("ci", range(len(SCASES)), ids=[c["name"] for c in SCASES])
def test_layernorm_stats(cuda, record, ci, dt):
    """dp_layernorm_stats at 512, 1024 and 2048 columns, with and without xl, with ldx / ldxb past the row and
    offset bases (the ctypes call: ops.layernorm_stats passes cols for both)."""
    P = sproblem(ci, dt)
    x = P.rx.fresh(P.x).to(cuda)
    dev = {"hi": P.rhi.fresh().to(cuda), "part": P.rpart.fresh().to(cuda)}
    if P.rlo is not None:
        dev["lo"] = P.rlo.fresh().to(cuda)
    rc = _lib.load().dp_layernorm_stats(x[P.rx.base:].data_ptr(), P.ldx, P.M, P.N, dev["hi"][P.rhi.base:].data_ptr(), P.ldxb,
                                        dev["lo"][P.rlo.base:].data_ptr() if P.rlo is not None else None,
                                        dev["part"][P.rpart.base:].data_ptr(), ops.dtype_code(dt),
                                        torch.cuda.current_stream(cuda).cuda_stream)
    assert rc == OK
    torch.cuda.synchronize()
    fails, fig = s_verify(P, {k: v.cpu() for k, v in dev.items()})
    record("part excess", fig["part excess"])
    assert not fails, f"{P.c['name']} {dt}:\n" + "\n".join(fails)


@pytest.mark.gpu
def test_zz_sticky_error_word_is_zero(cuda):
    """Last in the module: no launch above left the workspace's sticky error word set."""
    ws = _STATE.get("ws")
    if ws is not None:
        assert ops.workspace_error(ws) == 0
