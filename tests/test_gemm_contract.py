"""dp_gemm's documented contract (include/dp_mi355x.h) at its edges, against an fp64 reference.

Every case runs under DP_TILE_AUTO and under every DP_TILE_* hint.  `expected_rc` -- written from
the header text alone -- says which (hint, case) pairs the library must reject and with which
DP_ERR_*; dp_gemm_plan must agree for every pair, and every accepted pair is launched.

Reference: the header's formula in fp64 on the CPU over the 16-bit operands upcast exactly.
Per-element bound (not per tensor), for every element of the documented store set:

    |out - ref| <= u_out * |ref| + (K + 16) * 2^-24 * S     (+ GELU_ALLOWANCE with DP_ACT_GELU)

S is the same formula on absolute values (|A| |B|^T + |bias|, through |gamma|, + |pos| + |R1| +
|R2| + |C_old|): (K + 16) * 2^-24 bounds an fp32 dot product of length K in any summation order
plus the epilogue's few additions; u_out = 2^-8 (bf16), 2^-11 (f16), 2^-23 (fp32 C).  ReLU is
1-Lipschitz (bound unchanged); for GELU the accumulation term is multiplied by 1.13 (its Lipschitz
constant).  The fused 1x1 head sums N such values: S_head = sum_n S[n] |head_w[n]| + |head_b| with
the factor (K + 16 + N) * 2^-24.

Canaries: every output (and accumulate) buffer carries 64 elements before and after, the [N, ldc)
padding, two rows past the last one and the gap rows of a row-group remap; 16-bit elements outside
the store set hold a fixed bit pattern, fp32 ones NaN, and must be bit-identical after the call.
Inputs carry the same margins, so a clamped out-of-range load reads mapped memory.

The CPU self-check (no GPU) shows the bound is neither too tight (a correct fp32 evaluation passes
every case) nor too loose (each seeded mutation of that evaluation fails at least one case).
"""

import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from depth_pro import _lib, ops
from depth_pro._lib import DP_ACT_GELU, DP_ACT_NONE, DP_ACT_RELU

DTYPES = [torch.bfloat16, torch.float16]
OK, ERR_ARG, ERR_SHAPE, ERR_ALIGN = 0, 1000, 1001, 1002
N_TILES = 24
NUM_CUS = 256              # MI355X; dp_gemm_plan's fallback without a device is the same
MARGIN = 64
PAT16 = 0x5A5A             # prefill of unwritten 16-bit elements (bf16 1.5e16, f16 203.25)
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -23}

# The device gelu_erf is x * sigmoid(odd polynomial), an approximation whose error cannot be derived
# from the formats.  Measured on MI355X over the GELU cases of this module (both dtypes, every engine):
# the largest value of |out - ref| - bound with allowance 0 was -2.3e-6 (chain_gelu_c32_136), i.e. no
# element exceeds the derived bound and the measured excess is 0; the allowance is twice it.
GELU_EXCESS_MEASURED = 0.0
GELU_ALLOWANCE = 2.0 * GELU_EXCESS_MEASURED


# ------------------------------------------------------------------------------------------ cases
def _case(name, kind, M, N, K, **kw):
    c = dict(name=name, kind=kind, M=M, N=N, K=K, bias=True, act=DP_ACT_NONE, gamma=False, pos=False, R1=False,
             R2=False, acc=False, c32=False, relu_a=False, rowgrp=False, head=False, strides=False, conv=None,
             deconv=None, half2=False)
    c.update(kw)
    return c


def _cases():
    cs = []
    for M, N, K in [(257, 20, 64), (300, 36, 128), (300, 60, 192), (130, 100, 64),          # ragged N < 8 columns
                    (321, 72, 128), (513, 200, 192), (257, 264, 320), (640, 520, 128),      # ragged N, 8-column engines
                    (1, 256, 128), (15, 256, 64), (255, 512, 128), (256, 256, 64), (1, 4, 64)]:   # small M
        cs.append(_case(f"dense_{M}x{N}x{K}", "dense", M, N, K))
    for M, N, K in [(257, 264, 128), (130, 36, 64)]:
        cs.append(_case(f"strides_{M}x{N}x{K}", "dense", M, N, K, strides=True, pos=True, R1=True, R2=True))
    for M, N, K in [(300, 136, 128), (300, 36, 128)]:
        full = dict(gamma=True, pos=True, R1=True, R2=True)
        for act, an in ((DP_ACT_RELU, "relu"), (DP_ACT_GELU, "gelu")):
            cs.append(_case(f"chain_{an}_acc32_{N}", "dense", M, N, K, act=act, acc=True, c32=True, **full))
            cs.append(_case(f"chain_{an}_c16_{N}", "dense", M, N, K, act=act, **full))
            cs.append(_case(f"chain_{an}_c32_{N}", "dense", M, N, K, act=act, c32=True, **full))
        cs.append(_case(f"chain_rowgrp_{N}", "dense", M, N, K, act=DP_ACT_RELU, gamma=True, pos=True, rowgrp=True))
        cs.append(_case(f"acc_only_{N}", "dense", M, N, K, acc=True, c32=True, gamma=True))   # the residual fast path
    convs = [(2, 9, 13, 64, 72, 3, 1, 1), (1, 11, 7, 128, 256, 3, 2, 1), (3, 6, 6, 64, 36, 1, 1, 0),
             (1, 8, 10, 64, 128, 3, 1, 0), (2, 8, 6, 64, 264, 2, 2, 0), (1, 7, 7, 64, 20, 5, 1, 2)]
    for i, (b, h, w, ci, co, k, s, p) in enumerate(convs):
        oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        g = dict(batch=b, in_h=h, in_w=w, in_c=ci, k=k, stride=s, pad=p, out_h=oh, out_w=ow)
        for relu_a in (False, True):
            cs.append(_case(f"conv{i}_b{b}_{h}x{w}_k{k}s{s}p{p}_co{co}_relu{int(relu_a)}", "conv", b * oh * ow, co,
                            k * k * ci, conv=g, relu_a=relu_a, act=DP_ACT_RELU if relu_a else DP_ACT_NONE,
                            R1=(i == 0), R2=(i == 0)))
    for N in (4, 20, 32):
        cs.append(_case(f"head_dense_{N}", "dense", 300, N, 128, head=True, act=DP_ACT_RELU, c32=True))
        g = dict(batch=2, in_h=9, in_w=13, in_c=64, k=3, stride=1, pad=1, out_h=9, out_w=13)
        cs.append(_case(f"head_conv_{N}", "conv", 2 * 9 * 13, N, 576, conv=g, head=True, act=DP_ACT_RELU, c32=True))
    for b, h, w, ci, co in [(1, 5, 9, 64, 4), (2, 5, 9, 64, 12), (1, 9, 5, 128, 16), (1, 6, 10, 64, 20),
                            (2, 7, 9, 64, 36), (1, 8, 8, 128, 64)]:
        for half2 in (False, True):
            cs.append(_case(f"deconv_b{b}_{h}x{w}_co{co}_half{int(half2)}", "deconv", b * h * w, 4 * co, ci,
                            deconv=(h, w, co), half2=half2))
    cs.append(_case("deconv_c32_co20", "deconv", 60, 80, 64, deconv=(6, 10, 20), c32=True))
    cs.append(_case("deconv_c32_co64", "deconv", 64, 256, 128, deconv=(8, 8, 64), c32=True))
    for b, h, w in [(1, 6, 8), (1, 5, 12), (2, 9, 20)]:     # the persistent 8-phase engine's 8-pixel steps
        cs.append(_case(f"deconv_p8_b{b}_{h}x{w}", "deconv", b * h * w, 256, 128, deconv=(h, w, 64)))
    return cs


CASES = _cases()
CASE_IDS = [c["name"] for c in CASES]


# ------------------------------------------------------------------------- seeded problem instances
class Problem:
    """CPU tensors of one case (16-bit operands, fp32 epilogue operands) and its leading dimensions."""


@functools.lru_cache(maxsize=None)
def problem(ci, dt):
    c = CASES[ci]
    g = torch.Generator().manual_seed(1000 + ci)
    M, N, K = c["M"], c["N"], c["K"]
    P = Problem()
    P.c, P.dt = c, dt
    r = lambda *s: torch.randn(*s, generator=g)    # noqa: E731  (entries of both signs)
    if c["kind"] == "conv":
        q = c["conv"]
        P.x = r(q["batch"], q["in_h"], q["in_w"], q["in_c"]).to(dt)          # NHWC
    else:
        P.A = r(M, K).to(dt)
    P.B = (r(N, K) * K ** -0.5).to(dt)
    P.bias = r(N) if c["bias"] else None
    P.gamma = r(N) if c["gamma"] else None                                   # negative entries included
    P.pos_group, P.pos_off = (7, 2) if c["pos"] else (0, 0)
    P.pos = r(P.pos_group + P.pos_off, N) if c["pos"] else None
    P.R1 = r(M, N).to(dt) if c["R1"] else None
    P.R2 = r(M, N).to(dt) if c["R2"] else None
    P.C_old = r(M, N) if c["acc"] else None
    P.head_w = r(N) if c["head"] else None
    P.head_b = 0.25
    P.row_group, P.row_group_out, P.row_off = (5, 7, 1) if c["rowgrp"] else (0, 0, 0)
    s = c["strides"]
    P.lda, P.ldb = K + (8 if s else 0), K + (16 if s else 0)
    P.ldc, P.ldr1, P.ldr2, P.ldpos = N + (8 if s else 0), N + (8 if s else 0), N + (16 if s else 0), N + (8 if s else 0)
    P.A_off, P.B_off, P.C_off = (8, 16, 8) if s else (0, 0, 0)
    if c["deconv"]:
        co = c["deconv"][2]
        P.ldc, P.C_off = (2 * co + 8, co + 8) if c["half2"] else (co, 0)
    P.c_dt = torch.float32 if c["c32"] else dt
    return P


def out_rows(P):
    """Rows of ldc elements the C allocation spans (documented rows + 2 beyond)."""
    c = P.c
    if c["head"]:
        return 1
    if c["deconv"]:
        return 4 * c["M"] + 2
    last = c["M"] - 1
    if P.row_group:
        last = (last // P.row_group) * P.row_group_out + P.row_off + last % P.row_group
    return last + 1 + 2


def out_numel(P):
    body = P.c["M"] if P.c["head"] else out_rows(P) * P.ldc
    return MARGIN + P.C_off + body + MARGIN


def store_index(P, mut=None):
    """Flat index into the C allocation of every (m, n) -- the header's store mapping, verbatim."""
    c = P.c
    M, N = c["M"], c["N"]
    base = MARGIN + P.C_off
    m = torch.arange(M).unsqueeze(1)
    n = torch.arange(N).unsqueeze(0)
    if c["head"]:
        return base + torch.arange(M)
    if c["deconv"]:
        h, w, co = c["deconv"]
        b, rr = m // (h * w), m % (h * w)
        y, x = rr // w, rr % w
        nq = (n // 8) * 8 if mut == "parity8" else n         # mutation: the parity of an 8-column chunk's first column
        q = nq // co
        pix = (b * 2 * h + 2 * y + q // 2) * (2 * w) + 2 * x + q % 2
        return base + pix * P.ldc + (n - q * co)
    row = m
    if P.row_group:
        row = (m // P.row_group) * P.row_group_out + P.row_off + m % P.row_group
    return base + row * P.ldc + n


# -------------------------------------------------------------------------------- the formula itself
def _im2col(P, x, mut=None):
    """[M][K] implicit-conv A with the header's k order, k = ((ci/64 * k_h + ky) * k_w + kx) * 64 + ci%64."""
    q = P.c["conv"]
    b_, H, W, C, k, s, p, oh, ow = (q[t] for t in ("batch", "in_h", "in_w", "in_c", "k", "stride", "pad", "out_h", "out_w"))
    m = torch.arange(P.c["M"])
    if mut == "one_image":            # mutation: the rows of a tile as one tall image (no batch boundary)
        b, oy, ox = torch.zeros_like(m), m // ow, m % ow
        iy_ok_hi = b_ * H
    else:
        b, oy, ox = m // (oh * ow), (m % (oh * ow)) // ow, m % ow
        iy_ok_hi = H
    ky, kx = torch.arange(k).view(1, k, 1), torch.arange(k).view(1, 1, k)
    iy = (oy * s - p).view(-1, 1, 1) + ky
    ix = (ox * s - p).view(-1, 1, 1) + kx
    ok = (iy >= 0) & (iy < iy_ok_hi) & (ix >= 0) & (ix < W)
    pitch = H if mut == "in_h_pitch" else W      # mutation: in_h where in_w belongs
    pix = (b.view(-1, 1, 1) * H * W + iy * pitch + ix).clamp(0, b_ * H * W - 1)
    g = x.reshape(b_ * H * W, C)[pix.reshape(-1)].reshape(-1, k, k, C // 64, 64)
    g = g * ok.reshape(-1, k, k, 1, 1).to(g.dtype)
    return g.permute(0, 3, 1, 2, 4).reshape(P.c["M"], k * k * C)


def _acc(P, ft, absval, via_conv2d, mut=None):
    """A . B^T in `ft`; absval: on absolute values (the bound's S)."""
    c = P.c
    B = P.B.to(ft)
    if absval:
        B = B.abs()
    if c["kind"] == "conv":
        x = P.x.to(ft)
        if c["relu_a"]:
            x = F.relu(x)
        if absval:
            x = x.abs()
        q = c["conv"]
        if via_conv2d:     # the inverse of ops.conv_weight's layout -> [Cout][Cin][kh][kw]
            w = B.reshape(c["N"], q["in_c"] // 64, q["k"], q["k"], 64).permute(0, 1, 4, 2, 3).reshape(
                c["N"], q["in_c"], q["k"], q["k"])
            y = F.conv2d(x.permute(0, 3, 1, 2), w, stride=q["stride"], padding=q["pad"])
            return y.permute(0, 2, 3, 1).reshape(c["M"], c["N"])
        A = _im2col(P, x, mut)
    else:
        A = P.A.to(ft)
        if c["relu_a"]:
            A = F.relu(A)
        if absval:
            A = A.abs()
    if mut == "drop_k":               # mutation: the last 64-wide K block never accumulated
        A, B = A[:, :-64], B[:, :-64]
    return A @ B.t()


def evaluate(P, ft=torch.float64, absval=False, via_conv2d=True, mut=None):
    """The header's epilogue chain on A . B^T: values [M][N] (or [M] with the fused head) in `ft`."""
    c = P.c
    a = (lambda t: t.to(ft).abs()) if absval else (lambda t: t.to(ft))
    v = _acc(P, ft, absval, via_conv2d, mut)
    if P.bias is not None:
        v = v + a(P.bias)
    gam_first = mut == "gamma_first" and P.gamma is not None
    if gam_first:                      # mutation: gamma before the activation
        v = v * a(P.gamma)
    if c["act"] == DP_ACT_RELU:
        v = v if absval else F.relu(v)
    elif c["act"] == DP_ACT_GELU:
        v = v * 1.13 if absval else F.gelu(v)
    if P.gamma is not None and not gam_first:
        v = v * a(P.gamma)
    if P.pos is not None:
        off = 0 if mut == "no_pos_off" else P.pos_off       # mutation: pos row m % pos_group
        v = v + a(P.pos)[torch.arange(c["M"]) % P.pos_group + off]
    if P.R1 is not None:
        v = v + a(P.R1)
    if P.R2 is not None and mut != "no_r2":                 # mutation: R2 omitted
        v = v + a(P.R2)
    if P.C_old is not None:
        v = v + a(P.C_old)
    if c["head"]:
        v = v @ a(P.head_w) + abs(P.head_b)
        v = v if absval else F.relu(v)
    return v


@functools.lru_cache(maxsize=None)
def reference(ci, dt):
    """(ref, bound, gelu) of case ci in fp64."""
    P = problem(ci, dt)
    c = P.c
    ref, S = evaluate(P), evaluate(P, absval=True)
    terms = c["K"] + 16 + (c["N"] if c["head"] else 0)
    bound = U_OUT[P.c_dt] * ref.abs() + terms * 2.0 ** -24 * S
    return ref, bound, c["act"] == DP_ACT_GELU


def prefill(P):
    """The C allocation before the call: canaries everywhere, C_old in the store set when accumulating."""
    n = out_numel(P)
    if P.c_dt == torch.float32:
        buf = torch.full((n,), float("nan"), dtype=torch.float32)
        if P.C_old is not None:
            buf[store_index(P).reshape(-1)] = P.C_old.reshape(-1)
        return buf
    return torch.full((n,), PAT16, dtype=torch.int16).view(P.c_dt)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def verify(P, ci, out, allowance=GELU_ALLOWANCE):
    """out: the C allocation after the call (CPU).  Returns (elements over the bound, canaries changed,
    largest excess over the allowance-free bound)."""
    ref, bound, gelu = reference(ci, P.dt)
    idx = store_index(P).reshape(-1)
    err = (out.double()[idx] - ref.reshape(-1)).abs()
    excess = err - bound.reshape(-1)
    lim = allowance if gelu else 0.0
    n_bad = int((~(excess <= lim)).sum())          # NaN counts as bad
    keep = torch.ones(out.numel(), dtype=torch.bool)
    keep[idx] = False
    n_canary = int((_bits(out)[keep] != _bits(prefill(P))[keep]).sum())
    return n_bad, n_canary, float(torch.nan_to_num(excess, nan=float("inf")).max())


def emulate(P, mut=None):
    """A correct kernel in fp32 on the CPU (an independent im2col for the convs), or a seeded mutation
    of it: the C allocation after the call."""
    c = P.c
    v = evaluate(P, torch.float32, via_conv2d=False, mut=mut)
    buf = prefill(P)
    idx = store_index(P, mut)
    if mut == "past_n" and not c["head"] and not c["deconv"]:   # mutation: one column past N is stored too
        buf[(idx[:, -1] + 1)] = v[:, -1].to(P.c_dt)
    buf[idx.reshape(-1)] = v.reshape(-1).to(P.c_dt)
    return buf


MUTATIONS = ["drop_k", "gamma_first", "no_pos_off", "no_r2", "parity8", "past_n", "one_image", "in_h_pitch"]


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_selfcheck_correct_fp32_evaluation_passes(dt):
    """(a) the bound is not tighter than a correct fp32 kernel can meet: no element excluded, no GELU allowance."""
    for ci, c in enumerate(CASES):
        P = problem(ci, dt)
        n_bad, n_canary, excess = verify(P, ci, emulate(P), allowance=0.0)
        assert n_bad == 0 and n_canary == 0, f"{c['name']}: {n_bad} over the bound (excess {excess:.3e}), {n_canary} canaries"


@pytest.mark.parametrize("mut", MUTATIONS)
def test_selfcheck_mutation_is_caught(mut):
    """(b) a subtly wrong kernel fails the bound or the canary check on at least one case."""
    caught = []
    for ci, c in enumerate(CASES):
        P = problem(ci, torch.bfloat16)      # the wider bound: what it catches, f16 catches too
        n_bad, n_canary, _ = verify(P, ci, emulate(P, mut), allowance=1e-5)
        if n_bad or n_canary:
            caught.append(c["name"])
    assert caught, f"mutation {mut} passes every case"


# ----------------------------------------------------------------------- the header as a predicate
def expected_rc(P, tile, ws_bytes):
    """Return code of dp_gemm / dp_gemm_plan for problem P under `tile`, from include/dp_mi355x.h:
    'What a tile hint accepts', checks 1 - 5 in order."""
    c = P.c
    M, N, K = c["M"], c["N"], c["K"]
    c16 = P.c_dt != torch.float32
    dense, dcv = c["kind"] != "conv", c["deconv"]
    # 1. general: K % 64, N % 4 (SHAPE); lda / ldb % 8, the % 4 rules (ALIGN); dc_cout % 4 (SHAPE)
    if K % 64 or N % 4:
        return ERR_SHAPE
    if P.ldb % 8 or (dense and P.lda % 8):
        return ERR_ALIGN
    if (not c["head"] and P.ldc % 4) or (c["R1"] and P.ldr1 % 4) or (c["R2"] and P.ldr2 % 4) or (c["pos"] and P.ldpos % 4):
        return ERR_ALIGN
    if dcv and dcv[2] % 4:
        return ERR_SHAPE
    if c["head"] and N > 32:
        return ERR_SHAPE
    # 2. the fused head always runs on DP_TILE_256x32; 3. hints 1 - 3 take everything (no head_corr here)
    if c["head"] or tile <= _lib.DP_TILE_256x32:
        return OK
    # 4. the 8-column rules
    if N % 8 or (dcv and dcv[2] % 8):
        return ERR_SHAPE
    if (c["R1"] and P.ldr1 % 8) or (c["R2"] and P.ldr2 % 8) or (c16 and P.ldc % 8):
        return ERR_ALIGN
    # 5. per engine
    T = _lib
    rows = not dcv
    perrow = c["R1"] or c["R2"] or c["pos"] or c["acc"]
    if tile == T.DP_TILE_STREAMK_256x256:
        return OK if ws_bytes and N % 256 == 0 else ERR_ARG
    if tile == T.DP_TILE_SPLITK_256x256:
        if not ws_bytes or N % 256 or not rows or P.row_group:
            return ERR_ARG
        tiles = -(-M // 256) * (N // 256)
        split = min(NUM_CUS // tiles, (K // 64) // 2, (ws_bytes - 4096) // (4 * M * N), 32)
        return OK if split >= 2 else ERR_SHAPE
    if tile in (T.DP_TILE_PBIG_320x256, T.DP_TILE_PBIG_256x256):
        return OK if N % 256 == 0 and rows else ERR_ARG                  # (extents here are far below the limits)
    if tile == T.DP_TILE_P8PH_256x256:
        ok = dense and N % 256 == 0 and K >= 128 and c16 and not perrow and not P.row_group and (
            rows or (not c["relu_a"] and c["act"] == DP_ACT_NONE and not c["gamma"] and dcv[1] >= 8))
        return OK if ok else ERR_ARG
    if tile == T.DP_TILE_8PH_320x256:
        ok = dense and not c["relu_a"] and N % 256 == 0 and rows and not (c["R1"] or c["R2"] or c["pos"]) and \
            not P.row_group and ((c16 and not c["acc"]) or (not c16 and c["acc"] and c["act"] == DP_ACT_NONE))
        return OK if ok else ERR_ARG
    if tile in (T.DP_TILE_CV3_256x256, T.DP_TILE_CV3_192x256, T.DP_TILE_CV3_384x128):
        q = c["conv"]
        ok = q is not None and q["k"] == 3 and q["stride"] == 1 and q["pad"] == 1 and \
            q["in_h"] == q["in_w"] == q["out_h"] == q["out_w"] and q["in_w"] % 16 == 0 and \
            (tile == T.DP_TILE_CV3_256x256 or q["in_w"] % 48 == 0) and not (c["gamma"] or c["pos"] or c["acc"]) and \
            not P.row_group and c["act"] != DP_ACT_GELU and c16 and N % 256 == 0 and rows and \
            tile != T.DP_TILE_CV3_384x128                                  # (no head_corr / HEAD_PS case here)
        return OK if ok else ERR_ARG
    return OK                                                              # BIG_* / DEEP* / DUAL / 8PH_256x256


# ------------------------------------------------------------------------------- launching a case
def _embed(t, ld, off, device, fill=0.0):
    """t [rows][cols] -> a flat buffer of MARGIN + off + rows * ld + MARGIN elements with t at MARGIN + off."""
    rows, cols = t.shape
    buf = torch.full((MARGIN + off + rows * ld + MARGIN,), fill, dtype=t.dtype)
    buf[MARGIN + off: MARGIN + off + rows * ld].view(rows, ld)[:, :cols] = t
    return buf.to(device)


def gemm_kwargs(P, device, ws=None):
    """ops.gemm arguments of P with every operand inside margins (C is allocated per launch)."""
    c = P.c
    M, N, K = c["M"], c["N"], c["K"]
    kw = dict(M=M, N=N, K=K, ldb=P.ldb, B_off=MARGIN + P.B_off, ldc=P.ldc, C_off=MARGIN + P.C_off, act=c["act"],
              relu_a=c["relu_a"], accumulate=c["acc"], workspace=ws)
    if c["kind"] == "conv":
        q = c["conv"]
        A = _embed(P.x.reshape(1, -1), P.x.numel(), 0, device)
        kw.update(conv={k: q[k] for k in ("in_h", "in_w", "in_c", "k", "stride", "pad", "out_h", "out_w")}, A_off=MARGIN)
    else:
        A = _embed(P.A, P.lda, P.A_off, device)
        kw.update(lda=P.lda, A_off=MARGIN + P.A_off)
    B = _embed(P.B, P.ldb, P.B_off, device)
    vec = lambda t: None if t is None else _embed(t.reshape(1, -1), t.numel(), 0, device)[MARGIN:]   # noqa: E731
    kw.update(bias=vec(P.bias), gamma=vec(P.gamma), head_w=vec(P.head_w), head_b=P.head_b)
    if P.pos is not None:
        kw.update(pos=_embed(P.pos, P.ldpos, 0, device)[MARGIN:], ldpos=P.ldpos, pos_group=P.pos_group, pos_off=P.pos_off)
    if P.R1 is not None:
        kw.update(R1=_embed(P.R1, P.ldr1, 0, device)[MARGIN:], ldr1=P.ldr1)
    if P.R2 is not None:
        kw.update(R2=_embed(P.R2, P.ldr2, 0, device)[MARGIN:], ldr2=P.ldr2)
    if c["deconv"]:
        kw.update(deconv=c["deconv"])
    if P.row_group:
        kw.update(row_group=P.row_group, row_group_out=P.row_group_out, row_off=P.row_off)
    return A, B, kw


def plan_rc(A, B, C, kw, tile):
    a = ops._gemm_args(A, B, C, **dict(kw, tile=tile))
    t, g = ctypes.c_int32(), ctypes.c_int32()
    return _lib.load().dp_gemm_plan(ctypes.byref(a), ctypes.byref(t), ctypes.byref(g)), t.value


@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_plan_rejects_exactly_what_the_header_says(ci):
    """Host only: dp_gemm_plan's return code for every (hint, case) pair == the header-derived predicate, with
    and without a workspace (operand pointers are never dereferenced by the planner)."""
    P = problem(ci, torch.bfloat16)
    cpu = torch.device("cpu")
    A, B, kw = gemm_kwargs(P, cpu)
    C = prefill(P)
    ws_bytes = int(_lib.load().dp_gemm_workspace_size())
    ws = torch.empty(8, dtype=torch.uint8)
    for with_ws in (False, True):
        for tile in range(N_TILES):
            a = ops._gemm_args(A, B, C, **dict(kw, tile=tile))
            if with_ws:
                a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
            t, g = ctypes.c_int32(), ctypes.c_int32()
            rc = _lib.load().dp_gemm_plan(ctypes.byref(a), ctypes.byref(t), ctypes.byref(g))
            want = expected_rc(P, tile, ws_bytes if with_ws else 0)
            assert rc == want, f"{P.c['name']} tile {tile} workspace {with_ws}: plan {rc}, header {want}"
            assert not (tile == 0 and rc), "DP_TILE_AUTO must serve every case the header allows"


_STATE = {}


@pytest.fixture(scope="module")
def workspace(cuda):
    ws = ops.gemm_workspace(cuda)
    _STATE["ws"] = ws
    return ws


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_contract_on_every_engine(cuda, workspace, record, ci, dt):
    P = problem(ci, dt)
    A, B, kw = gemm_kwargs(P, cuda, workspace)
    ws_bytes = workspace.numel()
    pre = prefill(P)
    failures, worst, ran = [], float("-inf"), 0
    for tile in range(N_TILES):
        C = pre.to(cuda)
        rc, planned = plan_rc(A, B, C, kw, tile)
        want = expected_rc(P, tile, ws_bytes)
        assert rc == want, f"{P.c['name']} tile {tile}: plan {rc}, header says {want}"
        if rc:
            continue
        ops.gemm(A, B, C, **dict(kw, tile=tile))
        n_bad, n_canary, excess = verify(P, ci, C.cpu())
        ran += 1
        worst = max(worst, excess)
        if n_bad or n_canary:
            failures.append(f"tile {tile} (ran as {planned}): {n_bad} elements over the bound "
                            f"(largest excess {excess:.3e}), {n_canary} canaries changed")
    record("largest excess over the allowance-free bound", worst)
    print(f"{P.c['name']} {dt}: {ran} engines, largest excess over the allowance-free bound {worst:.3e}")
    assert ran >= 1
    assert not failures, f"{P.c['name']} {dt}:\n" + "\n".join(failures)


@pytest.mark.gpu
def test_zz_sticky_error_word_is_zero(cuda):
    """Last in the module: no stream-K launch above gave up waiting (dp_mi355x.h, DP_GEMM_WS_ERROR_OFFSET)."""
    ws = _STATE.get("ws")
    if ws is not None:
        assert ops.workspace_error(ws) == 0
