"""dp_attention / dp_attention_log2q (include/dp_mi355x.h) at their contract edges, against fp64.

Reference: the header's formula in fp64 on the CPU over the 16-bit qkv upcast exactly,
out = softmax(scale * Q K^T) V per (image, head).  For dp_attention_log2q the reference Q is the
rounded pre-scaled Q divided by gamma (the scale is rounded before the 16-bit Q, not after).

Per-element bound (not per tensor), for every element of out:

    |out - ref| <= u_out * |ref| + Z_out + 2 D / (1 - D) * A + Z          (+ EXP2_ALLOWANCE)
    A = softmax(...) @ |V|

The kernel computes out = sum_j P_j V_j / sum_j P_j with unnormalised weights P_j = 2^(t_j - m) (t:
score in log2 units, m: a running max common to the row).  If every P_j carries a relative
perturbation of at most D in the numerator and in the denominator, |out - ref| <= 2 D / (1 - D) A.
D is per query:

    D = u_p + expm1(ln 2 * 2 * (HD + 8) * 2^-24 * T) + 3 * (seq + 8) * 2^-24

  u_p   the RNE rounding of P to 16 bits for the P V MFMA (K_::pack2 / from_f): 2^-9 (bf16), 2^-12 (f16);
  T     max_j |sl2| sum_d |q_d| |k_jd|, sl2 = scale * log2 e.  An fp32 dot product of length HD = 64 in
        any order errs by at most HD 2^-24 sum_d |q_d| |k_d|; the 8 extra units cover the scale's own
        rounding to fp32, the scale multiply and the subtraction of m (an FMA, or the accumulator
        started at -m: |m| <= T, hence the factor 2).  An error e in log2 units moves P by expm1(ln 2 e);
  seq   terms: the fp32 row sum, the fp32 accumulation of P V (each (seq + 8) 2^-24 on sums of
        non-negative terms) and the multiplies of the exact path's rescales, 1 / rowsum and O * inv.

Z is absolute: a P below the 16-bit normal range is rounded on the subnormal grid (f16: spacing
2^-24, error <= 2^-25; bf16 shares fp32's range: below 2^-126, error <= 2^-126).  The kernel's m never
exceeds the row's true max, so its P_j >= 2^(t_j - max t) and its row sum >= L = sum_j 2^(t_j - max t):

    Z = z * sum_{j : t_j - max t < log2(z) + 12} |V_jd| / L,    z = 2^-25 (f16), 2^-126 (bf16)

(the 12: keys within a factor 2 of the normal range 2^11 z are counted too, for the score error).
u_out = 2^-8 (bf16), 2^-11 (f16) as in test_gemm_contract.py; an output below the 16-bit normal
range is rounded to half the subnormal spacing instead, which Z_out = 2^-25 (f16), 2^-134 (bf16)
adds.  The hardware exp2 (v_exp_f32) cannot be derived from the formats: EXP2_EXCESS_MEASURED below,
the GELU_EXCESS_MEASURED pattern.

Canaries: out carries 64 elements of a fixed 16-bit pattern before and after and is prefilled
with it, so an element never written fails the bound, and the margins must be bit-identical; qkv
carries two rows of NaN before and after, so a key past seq that leaks shows as NaN.  One NaN in V
must make exactly out[b, :, h, d] NaN.  Every case is launched twice: bit-identical outputs.

The CPU self-check (no GPU) shows the bound is neither too tight (an fp32 emulation of the
kernel's arithmetic -- max from the first 32 keys only, P rounded to 16 bits, fp32 sums, the exact
path when that goes non-finite -- passes every case with allowance 0) nor too loose (each seeded
mutation of it fails at least one named case).  The emulation's exact path moves a query's max by
its own scores (the kernel: when any query of the wave exceeds it by 8); both keep P <= 256.
"""

import functools
import math

import pytest
import torch

from depth_pro import ops

DTYPES = [torch.bfloat16, torch.float16]
HD = 64
MARGIN = 64                # elements of out before and after (a multiple of 8: 16-B alignment kept)
QKV_MARGIN_ROWS = 2
PAT16 = 0x5A5A             # bf16 1.5e16, f16 203.25
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
U_P = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}
SUB_OUT = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
Z_SUB = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -25}
LOG2E = ops.LOG2E
LN2 = math.log(2.0)

# v_exp_f32's own error is not derivable from the formats.  Measured on MI355X over every case of this
# module (both dtypes, both entry points) with allowance 0: the largest value of |out - ref| - bound.
# A negative value means no element exceeds the derived bound; the allowance is twice the excess, or 0.
EXP2_EXCESS_MEASURED = -4.848e-09
EXP2_EXCESS_CASE = "spike200_tile0_half1_seq577_key40, dp_attention, bf16"      # f16: -3.672e-07, grid_h7_b3_s130
EXP2_ALLOWANCE = 2.0 * max(EXP2_EXCESS_MEASURED, 0.0)


# ------------------------------------------------------------------------------------------ cases
def _case(name, heads, batch, seq, **kw):
    c = dict(name=name, heads=heads, batch=batch, seq=seq, qscale=2.0, scale=None, spikes=(), spike_ref="first",
             nan_v=None, cancel=False)
    c.update(kw)
    return c


def _cases():
    cs = []
    for i, seq in enumerate([1, 2, 31, 32, 33, 63, 64, 65, 66, 67, 96, 97, 127, 128, 129, 130, 192, 193, 194, 195,
                             256, 258, 577, 640]):
        cs.append(_case(f"seq{seq}", 2, 1 + (seq < 100), seq, qscale=(2.0, 0.25)[i % 2]))
    # workgroups = ceil(seq / 128) * heads * batch: every remainder mod 8 of the XCD remap
    for heads, batch, seq in [(1, 1, 64), (1, 2, 64), (3, 1, 64), (1, 2, 130), (5, 1, 64), (3, 1, 130), (7, 1, 64),
                              (16, 1, 33), (3, 3, 258), (5, 2, 577), (12, 1, 130), (7, 3, 130), (5, 3, 100),
                              (3, 5, 129)]:
        nwg = -(-seq // 128) * heads * batch
        cs.append(_case(f"grid_h{heads}_b{batch}_s{seq}_wg{nwg}_r{nwg % 8}", heads, batch, seq))
    for scale, sn in ((HD ** -0.5, "default"), (0.07, "0.07"), (1.0, "1.0"), (0.0, "0")):
        for seq in (100, 130, 577):
            cs.append(_case(f"scale{sn}_seq{seq}", 2, 1, seq, scale=scale, qscale=0.25))
    # spikes: key j = f * query 0's row, L log2 units above the first half tile's max of query 0
    for seq, j, where in [(577, 5, "sets_max"), (577, 40, "tile0_half1"), (577, 200, "steady"), (577, 575, "last_full"),
                          (100, 90, "partial"), (577, 576, "tail"), (130, 128, "tail0"), (130, 129, "tail1")]:
        for L in (10, 20, 200):
            cs.append(_case(f"spike{L}_{where}_seq{seq}_key{j}", 2, 1, seq, qscale=0.25, spikes=((j, float(L)),)))
    stairs = (40, 70, 130, 300, 575, 576)
    cs.append(_case("stair_f16_redo", 2, 1, 577, qscale=0.25, spikes=tuple((j, 9.0 * (i + 1)) for i, j in enumerate(stairs))))
    cs.append(_case("stair_both_redo", 2, 1, 577, qscale=0.25,
                    spikes=tuple((j, 130.0 + 9.0 * (i + 1)) for i, j in enumerate(stairs))))
    cs.append(_case("stair_partial_seq100", 2, 1, 100, qscale=0.25,
                    spikes=tuple((j, 130.0 + 9.0 * (i + 1)) for i, j in enumerate((33, 50, 64, 70, 96, 99)))))
    cs.append(_case("reverse_key3_seq577", 2, 1, 577, qscale=0.25, spikes=((3, 200.0),), spike_ref="all"))
    cs.append(_case("reverse_key3_seq100", 2, 1, 100, qscale=0.25, spikes=((3, 200.0),), spike_ref="all"))
    cs.append(_case("cancel_seq258", 2, 1, 258, qscale=0.01, cancel=True))
    cs.append(_case("cancel_seq64", 1, 1, 64, qscale=0.01, cancel=True))
    for seq, j in ((577, 300), (577, 576), (100, 99), (64, 0)):       # (b, key, head, d) of the NaN
        cs.append(_case(f"nanV_seq{seq}_key{j}", 3, 2, seq, qscale=0.25, nan_v=(1, j, 1, 37)))
    return cs


CASES = _cases()
CASE_IDS = [c["name"] for c in CASES]
ENTRIES = ["attention", "log2q"]


def _runs(c, log2q):
    """dp_attention_log2q has no scale argument: the scale cases run on dp_attention only."""
    return not (log2q and c["scale"] is not None)


LAUNCHES = [(ci, e) for ci, c in enumerate(CASES) for e in ENTRIES if _runs(c, e == "log2q")]


# ------------------------------------------------------------------------- seeded problem instances
class Problem:
    """One case in one dtype: qkv [B][seq][3][H][64] (16 bits, CPU) and the log2q entry's pre-scaled copy."""


def _scale(c):
    return HD ** -0.5 if c["scale"] is None else c["scale"]


@functools.lru_cache(maxsize=None)
def problem(ci, dt):
    c = CASES[ci]
    g = torch.Generator().manual_seed(4000 + ci)
    B, S, H = c["batch"], c["seq"], c["heads"]
    x = torch.randn(B, S, 3, H, HD, generator=g)
    x[:, :, 0] *= c["qscale"]
    x[:, :, 1] *= 2.0
    x[:, :, 2] *= 2.0 ** (torch.arange(HD) % 8 - 4).float()                    # small V columns matter
    if c["cancel"]:         # near-uniform weights over V = +-1 (alternating keys) + noise: out ~ 0, A ~ 1
        sign = (1 - 2 * (torch.arange(S) % 2)).float().view(1, S, 1, 1)
        x[:, :, 2] = sign + 0.01 * torch.randn(B, S, H, HD, generator=g)
    qkv = x.to(dt)
    sl2 = _scale(c) * LOG2E
    for j, L in c["spikes"]:
        q0 = qkv[:, 0, 0].double()                                              # [B][H][64]
        T0 = sl2 * torch.einsum("bhd,bkhd->bhk", q0, qkv[:, :, 1].double())     # query 0's scores, log2 units
        others = torch.ones(S, dtype=torch.bool)
        others[[jj for jj, _ in c["spikes"]]] = False
        if c["spike_ref"] == "first":
            others[32:] = False
        base = T0[:, :, others].max(-1).values
        f = (base + L) / (sl2 * (q0 * q0).sum(-1))
        qkv[:, j, 1] = (f.unsqueeze(-1) * q0).to(dt)
    if c["nan_v"]:
        b, j, h, d = c["nan_v"]
        qkv[b, j, 2, h, d] = float("nan")
    P = Problem()
    P.c, P.dt, P.qkv = c, dt, qkv
    P.gamma = torch.ones(3, H, HD)
    P.gamma[0] = float(HD ** -0.5 * LOG2E)                                      # ops.log2q_gamma, fp32
    P.qkv_in = (qkv.float() * P.gamma).to(dt)                                   # what the qkv epilogue writes
    return P


def qkv_buffer(P, log2q):
    """[2 + B * seq + 2][3 * H * 64] with NaN margin rows."""
    c = P.c
    ld = 3 * c["heads"] * HD
    body = (P.qkv_in if log2q else P.qkv).reshape(-1, ld)
    nan = torch.full((QKV_MARGIN_ROWS, ld), float("nan"), dtype=P.dt)
    return torch.cat([nan, body, nan])


def prefill(P):
    n = P.c["batch"] * P.c["seq"] * P.c["heads"] * HD
    return torch.full((MARGIN + n + MARGIN,), PAT16, dtype=torch.int16).view(P.dt)


# -------------------------------------------------------------------------------- reference + bound
@functools.lru_cache(maxsize=None)
def reference(ci, dt, log2q):
    """(ref, bound, nan_cols) in fp64, [B][seq][H][64]; nan_cols [B][H][64]: columns that must be NaN."""
    P = problem(ci, dt)
    c = P.c
    S = c["seq"]
    x = (P.qkv_in if log2q else P.qkv).double()
    q, k, v = x[:, :, 0], x[:, :, 1], x[:, :, 2]
    scale = _scale(c)
    if log2q:
        q = q / P.gamma[0].double()
    nan_cols = v.isnan().any(1)                                                 # [B][H][64]
    v = torch.nan_to_num(v, nan=0.0)
    sl2 = scale * LOG2E
    T = sl2 * torch.einsum("bqhd,bkhd->bhqk", q, k)                             # log2 units
    Tabs = abs(sl2) * torch.einsum("bqhd,bkhd->bhqk", q.abs(), k.abs()).max(-1).values      # [B][H][seq]
    W = torch.softmax(T * LN2, -1)
    ref = torch.einsum("bhqk,bkhd->bqhd", W, v)
    A = torch.einsum("bhqk,bkhd->bqhd", W, v.abs())
    D = U_P[dt] + torch.expm1(LN2 * 2 * (HD + 8) * 2.0 ** -24 * Tabs) + 3 * (S + 8) * 2.0 ** -24
    rel = T - T.max(-1, keepdim=True).values
    small = (rel < math.log2(Z_SUB[dt]) + 12).double()
    L = torch.exp2(rel).sum(-1)                                                 # >= 1
    Z = Z_SUB[dt] * torch.einsum("bhqk,bkhd->bqhd", small, v.abs()) / L.permute(0, 2, 1).unsqueeze(-1)
    bound = U_OUT[dt] * ref.abs() + SUB_OUT[dt] + (2 * D / (1 - D)).permute(0, 2, 1).unsqueeze(-1) * A + Z
    if c["scale"] == 0.0:   # the reference itself: softmax of zeros is the plain mean of V
        assert torch.allclose(ref, v.mean(1, keepdim=True).expand_as(ref), rtol=1e-12, atol=1e-14)
    return ref, bound, nan_cols


def verify(P, ci, log2q, out, allowance=EXP2_ALLOWANCE):
    """out: the flat allocation after the call (CPU).  (elements over the bound or wrongly (non-)NaN,
    margin elements changed, largest excess over the allowance-free bound)."""
    ref, bound, nan_cols = reference(ci, P.dt, log2q)
    body = out[MARGIN:-MARGIN].view(ref.shape).double()
    must_nan = nan_cols.unsqueeze(1).expand_as(ref)
    excess = (body - ref).abs() - bound
    bad = torch.where(must_nan, ~body.isnan(), ~(excess <= allowance))         # NaN elsewhere counts as bad
    pat = prefill(P).view(torch.int16)
    bits = out.view(torch.int16)
    n_canary = int((bits[:MARGIN] != pat[:MARGIN]).sum() + (bits[-MARGIN:] != pat[-MARGIN:]).sum())
    worst = torch.nan_to_num(excess, nan=float("inf"))[~must_nan].max()
    return int(bad.sum()), n_canary, float(worst)


# ----------------------------------------------------------------- the kernel's arithmetic in fp32
def _exact_rows(Ssc, V, dt, mut):
    """The exact path over 32-key steps: Ssc [n][keys] scores in log2 units (fp32)."""
    n, nk = Ssc.shape
    m = torch.full((n,), float("-inf"))
    l = torch.zeros(n)
    O = torch.zeros(n, HD)
    for k0 in range(0, nk, 32):
        s = Ssc[:, k0:k0 + 32]
        mn = s.max(1).values
        m_new = torch.where(mn > m + 8.0, torch.maximum(m, mn), m)
        alpha = torch.exp2(m - m_new)
        alpha = torch.where(m == m_new, torch.ones_like(alpha), alpha)         # (-inf) - (-inf)
        if mut != "no_rescale":                                                  # mutation: O keeps the old frame
            O = O * alpha.unsqueeze(1)
        l = l * alpha
        m = m_new
        p = torch.exp2(s - m.unsqueeze(1))
        l = l + p.sum(1)
        O = O + p.to(dt).float() @ V[k0:k0 + 32]
    return O, l


def emulate(P, log2q, mut=None):
    """A correct kernel in fp32 on the CPU, or a seeded mutation of it: the out allocation after the call."""
    c, dt = P.c, P.dt
    B, S, H = c["batch"], c["seq"], c["heads"]
    rows = qkv_buffer(P, log2q).float()
    out = prefill(P)
    body = out[MARGIN:-MARGIN].view(B, S, H, HD)
    sl2 = torch.tensor(1.0 if log2q else _scale(c) * LOG2E, dtype=torch.float32)
    if mut == "scale":                                                           # mutation: scale * (1 + 2^-7)
        sl2 = sl2 * (1 + 2.0 ** -7)
    nk = S - 1 if mut == "drop_last" and S > 1 else S + 1 if mut == "past_seq" else S     # mutations: keys seen
    for b in range(B):
        r0 = QKV_MARGIN_ROWS + b * S
        for h in range(H):
            hv = h - 1 if mut == "v_neighbour" and h == H - 1 else h             # mutation: last head, wrong V
            Q = rows[r0:r0 + S, h * HD:(h + 1) * HD]
            K = rows[r0:r0 + nk, (H + h) * HD:(H + h + 1) * HD]
            V = rows[r0:r0 + nk, (2 * H + hv) * HD:(2 * H + hv + 1) * HD]
            Ssc = (Q @ K.t()) * sl2
            m = Ssc[:, :min(32, nk)].max(1).values                              # the first half tile only
            p = torch.exp2(Ssc - m.unsqueeze(1))
            pr = p.to(dt).float()
            tail = nk % 64 if 0 < nk % 64 <= 2 else 0                           # VALU tail keys add the rounded P
            l = p[:, :nk - tail].sum(1) + pr[:, nk - tail:].sum(1)
            O = pr @ V
            for q0 in range(0, S, 128):                                          # one workgroup's redo
                blk = slice(q0, min(q0 + 128, S))
                if not (torch.isfinite(O[blk]).all() and torch.isfinite(l[blk]).all()):
                    O[blk], l[blk] = _exact_rows(Ssc[blk], V, dt, mut)
            res = (O * (1.0 / l).unsqueeze(1)).to(dt)
            if mut == "unwritten" and b == B - 1 and h == H - 1:                 # mutation: one item never stored
                res[S - 1 - (S - 1) % 128:] = body[b, S - 1 - (S - 1) % 128:, h]
            body[b, :, h] = res
    return out


MUTATIONS = ["drop_last", "past_seq", "v_neighbour", "scale", "no_rescale", "unwritten"]


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_selfcheck_fp32_emulation_passes(dt, entry):
    """(a) the bound is not tighter than a correct fp32 kernel can meet, with no allowance."""
    log2q = entry == "log2q"
    for ci, c in enumerate(CASES):
        if not _runs(c, log2q):
            continue
        P = problem(ci, dt)
        n_bad, n_canary, excess = verify(P, ci, log2q, emulate(P, log2q), allowance=0.0)
        assert n_bad == 0 and n_canary == 0, f"{c['name']}: {n_bad} over the bound (excess {excess:.3e}), {n_canary} canaries"


@pytest.mark.parametrize("mut", MUTATIONS)
def test_selfcheck_mutation_is_caught(mut):
    """(b) a subtly wrong kernel fails at least one named case (bf16, the wider bound)."""
    caught = []
    for ci, c in enumerate(CASES):
        P = problem(ci, torch.bfloat16)
        n_bad, n_canary, _ = verify(P, ci, False, emulate(P, False, mut), allowance=1e-5)
        if n_bad or n_canary:
            caught.append(c["name"])
    print(f"mutation {mut}: caught by {len(caught)} cases, e.g. {caught[:6]}")
    assert caught, f"mutation {mut} passes every case"


def test_cases_cover_what_they_claim():
    """Every XCD-remap remainder 0..7 occurs, at least three of them with more than 8 workgroups."""
    nwg = [-(-c["seq"] // 128) * c["heads"] * c["batch"] for c in CASES]
    assert {n % 8 for n in nwg} == set(range(8))
    assert len({n % 8 for n in nwg if n > 8}) >= 3
    assert {1, 3, 5, 7, 12, 16} <= {c["heads"] for c in CASES}


# ------------------------------------------------------------------------------- launching a case
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("ci,entry", LAUNCHES, ids=[f"{CASE_IDS[ci]}-{e}" for ci, e in LAUNCHES])
def test_contract(cuda, record, ci, entry, dt):
    c = CASES[ci]
    log2q = entry == "log2q"
    P = problem(ci, dt)
    ld = 3 * c["heads"] * HD
    qkv = qkv_buffer(P, log2q).to(cuda)
    outs = []
    for _ in range(2):
        out = prefill(P).to(cuda)
        ops.attention(qkv[QKV_MARGIN_ROWS:].reshape(-1)[:c["batch"] * c["seq"] * ld], out[MARGIN:], c["batch"],
                      c["seq"], c["heads"], HD, log2q=log2q, scale=c["scale"])
        outs.append(out.cpu())
    n_bad, n_canary, excess = verify(P, ci, log2q, outs[0])
    record("largest excess over the allowance-free bound", excess)
    print(f"EXCESS {c['name']} {entry} {dt}: {excess:.3e}")
    assert n_bad == 0 and n_canary == 0, \
        f"{c['name']} {entry} {dt}: {n_bad} elements over the bound (largest excess {excess:.3e}), {n_canary} canaries changed"
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "two launches differ"
    if c["scale"] == 0.0:               # the plain mean of V, to the output rounding and the fp32 sums
        mean = P.qkv[:, :, 2].double().mean(1, keepdim=True)
        amean = P.qkv[:, :, 2].double().abs().mean(1, keepdim=True)
        got = outs[0][MARGIN:-MARGIN].view(c["batch"], c["seq"], c["heads"], HD).double()
        lim = U_OUT[dt] * mean.abs() + 2 * (U_P[dt] + 3 * (c["seq"] + 8) * 2.0 ** -24) * amean * 1.01
        assert bool(((got - mean).abs() <= lim).all()), "scale 0 is not the mean of V"
