"""dp_layernorm, dp_layernorm_grouped and dp_layernorm_stats (include/dp_mi355x.h) at their contract
edges, against fp64.

Reference: fp64 on the CPU, y = (x - mean) / sqrt(var + eps) * w + b with the biased variance.

Per-element bound for the two-pass fp32 kernels (u = 2^-24).  The kernels sum a row as a tree: a
lane adds its <= 32 values in <= 10 dependent additions, six cross-lane steps follow, so no input
passes through more than T = 18 roundings (the 1 / cols multiply included); any tree of that depth
obeys |sum^ - sum| <= T u sum |x|.  With mabs = mean |x|, d = x - mean, r = (var + eps)^-1/2:

    dm    = T u mabs                                            error of the mean
    var^  = (var + dm'^2)(1 + theta), |theta| <= (T + 6) u      sum (x - mean^)^2 = sum d^2 + n dm'^2 exactly,
                                                                dm' <= dm; squares and subtractions: 6 u
    rel_r = ((T + 8) u var + 2 dm^2) / (2 (var + eps)) + 4 u    d r / r = -1/2 d(var + eps) / (var + eps); rsqrt, + eps
    |y - ref| <= u_out |ref| + |w| r (dm + |d| (rel_r + 6 u)) + 2 u (|w| |d| r + |b|)

u_out = 2^-8 (bf16), 2^-11 (f16); an output below the 16-bit normal range is rounded on the
subnormal grid instead, to half its spacing: + 2^-25 (f16), 2^-134 (bf16).  A constant row c (c cols
exactly representable) has mean^ = c and d = 0 exactly: its output must equal b in 16 bits bit for
bit.  A row holding a NaN is NaN throughout and no other row is.

dp_layernorm_stats: xb == x.to(dtype) bit for bit (a NaN as any NaN); xl == the int8 low part of
ops.split_residual bit for bit and hi + lo restores x to 4e-5 |x| + (1e-36 bf16 / 6e-8 f16), where
hi is finite (the bound test_layernorm_stats_split_residual states); each 128-column chunk's
(mean, M2) against fp64 with the same tree argument at depth Ts = 10 (3 in-lane, 4 cross-lane
steps, the multiply, slack):

    |mean^ - mean| <= dm = Ts u mabs;    |M2^ - M2| <= (Ts + 6) u (M2 + 128 dm^2) + 128 dm^2

Canaries: every output carries 64 elements before and after, the [cols, ld) padding and two rows
past the end, all holding a fixed bit pattern that must be bit-identical after the call (outputs
are prefilled with it, so an element never written fails its bound); inputs carry the same margins
filled with NaN, so a load outside the rows shows.

The CPU self-check (no GPU) shows the bounds are not too tight (a two-pass fp32 evaluation passes
every case) and not too loose (each seeded mutation of it fails at least one named case).
"""

import ctypes
import functools

import pytest
import torch

from depth_pro import _lib, ops

DTYPES = [torch.bfloat16, torch.float16]
MARGIN = 64
PAT16, PAT32, PAT8 = 0x5A5A, 0x5A5A5A5A, 0x5A          # 16-bit, fp32 (1.5e16) and int8 prefill
U = 2.0 ** -24
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SUB_OUT = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
T_LN, T_STATS = 18, 10
EPS = 1e-6
ROW_KINDS = ["normal_1_3", "constant", "mean_1e4", "spread_1e-4", "outlier_1e6", "nan"]


# ------------------------------------------------------------------------------------------ cases
def _cases():
    cs = []
    lds = [(0, 0), (4, 8), (64, 8)]                     # (ldx - cols, ldy - cols)
    i = 0
    for cols in (256, 512, 1024, 2048):
        for rows in (1, 2, 3, 4, 5, 7, 9):
            dx, dy = lds[i % 3]
            cs.append(dict(name=f"ln_c{cols}_r{rows}_ldx+{dx}_ldy+{dy}", kind="ln", cols=cols, groups=1, rpg=rows,
                           ldx=cols + dx, ldy=cols + dy))
            i += 1
    for groups in (1, 2, 3, 4):
        for rpg in (1, 3, 5):
            cols = (256, 512, 1024, 2048)[i % 4]
            dx, dy = lds[i % 3]
            cs.append(dict(name=f"grouped_g{groups}x{rpg}_c{cols}_ldx+{dx}_ldy+{dy}", kind="grouped", cols=cols,
                           groups=groups, rpg=rpg, ldx=cols + dx, ldy=cols + dy))
            i += 1
    for cols in (512, 1024, 2048):
        for rows in (1, 2, 3, 4, 5, 7, 9):
            dx, dy = lds[i % 3]
            cs.append(dict(name=f"stats_c{cols}_r{rows}_ldx+{dx}_ldxb+{dy}_xl{i % 2}", kind="stats", cols=cols, groups=1,
                           rpg=rows, ldx=cols + dx, ldy=cols + dy, xl=bool(i % 2)))
            i += 1
    return cs


CASES = _cases()
CASE_IDS = [c["name"] for c in CASES]


class Problem:
    """CPU tensors of one case: x [rows][cols] fp32, w / b per group."""


@functools.lru_cache(maxsize=None)
def problem(ci):
    c = CASES[ci]
    g = torch.Generator().manual_seed(7000 + ci)
    rows, cols = c["groups"] * c["rpg"], c["cols"]
    x = torch.empty(rows, cols)
    kinds = []
    for r in range(rows):
        k = ROW_KINDS[(r + ci) % len(ROW_KINDS)]
        z = torch.randn(cols, generator=g)
        if k == "normal_1_3":
            x[r] = 1 + 3 * z
        elif k == "constant":
            x[r] = 1.5
        elif k == "mean_1e4":
            x[r] = 1e4 + z
        elif k == "spread_1e-4":
            x[r] = 0.5 + 1e-4 * z                       # variance 1e-8 < eps
        elif k == "outlier_1e6":
            x[r] = z
            x[r, (37 * ci + 5) % cols] = 1e6
        else:
            x[r] = 1 + 3 * z
            x[r, (91 * ci + 130) % cols] = float("nan")
        kinds.append(k)
    P = Problem()
    P.c, P.x, P.rows, P.kinds = c, x, rows, kinds
    P.w = [torch.randn(cols, generator=g) for _ in range(c["groups"])]
    P.b = [torch.randn(cols, generator=g) for _ in range(c["groups"])]
    return P


def _wb(P, which, mut=None):
    """[rows][cols] affine parameters of every row (mutation: a group takes its neighbour's w)."""
    G = P.c["groups"]
    sel = [(g + 1) % G if (mut == "neighbour_w" and which == "w") else g for g in range(G)]
    src = P.w if which == "w" else P.b
    return torch.stack([src[sel[r // P.c["rpg"]]] for r in range(P.rows)])


# -------------------------------------------------------------------------------- reference + bound
@functools.lru_cache(maxsize=None)
def reference_ln(ci, dt):
    P = problem(ci)
    x, w, b = P.x.double(), _wb(P, "w").double(), _wb(P, "b").double()
    mean = x.mean(1, keepdim=True)
    d = x - mean
    var = (d * d).mean(1, keepdim=True)
    r = (var + EPS).rsqrt()
    ref = d * r * w + b
    dm = T_LN * U * x.abs().mean(1, keepdim=True)
    rel_r = ((T_LN + 8) * U * var + 2 * dm * dm) / (2 * (var + EPS)) + 4 * U
    bound = U_OUT[dt] * ref.abs() + SUB_OUT[dt] + w.abs() * r * (dm + d.abs() * (rel_r + 6 * U)) + \
        2 * U * (w.abs() * d.abs() * r + b.abs())
    return ref, bound


@functools.lru_cache(maxsize=None)
def reference_stats(ci):
    """(ref, bound) [rows][cols / 128][2] of the chunk (mean, M2)."""
    P = problem(ci)
    x = P.x.double().view(P.rows, -1, 128)
    mean = x.mean(2)
    M2 = ((x - mean.unsqueeze(2)) ** 2).sum(2)
    dm = T_STATS * U * x.abs().mean(2)
    bM2 = (T_STATS + 6) * U * (M2 + 128 * dm * dm) + 128 * dm * dm
    return torch.stack([mean, M2], 2), torch.stack([dm, bM2], 2)


# ----------------------------------------------------------------------------- buffers with margins
def _alloc(rows, ld, dtype, fill):
    n = MARGIN + (rows + 2) * ld + MARGIN
    if dtype in DTYPES:
        return torch.full((n,), fill, dtype=torch.int16).view(dtype)
    if dtype == torch.int8:
        return torch.full((n,), fill, dtype=torch.int8)
    if isinstance(fill, int):
        return torch.full((n,), fill, dtype=torch.int32).view(torch.float32)
    return torch.full((n,), fill, dtype=torch.float32)


def _body(buf, rows, ld, cols):
    return buf[MARGIN:MARGIN + rows * ld].view(rows, ld)[:, :cols]


def _embed(t, ld):
    """fp32 [rows][cols] inside NaN margins, padding and two NaN rows past the end."""
    buf = _alloc(t.shape[0], ld, torch.float32, float("nan"))
    _body(buf, t.shape[0], ld, t.shape[1])[:] = t
    return buf


def _canaries_changed(buf, fresh, rows, ld, cols):
    keep = torch.ones(buf.numel(), dtype=torch.bool)
    _body(keep, rows, ld, cols)[:] = False
    bits = {2: torch.int16, 4: torch.int32, 1: torch.int8}[buf.element_size()]
    return int((buf.view(bits)[keep] != fresh.view(bits)[keep]).sum())


class Out:
    """The output allocations of one call (CPU)."""


def fresh_outputs(P, dt):
    c = P.c
    o = Out()
    if c["kind"] == "stats":
        nch = c["cols"] // 128
        o.xb = _alloc(P.rows, c["ldy"], dt, PAT16)
        o.xl = _alloc(P.rows, c["ldy"], torch.int8, PAT8) if c["xl"] else None
        o.part = _alloc(P.rows, 2 * nch, torch.float32, PAT32)
    else:
        o.y = _alloc(P.rows, c["ldy"], dt, PAT16)
    return o


def verify(P, ci, dt, o):
    """List of what is wrong with the outputs `o` of case ci (empty: the contract holds)."""
    c = P.c
    rows, cols = P.rows, c["cols"]
    f = fresh_outputs(P, dt)
    nan_row = P.x.isnan().any(1)
    msgs = []
    if c["kind"] == "stats":
        nch = cols // 128
        xb = _body(o.xb, rows, c["ldy"], cols)
        want = P.x.to(dt)                # (a NaN stays a NaN; its payload bits are the converter's own)
        num = ~P.x.isnan()
        n_diff = int((xb.view(torch.int16) != want.view(torch.int16))[num].sum()) + int((~xb.isnan())[~num].sum())
        if n_diff:
            msgs.append(f"xb != x.to(dtype) in {n_diff} elements")
        if _canaries_changed(o.xb, f.xb, rows, c["ldy"], cols):
            msgs.append("xb canaries changed")
        if c["xl"]:
            xl = _body(o.xl, rows, c["ldy"], cols)
            hi, q = ops.split_residual(P.x, dt)
            ok = torch.isfinite(hi.float())
            if not torch.equal(xl[ok], q[ok]):
                msgs.append("xl != the low part of split_residual")
            err = (ops.merge_residual(xb, xl) - P.x).abs()
            lim = 4e-5 * P.x.abs() + (1e-36 if dt == torch.bfloat16 else 6e-8)
            if not bool((err <= lim)[ok].all()):
                msgs.append("hi + lo does not restore x")
            if _canaries_changed(o.xl, f.xl, rows, c["ldy"], cols):
                msgs.append("xl canaries changed")
        ref, bound = reference_stats(ci)
        part = _body(o.part, rows, 2 * nch, 2 * nch).view(rows, nch, 2).double()
        excess = (part - ref).abs() - bound
        bad = torch.where(ref.isnan(), ~part.isnan(), ~(excess <= 0))
        if bad.any():
            msgs.append(f"{int(bad.sum())} chunk statistics over the bound (largest excess "
                        f"{float(torch.nan_to_num(excess, nan=0.0).max()):.3e})")
        if _canaries_changed(o.part, f.part, rows, 2 * nch, 2 * nch):
            msgs.append("part canaries changed")
        return msgs
    ref, bound = reference_ln(ci, dt)
    y = _body(o.y, rows, c["ldy"], cols)
    excess = (y.double() - ref).abs() - bound
    bad = torch.where(nan_row.unsqueeze(1).expand_as(ref), ~y.isnan(), ~(excess <= 0))
    if bad.any():
        msgs.append(f"{int(bad.sum())} elements over the bound (largest excess "
                    f"{float(torch.nan_to_num(excess, nan=0.0).max()):.3e})")
    for r, k in enumerate(P.kinds):
        if k == "constant" and not torch.equal(y[r].view(torch.int16), _wb(P, "b")[r].to(dt).view(torch.int16)):
            msgs.append(f"constant row {r} is not exactly b")
    if _canaries_changed(o.y, f.y, rows, c["ldy"], cols):
        msgs.append("y canaries changed")
    return msgs


# ----------------------------------------------------------- a two-pass fp32 evaluation + mutations
def emulate(P, dt, mut=None):
    c = P.c
    rows, cols = P.rows, c["cols"]
    o = fresh_outputs(P, dt)
    keep = cols - 8 if mut == "last8" else cols          # mutation: the last 8 columns unwritten
    x = P.x
    if c["kind"] == "stats":
        nch = cols // 128
        _body(o.xb, rows, c["ldy"], cols)[:, :keep] = x.to(dt)[:, :keep]
        if c["xl"]:
            _body(o.xl, rows, c["ldy"], cols)[:, :keep] = ops.split_residual(x, dt)[1][:, :keep]
        xc = x.view(rows, nch, 128)
        mean = xc.sum(2) * (1.0 / 128)
        if mut == "var_e2":                              # mutation: E[x^2] - mean^2
            M2 = (xc * xc).sum(2) - 128 * mean * mean
        else:
            M2 = ((xc - mean.unsqueeze(2)) ** 2).sum(2)
        _body(o.part, rows, 2 * nch, 2 * nch)[:] = torch.stack([mean, M2], 2).view(rows, 2 * nch)
        return o
    w, b = _wb(P, "w", mut), _wb(P, "b")
    mean = x.sum(1, keepdim=True) * (1.0 / cols)
    d = x - mean
    if mut == "var_e2":
        var = (x * x).sum(1, keepdim=True) * (1.0 / cols) - mean * mean
    else:
        var = (d * d).sum(1, keepdim=True) * (1.0 / cols)
    r = torch.rsqrt(var + (0.0 if mut == "no_eps" else EPS))         # mutation: eps missing
    _body(o.y, rows, c["ldy"], cols)[:, :keep] = (d * r * w + b).to(dt)[:, :keep]
    return o


MUTATIONS = ["var_e2", "no_eps", "neighbour_w", "last8"]


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
def test_selfcheck_two_pass_fp32_passes(dt):
    """(a) the bounds are not tighter than a correct two-pass fp32 kernel can meet."""
    for ci, c in enumerate(CASES):
        P = problem(ci)
        msgs = verify(P, ci, dt, emulate(P, dt))
        assert not msgs, f"{c['name']}: {msgs}"


@pytest.mark.parametrize("mut", MUTATIONS)
def test_selfcheck_mutation_is_caught(mut):
    """(b) a subtly wrong kernel fails at least one named case (bf16, the wider bound)."""
    caught = [c["name"] for ci, c in enumerate(CASES)
              if verify(problem(ci), ci, torch.bfloat16, emulate(problem(ci), torch.bfloat16, mut))]
    print(f"mutation {mut}: caught by {len(caught)} cases, e.g. {caught[:6]}")
    assert caught, f"mutation {mut} passes every case"


def test_cases_cover_what_they_claim():
    """Every row kind occurs in every kernel family; group boundaries fall inside a block of 4 rows."""
    for kind in ("ln", "grouped", "stats"):
        seen = {k for ci, c in enumerate(CASES) if c["kind"] == kind for k in problem(ci).kinds}
        assert seen == set(ROW_KINDS), (kind, seen)
    assert any(c["kind"] == "grouped" and c["groups"] > 1 and c["rpg"] % 4 for c in CASES)


# ------------------------------------------------------------------------------- launching a case
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_contract(cuda, ci, dt):
    P = problem(ci)
    c = P.c
    rows, cols = P.rows, c["cols"]
    lib = _lib.load()
    x = _embed(P.x, c["ldx"]).to(cuda)
    ws = [_embed(t.view(1, -1), cols).to(cuda) for t in P.w]
    bs = [_embed(t.view(1, -1), cols).to(cuda) for t in P.b]
    code = ops.dtype_code(dt)
    runs = []
    for _ in range(2):
        o = fresh_outputs(P, dt)
        dev = {k: (v.to(cuda) if v is not None else None) for k, v in vars(o).items()}
        ptr = lambda t: t[MARGIN:].data_ptr()            # noqa: E731
        if c["kind"] == "stats":
            rc = lib.dp_layernorm_stats(ptr(x), c["ldx"], rows, cols, ptr(dev["xb"]), c["ldy"],
                                        ptr(dev["xl"]) if c["xl"] else None, ptr(dev["part"]), code, ops._stream(x))
        elif c["kind"] == "ln":
            rc = lib.dp_layernorm(ptr(x), c["ldx"], ptr(ws[0]), ptr(bs[0]), ptr(dev["y"]), c["ldy"], rows, cols,
                                  EPS, code, ops._stream(x))
        else:
            pw = (ctypes.c_void_p * c["groups"])(*[ptr(t) for t in ws])
            pb = (ctypes.c_void_p * c["groups"])(*[ptr(t) for t in bs])
            rc = lib.dp_layernorm_grouped(ptr(x), c["ldx"], pw, pb, c["groups"], ptr(dev["y"]), c["ldy"], c["rpg"],
                                          cols, EPS, code, ops._stream(x))
        _lib.check(rc, c["name"])
        for k, v in dev.items():
            setattr(o, k, v.cpu() if v is not None else None)
        runs.append(o)
    msgs = verify(P, ci, dt, runs[0])
    assert not msgs, f"{c['name']} {dt}: {msgs}"
    for k, v in vars(runs[0]).items():
        if v is not None:
            assert torch.equal(v.view(torch.uint8), getattr(runs[1], k).view(torch.uint8)), f"two launches differ in {k}"
