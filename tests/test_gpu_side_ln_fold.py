"""The folded-LayerNorm forms of dp_gemm_grouped (the side encoders' proj / fc2 producers and qkv /
fc1 consumers on the grouped 128 x 128 tile) against fp64, two groups with their own weights.

M = 130 rows per group: one full 128-row tile and one 2-row tile.  Measured figures (MI355X) are
quoted in the docstrings and in profiles/side_ln_fold/README.md.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from depth_pro import _lib, ops  # noqa: E402
from depth_pro._lib import DP_ACT_GELU  # noqa: E402

DTYPES = [torch.bfloat16, torch.float16]
M, G = 130, 2
OFFSET_ROWS = (3, 129)      # rows (of each group) whose C values are 300 +- 1


def _rnd(*shape, gen, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


def _chunk_stats64(c):
    """fp64 (mean, M2) per 128-column chunk of c [rows][N] -> [rows][N/128][2]."""
    x = c.double().reshape(c.shape[0], -1, 128)
    mean = x.mean(2)
    return torch.stack((mean, ((x - mean[..., None]) ** 2).sum(2)), 2)


def _part_err(part, ref):
    """(max |mean - ref| / max |ref mean|, max relative M2 error)."""
    part, ref = part.double().cpu(), ref.cpu()
    e_mean = ((part[..., 0] - ref[..., 0]).abs().max() / ref[..., 0].abs().max()).item()
    e_m2 = ((part[..., 1] - ref[..., 1]).abs() / ref[..., 1]).max().item()
    return e_mean, e_m2


def _producer_case(cuda, dt, K, seed=3):
    g = torch.Generator().manual_seed(seed + K)
    N = 1024
    A = _rnd(G * M, K, gen=g).to(dt).to(cuda)
    C0 = _rnd(G * M, N, gen=g)
    for r in OFFSET_ROWS:
        for i in range(G):
            C0[i * M + r] = 300.0 + (torch.rand(N, generator=g) * 2 - 1)
    per = [dict(A=A, B=_rnd(N, K, gen=g, scale=K ** -0.5).to(dt).to(cuda), bias=_rnd(N, gen=g).to(cuda),
                gamma=(torch.rand(N, generator=g) + 0.5).to(cuda), A_off=i * M * K, C_off=i * M * N) for i in range(G)]
    return A, C0, per, N


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("K", [64, 128])
def test_grouped_ln_producer(cuda, dt, K):
    """proj / fc2 form: C += gamma (A B^T + bias) in fp32, xb = C in 16 bits, part = (mean, M2) per
    128-column chunk of C.  C within test_gemm_grouped_bit_identical_to_single's accumulate
    tolerance of fp64 (and bit-identical to the launch without ln_out); xb bit-exact = the
    round-to-nearest 16-bit value of the C read back; part within 2x dp_layernorm_stats' own error
    against fp64 on the same rows (rows at 300 +- 1 included).
    Measured on MI355X (the four cases; also in profiles/side_ln_fold/README.md): max mean error /
    max |mean| -- dp_layernorm_stats 9.5e-8 .. 1.2e-7, this epilogue 4.7e-8 .. 5.1e-8; max relative
    M2 error -- dp_layernorm_stats 1.28e-7 .. 1.39e-7, this epilogue 1.48e-7 .. 1.74e-7 (the bound is
    twice the dp_layernorm_stats figure of the same run)."""
    A, C0, per, N = _producer_case(cuda, dt, K)
    C = C0.to(cuda)
    Cplain = C0.to(cuda)
    xb = torch.zeros(G * M, N, dtype=dt, device=cuda)
    part = torch.zeros(G * M, N // 128, 2, device=cuda)
    kw = dict(M=M, N=N, K=K, accumulate=True)
    ops.gemm_grouped([dict(d, C=C, ln_out=(xb[i * M:], part[i * M:])) for i, d in enumerate(per)], **kw)
    ops.gemm_grouped([dict(d, C=Cplain) for d in per], **kw)
    torch.cuda.synchronize()
    assert torch.equal(C, Cplain)
    ref = torch.cat([(A.double().cpu()[i * M:(i + 1) * M] @ d["B"].double().cpu().t() + d["bias"].double().cpu())
                     * d["gamma"].double().cpu() for i, d in enumerate(per)]) + C0.double()
    err = (C.double().cpu() - ref).abs().max().item()
    tol = 2e-2 if dt == torch.bfloat16 else 4e-3      # test_gpu_kernels.close, the accumulate case
    print(f"\nproducer {dt} K={K}: max|C - fp64| {err:.3e} (bound {tol * ref.abs().max().item():.3e})")
    assert err <= tol * (ref.abs().max().item() + 1e-6)
    assert torch.equal(xb, C.to(dt))
    ref_part = _chunk_stats64(C)
    # the reference kernel's own error on the same rows
    xb2, part2 = torch.empty_like(xb), torch.empty_like(part)
    ops.layernorm_stats(C, xb2, part2, G * M, N)
    torch.cuda.synchronize()
    assert torch.equal(xb2, xb)
    e_mean, e_m2 = _part_err(part, ref_part)
    s_mean, s_m2 = _part_err(part2, ref_part)
    print(f"producer {dt} K={K}: part mean err {e_mean:.3e} (dp_layernorm_stats {s_mean:.3e}), "
          f"M2 rel err {e_m2:.3e} (dp_layernorm_stats {s_m2:.3e})")
    assert e_mean <= 2 * s_mean and e_m2 <= 2 * s_m2


def _consumer_case(cuda, dt, act, seed=7):
    g = torch.Generator().manual_seed(seed + act)
    K, N = 1024, 256
    x = _rnd(G * M, K, gen=g, scale=2.0) + _rnd(G * M, 1, gen=g)
    x[:, 7] += 40.0                                          # an outlier channel, as DINOv2's
    ws = [dict(w=_rnd(N, K, gen=g, scale=K ** -0.5), b=_rnd(N, gen=g, scale=0.02),
               lw=1.0 + 0.1 * _rnd(K, gen=g), lb=0.02 * _rnd(K, gen=g)) for _ in range(G)]
    return x, ws, K, N


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("act", [0, DP_ACT_GELU])
def test_grouped_ln_consumer(cuda, dt, act):
    """qkv / fc1 form over dp_layernorm_stats' rows and statistics, with ops.fold_layernorm's weights,
    against fp64 LN(x) W^T + b on the unfolded weights: max error <= 1.5 x the error of the existing
    unfolded pair (layernorm_grouped -> gemm_grouped) against the same fp64 on the same inputs.
    Measured on MI355X, rel-L1 folded / unfolded pair: bf16 2.92e-3 / 2.82e-3 (NONE), 3.12e-3 /
    3.08e-3 (GELU); f16 3.67e-4 / 3.52e-4, 3.89e-4 / 3.85e-4 (profiles/side_ln_fold/README.md)."""
    x, ws, K, N = _consumer_case(cuda, dt, act)
    xd = x.to(cuda)
    xb = torch.empty(G * M, K, dtype=dt, device=cuda)
    part = torch.empty(G * M, K // 128, 2, device=cuda)
    ops.layernorm_stats(xd, xb, part, G * M, K)
    out = torch.zeros(G * M, N, dtype=dt, device=cuda)
    groups = []
    for i, w in enumerate(ws):
        wf, bf, sf = ops.fold_layernorm(w["w"].to(cuda), w["b"].to(cuda), w["lw"].to(cuda), w["lb"].to(cuda), dt)
        groups.append(dict(A=xb, B=wf, C=out, bias=bf, A_off=i * M * K, C_off=i * M * N,
                           ln_in=(part[i * M:], sf)))
    ops.gemm_grouped(groups, M=M, N=N, K=K, act=act)
    # the unfolded pair
    h = torch.empty(G * M, K, dtype=dt, device=cuda)
    ops.layernorm_grouped(xd, [w["lw"].to(cuda) for w in ws], [w["lb"].to(cuda) for w in ws], h, M, K)
    out2 = torch.zeros(G * M, N, dtype=dt, device=cuda)
    ops.gemm_grouped([dict(A=h, B=w["w"].to(dt).to(cuda), C=out2, bias=w["b"].to(cuda), A_off=i * M * K,
                           C_off=i * M * N) for i, w in enumerate(ws)], M=M, N=N, K=K, act=act)
    torch.cuda.synchronize()
    ref = torch.cat([F.linear(F.layer_norm(x[i * M:(i + 1) * M].double(), (K,), w["lw"].double(), w["lb"].double(),
                                           1e-6), w["w"].double(), w["b"].double()) for i, w in enumerate(ws)])
    if act == DP_ACT_GELU:
        ref = F.gelu(ref)
    # rel-L1 (test_gemm_8ph320_ln_consumer's measure): both errors are 16-bit rounding noise, whose
    # mean over the 2 x 130 x 256 outputs is stable where the maximum is one sample
    e1 = ((out.double().cpu() - ref).abs().mean() / ref.abs().mean()).item()
    e2 = ((out2.double().cpu() - ref).abs().mean() / ref.abs().mean()).item()
    m1 = (out.double().cpu() - ref).abs().max().item()
    m2 = (out2.double().cpu() - ref).abs().max().item()
    print(f"\nconsumer {dt} act={act}: folded rel-L1 {e1:.3e} (max {m1:.3e}), unfolded pair {e2:.3e} (max {m2:.3e})")
    assert e1 <= 1.5 * e2


@pytest.mark.parametrize("dt", DTYPES)
def test_grouped_ln_chain_repeats_bit_identically(cuda, dt):
    """stats -> qkv consumer -> proj producer -> fc1 consumer -> fc2 producer (attention skipped: proj
    reads the first 1024 qkv columns) run twice from the same input gives the same bits: the
    epilogues keep no counters and no state between launches."""
    g = torch.Generator().manual_seed(21)
    D, H = 1024, 4096
    x0 = _rnd(G * M, D, gen=g)
    W = []
    for _ in range(G):
        w = {}
        for name, n, k in (("qkv", 3 * D, D), ("fc1", H, D)):
            w[name] = ops.fold_layernorm(_rnd(n, k, gen=g, scale=k ** -0.5).to(cuda), _rnd(n, gen=g, scale=0.02).to(cuda),
                                         (1.0 + 0.1 * _rnd(k, gen=g)).to(cuda), (0.02 * _rnd(k, gen=g)).to(cuda), dt)
        for name, n, k in (("proj", D, D), ("fc2", D, H)):
            w[name] = (_rnd(n, k, gen=g, scale=k ** -0.5).to(dt).to(cuda), _rnd(n, gen=g, scale=0.02).to(cuda),
                       (torch.rand(n, generator=g) * 0.5).to(cuda))
        W.append(w)
    h = torch.empty(G * M, D, dtype=dt, device=cuda)
    part = torch.empty(G * M, D // 128, 2, device=cuda)
    qkv = torch.empty(G * M, 3 * D, dtype=dt, device=cuda)
    m = torch.empty(G * M, H, dtype=dt, device=cuda)

    def run():
        x = x0.to(cuda)
        ops.layernorm_stats(x, h, part, G * M, D)

        def cons(name, A, C, n, act):
            ops.gemm_grouped([dict(A=A, B=w[name][0], C=C, bias=w[name][1], A_off=i * M * D, C_off=i * M * n,
                                   ln_in=(part[i * M:], w[name][2])) for i, w in enumerate(W)], M=M, N=n, K=D, act=act)

        def prod(name, A, k, lda):
            ops.gemm_grouped([dict(A=A, B=w[name][0], C=x, bias=w[name][1], gamma=w[name][2], A_off=i * M * lda,
                                   C_off=i * M * D, ln_out=(h[i * M:], part[i * M:])) for i, w in enumerate(W)],
                             M=M, N=D, K=k, lda=lda, accumulate=True)

        cons("qkv", h, qkv, 3 * D, 0)
        prod("proj", qkv, D, 3 * D)
        cons("fc1", h, m, H, DP_ACT_GELU)
        prod("fc2", m, H, H)
        torch.cuda.synchronize()
        return x.clone(), h.clone(), part.clone(), qkv.clone(), m.clone()

    a, b = run(), run()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.isfinite(a[0]).all() and (a[0].cpu() != x0).any()
    assert torch.equal(a[1], a[0].to(dt))


DP_ERR_ARG = 1000     # dp_mi355x.h


def _rc(arr, n, like):
    return _lib.load().dp_gemm_grouped(arr, n, ops._stream(like))


def test_grouped_ln_refusals(cuda):
    """Every ln_* combination outside the two grouped forms is DP_ERR_ARG (nothing is launched)."""
    dt = torch.bfloat16
    N, K = 1024, 1024
    A = torch.zeros(G * M, K, dtype=dt, device=cuda)
    B = torch.zeros(4096, K, dtype=dt, device=cuda)
    C32 = torch.zeros(G * M + 8, N, device=cuda)       # (slack rows: a case that were launched stays inside)
    C16 = torch.zeros(G * M, 4096, dtype=dt, device=cuda)
    xb = torch.zeros(G * M + 8, N, dtype=dt, device=cuda)
    xl = torch.zeros(G * M, N, dtype=torch.int8, device=cuda)
    part = torch.zeros(G * M, 8, 2, device=cuda)
    rs = torch.zeros(G * M + 256, 2, device=cuda)
    cs = torch.zeros(4096, device=cuda)
    ws = ops.gemm_workspace(cuda)

    def build(kind, n=N, k=K, **over):
        arr = (ops.GemmArgs * G)()
        for i in range(G):
            if kind == "prod":
                a = ops._gemm_args(A, B, C32, M=M, N=n, K=k, lda=K, accumulate=True, A_off=i * M * K, C_off=i * M * N,
                                   ldc=N, workspace=ws)
                a.ln_xb_out, a.ln_part_out = xb.data_ptr(), part.data_ptr()
            else:
                a = ops._gemm_args(A, B, C16, M=M, N=n, K=k, lda=K, A_off=i * M * K, C_off=i * M * 4096, ldc=4096,
                                   workspace=ws)
                a.ln_part_in, a.ln_colsum, a.ln_eps = part.data_ptr(), cs.data_ptr(), 1e-6
            for f, v in over.items():
                if f.startswith("g1_"):
                    if i == 1:
                        setattr(a, f[3:], v)
                else:
                    setattr(a, f, v)
            arr[i] = a
        return arr

    cases = {
        "producer + ln_xl": build("prod", ln_xl=xl.data_ptr()),
        "producer + ln_rs_out": build("prod", ln_rs_out=rs.data_ptr(), ln_eps=1e-6),
        "producer without xb": build("prod", ln_xb_out=None),
        "producer without part": build("prod", ln_part_out=None),
        "producer N % 128": build("prod", n=1088),
        "producer with GELU": build("prod", act=DP_ACT_GELU),
        "producer and consumer": build("prod", ln_part_in=part.data_ptr(), ln_colsum=cs.data_ptr(), ln_eps=1e-6),
        "groups disagree (producer)": build("prod", g1_ln_part_out=None, g1_ln_xb_out=None),
        "consumer K != 1024": build("cons", k=512),
        "consumer + ln_rs_in": build("cons", ln_rs_in=rs.data_ptr()),
        "consumer ln_rs_in only": build("cons", ln_part_in=None, ln_rs_in=rs.data_ptr()),
        "consumer without colsum": build("cons", ln_colsum=None),
        "consumer with gamma": build("cons", gamma=cs.data_ptr()),
        "consumer eps 0": build("cons", ln_eps=0.0),
        "groups disagree (consumer)": build("cons", g1_ln_part_in=None, g1_ln_colsum=None),
    }
    for what, arr in cases.items():
        assert _rc(arr, G, A) == DP_ERR_ARG, what
    # and the two forms themselves are taken
    assert _rc(build("prod"), G, A) == 0
    assert _rc(build("cons"), G, A) == 0
    torch.cuda.synchronize()
