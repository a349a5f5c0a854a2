"""The image / FOV encoders' packed folded weights (engine.pack_vit -> attn.qkv.fold.*, mlp.fc1.fold.*;
CPU): rstd * (x B^T - mean * S) + b' reproduces fp64 LayerNorm -> Linear on the seed-0 weights, to the
bound of test_ln_fold.test_fold_is_exact_algebra_in_fp64.  B is the packed 16-bit matrix, so the
reference multiplies LN(x)'s normalised part by the weights that B holds (B / (ln.weight o scale),
exact in fp64) -- the rounding of B is the GEMM's operand rounding, not the fold's; that B is the
nearest 16-bit value of the exact fold is asserted beside it."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ml-depth-pro-video_amd"))
from depth_pro import engine, ops  # noqa: E402
from depth_pro.spec import EMBED_DIM, HEADS, vit_spec  # noqa: E402
from depth_pro.weights import synthetic_tensor  # noqa: E402

BLOCKS = (0, 23)


@pytest.mark.parametrize("vit", ["encoder.image_encoder.", "fov.encoder.0."])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_packed_side_fold_reproduces_ln_linear(vit, dt):
    keep = tuple(f"{vit}blocks.{i}." for i in BLOCKS)
    sd = {k: synthetic_tensor(k, s) for k, s in vit_spec(vit).items() if "blocks." not in k or k.startswith(keep)}
    P = engine.pack_vit(sd, vit, torch.device("cpu"), dt, blocks=BLOCKS)
    assert engine.side_ln_fold_enabled()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(19, EMBED_DIM, generator=g, dtype=torch.float64) * 3 + 0.5
    mean = x.mean(1, keepdim=True)
    rstd = (x.var(1, unbiased=False, keepdim=True) + 1e-6).rsqrt()
    qg = ops.log2q_gamma(HEADS, EMBED_DIM // HEADS, "cpu").double()
    for i in BLOCKS:
        b = f"{vit}blocks.{i}."
        # one weight set per LayerNorm path: no plain qkv / fc1, no norm1 / norm2
        assert not any(b + n in P for n in ("attn.qkv.weight", "mlp.fc1.weight", "norm1.weight", "norm1.bias",
                                            "norm2.weight", "norm2.bias"))
        assert b + "attn.proj.weight" in P and b + "mlp.fc2.weight" in P
        for lin, ln, s in (("attn.qkv", "norm1", qg), ("mlp.fc1", "norm2", None)):
            w, bias = sd[b + lin + ".weight"].double(), sd[b + lin + ".bias"].double()
            lw, lb = sd[b + ln + ".weight"].double(), sd[b + ln + ".bias"].double()
            s = torch.ones(w.shape[0], dtype=torch.float64) if s is None else s
            B, bf, S = P[b + lin + ".fold.w"], P[b + lin + ".fold.b"], P[b + lin + ".fold.s"]
            assert B.dtype == dt and bf.dtype == torch.float32 and S.dtype == torch.float32
            assert torch.equal(B, (w * lw[None, :] * s[:, None]).to(dt))
            wr = B.double() / (lw[None, :] * s[:, None])          # the weights B holds
            ref = ((x - mean) * rstd * lw) @ wr.t() * s + (lb @ w.t() + bias) * s
            out = rstd * (x @ B.double().t() - mean * S.double()) + bf.double()
            assert torch.allclose(out, ref, rtol=1e-5, atol=1e-5), (lin, (out - ref).abs().max().item())
