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
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ml-depth-pro-video_amd")

# What a child process does under its own DP_ABLATE (read at import): pack two Blocks of the patch and the
# image encoder, print each set's LayerNorm path (engine.vit_ln_mode) and key names, and -- given the key
# names of sets packed under another DP_ABLATE as argv[1] -- what vit_ln_mode says of those.
CHILD = """
import json, sys, torch
sys.path.insert(0, %r)
from depth_pro import engine
from depth_pro.spec import vit_spec
from depth_pro.weights import synthetic_tensor
foreign = json.loads(sys.argv[1]) if len(sys.argv) > 1 else {}
out = {}
for vit in ("encoder.patch_encoder.", "encoder.image_encoder."):
    keep = tuple(f"{vit}blocks.{i}." for i in (0, 1))
    sd = {k: synthetic_tensor(k, s) for k, s in vit_spec(vit).items() if "blocks." not in k or k.startswith(keep)}
    P = engine.pack_vit(sd, vit, torch.device("cpu"), torch.bfloat16, blocks=(0, 1))
    out[vit] = {"mode": engine.vit_ln_mode(P, vit), "keys": sorted(P)}
    if vit in foreign:
        try:
            out[vit]["foreign"] = engine.vit_ln_mode(dict.fromkeys(foreign[vit]), vit)
        except engine.DPError as e:
            out[vit]["foreign"] = "DPError: " + str(e)
print(json.dumps(out))
""" % PKG


def _packed_modes(ablate, foreign=None):
    import json
    import subprocess

    env = dict(os.environ, DP_ABLATE=ablate)
    argv = [sys.executable, "-c", CHILD] + ([json.dumps({v: d["keys"] for v, d in foreign.items()})] if foreign else [])
    p = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr
    return json.loads(p.stdout.splitlines()[-1])


def test_vit_ln_mode_of_packed_sets():
    """engine.vit_ln_mode: split / folded / unfolded for sets that pack_vit made under the matching
    DP_ABLATE, DPError where the set and the environment disagree (patch and side prefix)."""
    patch, image = "encoder.patch_encoder.", "encoder.image_encoder."
    plain = _packed_modes("")
    assert (plain[patch]["mode"], plain[image]["mode"]) == ("split", "folded")
    for ablate in ("ln", "vitgemm"):        # both unfolded; the default's folded sets are refused
        got = _packed_modes(ablate, plain)
        assert (got[patch]["mode"], got[image]["mode"]) == ("unfolded", "unfolded")
        assert got[patch]["foreign"].startswith("DPError") and got[image]["foreign"].startswith("DPError")
    unfolded = got
    got = _packed_modes("sideln", plain)    # the side encoders alone unfolded
    assert (got[patch]["mode"], got[image]["mode"]) == ("split", "unfolded")
    assert got[patch]["foreign"] == "split" and got[image]["foreign"].startswith("DPError")
    got = _packed_modes("", unfolded)       # and unfolded sets where the folded paths run
    assert got[patch]["foreign"].startswith("DPError") and got[image]["foreign"].startswith("DPError")
    assert "other LayerNorm path" in got[patch]["foreign"]


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
