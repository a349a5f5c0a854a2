"""The 3x3 patch-conv engine's K-loop schedule at the shapes where its LDS-DMA wait accounting can go
wrong: the next channel block's patch is streamed one piece per K step over the block's first taps,
so the counted waits differ between the steps that carry a patch piece, the steps that do not, the
last block (no next patch) and the loop's tail (no weight step t + 2).

Every case is bit-identical to the row-raster engine on the same operands (256 x 256 big engine; the
512 x 128 one for the border-corrected 128-channel conv) and close to F.conv2d in fp32, with the
tolerance of the existing patch-conv test.  A wrong wait shows as stale or half-written LDS data,
i.e. as wrong numbers.

in_c = 64: one channel block, no patch hand-over, 9 K steps (odd); 128: exactly one hand-over, even
step count; 192: an odd block count (the unpaired tail block).  S = 16: a single 16 x 16 tile, every
pixel on the border (all halo pieces zero-filled).  S = 48: 12-row tiles (4 patch pieces per wave)
and 24-row tiles (8 pieces: the hand-over reaches tap 7; N = 128 with the border correction, which
has no ReLU prologue and no residuals).  S = 32 with 2 images: tiles of a second image.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from depth_pro import ops  # noqa: E402
from depth_pro._lib import (DP_ACT_RELU, DP_TILE_BIG_256x256, DP_TILE_BIG_512x128,  # noqa: E402
                            DP_TILE_CV3_192x256, DP_TILE_CV3_256x256, DP_TILE_CV3_384x128)
from test_gpu_kernels import close, rnd  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16]
# name: (side, images, tile rows)
MAPS = {"s16_one_tile": (16, 1, 16), "s48_th12": (48, 1, 12), "s48_th24": (48, 1, 24), "s32_two_images": (32, 2, 16)}


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("variant", ["relu_bias_relu", "bias_r1_r2"])
@pytest.mark.parametrize("cin", [64, 128, 192])
@pytest.mark.parametrize("shape", list(MAPS))
def test_cv3_schedule_bit_identical(cuda, dt, variant, cin, shape):
    S, nb, th = MAPS[shape]
    g = torch.Generator().manual_seed(1000 * S + 10 * cin + nb + len(variant))
    head = th == 24
    Co = 128 if head else 256
    x = rnd(nb, cin, S, S, dt=dt, dev=cuda, gen=g)
    w = rnd(Co, cin, 3, 3, dt=dt, dev=cuda, gen=g, scale=(9 * cin) ** -0.5)
    b = torch.randn(Co, generator=g).to(cuda)
    xh = x.permute(0, 2, 3, 1).reshape(nb * S * S, cin).contiguous()
    M = nb * S * S
    kw = dict(M=M, N=Co, K=9 * cin, conv=dict(in_h=S, in_w=S, in_c=cin, k=3, stride=1, pad=1, out_h=S, out_w=S), bias=b)
    ref = F.conv2d(x.float(), w.float(), b, padding=1)
    if head:
        # border-corrected conv: minus corr[tap] for every tap that falls into the zero padding;
        # variants: plain / with the ReLU epilogue
        corr = (torch.randn(9 * Co, generator=g) * 0.1).to(cuda)
        kw.update(border_corr=corr)
        pad = F.pad(torch.zeros(1, 1, S, S, device=cuda), (1, 1, 1, 1), value=1.0)
        ref = ref - F.conv2d(pad, corr.reshape(9, Co).t().reshape(Co, 1, 3, 3))
        if variant == "relu_bias_relu":
            kw.update(act=DP_ACT_RELU)
            ref = F.relu(ref)
        tile, raster = DP_TILE_CV3_384x128, DP_TILE_BIG_512x128
    else:
        if variant == "relu_bias_relu":
            kw.update(relu_a=True, act=DP_ACT_RELU)
            ref = F.relu(F.conv2d(F.relu(x.float()), w.float(), b, padding=1))
        else:
            r1 = rnd(M, Co, dt=dt, dev=cuda, gen=g)
            r2 = rnd(M, Co, dt=dt, dev=cuda, gen=g)
            kw.update(R1=r1, ldr1=Co, R2=r2, ldr2=Co)
            ref = ref + (r1.float() + r2.float()).reshape(nb, S, S, Co).permute(0, 3, 1, 2)
        tile, raster = (DP_TILE_CV3_256x256 if th == 16 else DP_TILE_CV3_192x256), DP_TILE_BIG_256x256
    out1 = torch.full((M, Co), 7.0, dtype=dt, device=cuda)
    out2 = out1.clone()
    wp = ops.conv_weight(w)
    ops.gemm(xh, wp, out1, tile=tile, **kw)
    ops.gemm(xh, wp, out2, tile=raster, **kw)
    torch.cuda.synchronize()
    assert torch.equal(out1, out2), (out1.float() - out2.float()).abs().max().item()
    close(out1.reshape(nb, S, S, Co).permute(0, 3, 1, 2), ref, dt, f"cv3 {shape} cin {cin} {variant}")


def test_cv3_head_planner_past_patch_dma_range(cuda):
    """The N = 128 border-corrected 768^2 conv: one map plans the 24-row patch-conv tiles; 8 stacked maps
    (M * in_c >= 2^30: the input map is past the patch DMA's 2-GiB buffer range) plan the 512 x 128
    engine instead of failing.  plan_only: no operand memory is touched."""
    A = torch.empty(8, dtype=torch.float16, device=cuda)
    corr = torch.zeros(9 * 128, device=cuda)
    S = 768
    conv = dict(in_h=S, in_w=S, in_c=256, k=3, stride=1, pad=1, out_h=S, out_w=S)
    for maps, want in ((1, DP_TILE_CV3_384x128), (8, DP_TILE_BIG_512x128)):
        assert (maps * S * S * 256 >= 1 << 30) == (maps == 8)
        tile, _ = ops.gemm(A, A, A, M=maps * S * S, N=128, K=2304, conv=conv, border_corr=corr, plan_only=True)
        assert tile == want, (maps, tile)
