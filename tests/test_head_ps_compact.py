"""The composed depth head's compact form: each output parity q = 2 dy + dx of the composed 3x3
conv (engine.compose_head) has non-zero weights only at the 2 x 2 taps (dy + j // 2, dx + j % 2),
so dp_gemm takes B = [q][o][j][ci] with K = 4 in_c (DP_STORE_HEAD_PS on the patch-conv engine) and
walks 4 taps per channel block instead of 9.

CPU: the zero structure and the packing.  GPU: bit identity with the dense patch-conv walk, the
layer-order tolerance of test_gpu_kernels.py's head tests, and the planner.
"""

import pytest
import torch
import torch.nn.functional as F

from depth_pro import ops
from depth_pro._lib import DP_TILE_BIG_512x128, DP_TILE_CV3_256x256, DP_TILE_CV3_384x128, DPError
from depth_pro.engine import compact_head_w, compose_head

CI, O = 128, 32


def _layers(seed):
    g = torch.Generator().manual_seed(seed)
    wd = torch.randn(CI, CI, 2, 2, generator=g) * CI ** -0.5
    bd = torch.randn(CI, generator=g)
    w2 = torch.randn(O, CI, 3, 3, generator=g) * (9 * CI) ** -0.5
    b2 = torch.randn(O, generator=g)
    w4 = torch.randn(O, generator=g) * O ** -0.5
    return g, wd, bd, w2, b2, w4


def _dense_wc(P):
    """head.ps.w (ops.conv_weight: [(q, o)][ci / 64][ty][tx][64]) back as W'[q, o, ty, tx, ci]."""
    return P["head.ps.w"].reshape(4, O, CI // 64, 3, 3, 64).permute(0, 1, 3, 4, 2, 5).reshape(4, O, 3, 3, CI)


def _taps(q):
    dy, dx = q >> 1, q & 1
    return [(dy + j // 2, dx + j % 2) for j in range(4)]


def test_compact_weights_zero_structure_and_packing():
    _, wd, bd, w2, b2, _ = _layers(5)
    P = compose_head(wd, bd, w2, b2, torch.float32)
    wc = _dense_wc(P)
    w4 = P["head.ps.w4"]
    assert w4.shape == (4 * O, 4 * CI)
    w4 = w4.reshape(4, O, 4, CI)
    back = torch.zeros_like(wc)
    for q in range(4):
        keep = _taps(q)
        assert keep == sorted(keep)                                  # ascending (ty, tx): the dense walk's order
        for ty in range(3):
            for tx in range(3):
                if (ty, tx) not in keep:
                    assert (wc[q, :, ty, tx] == 0.0).all(), (q, ty, tx)
        for j, (ty, tx) in enumerate(keep):
            assert wc[q, :, ty, tx].abs().max() > 0
            back[q, :, ty, tx] = w4[q, :, j]
    assert torch.equal(back, wc)                                     # compact -> dense, bit for bit
    # the 16-bit packings round the same fp32 values
    for dt in (torch.float16, torch.bfloat16):
        Pd = compose_head(wd, bd, w2, b2, dt)
        wcd, w4d = _dense_wc(Pd), Pd["head.ps.w4"].reshape(4, O, 4, CI)
        for q in range(4):
            for j, (ty, tx) in enumerate(_taps(q)):
                assert torch.equal(wcd[q, :, ty, tx], w4d[q, :, j])
    # a weight on a dropped tap must not be lost silently
    bad = wc.clone()
    bad[1, 7, 2, 0, 3] = 1e-30                                      # parity 1 = (dy 0, dx 1) never reads tap (2, 0)
    with pytest.raises(AssertionError):
        compact_head_w(bad, torch.float32)
    compact_head_w(wc, torch.float32)                               # the composed weights pass


def _problem(cuda, dt, S, seed):
    g, wd, bd, w2, b2, w4 = _layers(seed)
    h0 = torch.randn(1, CI, S, S, generator=g).to(dt).float()
    P = {k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in compose_head(wd, bd, w2, b2, dt).items()}
    x = h0[0].permute(1, 2, 0).reshape(S * S, CI).contiguous().to(dt).to(cuda)
    kw = dict(M=S * S, N=128, conv=dict(in_h=S, in_w=S, in_c=CI, k=3, stride=1, pad=1, out_h=S, out_w=S),
              bias=P["head.ps.b"], head_w=w4.to(cuda), head_b=0.25, head_corr=P["head.ps.corr"])
    ref = F.conv_transpose2d(h0, wd, bd, stride=2)
    ref = F.relu(F.conv2d(F.relu(F.conv2d(ref, w2, b2, padding=1)), w4.reshape(1, O, 1, 1), torch.tensor([0.25])))
    return x, P, kw, ref[0, 0]


def _close(out, ref, dt, what):
    """test_gpu_kernels.close with its tolerances (2e-2 bf16, 4e-3 f16, of the reference's max)."""
    out, ref = out.float().cpu(), ref.float().cpu()
    err = (out - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    print(f"{what}: max|d| = {err:.3e}, scale {scale:.3e}")
    assert err <= (2e-2 if dt == torch.bfloat16 else 4e-3) * scale, f"{what}: max|d|={err:.3e} vs scale {scale:.3e}"


# S = 16: one 16-row tile whose four edges are image borders (head_corr on every side and corner);
# S = 48: 3 x 3 tiles of 16 rows (one interior tile) and 2 x 3 tiles of 24 rows
@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("S,tile", [(16, DP_TILE_CV3_256x256), (48, DP_TILE_CV3_256x256), (48, DP_TILE_CV3_384x128)])
def test_compact_head_bit_identical_to_dense_patch_conv(cuda, dt, S, tile):
    x, P, kw, ref = _problem(cuda, dt, S, 100 + S)
    dense = torch.full((2 * S, 2 * S), float("nan"), device=cuda)
    comp = dense.clone()
    ops.gemm(x, P["head.ps.w"], dense, K=9 * CI, tile=tile, **kw)
    ops.gemm(x, P["head.ps.w4"], comp, K=4 * CI, tile=tile, **kw)
    torch.cuda.synchronize()
    assert not torch.isnan(comp).any()
    assert torch.equal(comp, dense), (comp - dense).abs().max().item()
    _close(comp, ref, dt, f"compact HEAD_PS S={S} tile={tile}")


@pytest.mark.gpu
def test_compact_head_planner(cuda):
    dt = torch.float16
    A = torch.zeros(8, dtype=dt, device=cuda)
    out = torch.zeros(8, device=cuda)

    def plan(S, tile=0, K=4 * CI):
        return ops.gemm(A, A, out, M=S * S, N=128, K=K, tile=tile, plan_only=True, bias=out, head_w=out, head_b=0.0,
                        head_corr=out, conv=dict(in_h=S, in_w=S, in_c=CI, k=3, stride=1, pad=1, out_h=S, out_w=S))

    assert plan(768)[0] == DP_TILE_CV3_384x128                       # the product shape: 24-row tiles
    assert plan(768, K=9 * CI)[0] == DP_TILE_BIG_512x128             # dense stays where it was
    assert plan(16)[0] == DP_TILE_CV3_256x256
    assert plan(48, tile=DP_TILE_CV3_256x256)[0] == DP_TILE_CV3_256x256
    for S, tile in ((40, 0), (24, 0), (32, DP_TILE_CV3_384x128), (768, DP_TILE_BIG_512x128)):
        with pytest.raises(DPError) as e:                            # no engine for compact weights: an error
            plan(S, tile)
        assert "DP_ERR_ARG" in str(e.value), e.value
    # ... and the launch itself refuses the same way (nothing runs)
    x, P, kw, _ = _problem(cuda, dt, 40, 7)
    o40 = torch.zeros(80, 80, device=cuda)
    with pytest.raises(DPError):
        ops.gemm(x, P["head.ps.w4"], o40, K=4 * CI, **kw)
