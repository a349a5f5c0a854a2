"""The C-ABI library loads and exports exactly what include/dp_mi355x.h declares (no GPU needed)."""

import ctypes
import os
import re
import subprocess

import pytest

from depth_pro import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "dp_mi355x.h")


def declared():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"^(?:int|int64_t) (dp_\w+)\(", src, flags=re.M)))


def test_header_and_python_export_lists_agree():
    assert declared() == sorted(_lib.EXPORTS)


def test_library_loads_and_exports_every_symbol():
    lib = _lib.load()
    for name in declared():
        assert hasattr(lib, name), name
    assert lib.dp_abi_version() == _lib.DP_ABI_VERSION


def test_gemm_args_struct_layout_matches_c(tmp_path):
    """ctypes GemmArgs == sizeof/offsetof of the C struct (compiled with gcc)."""
    fields = [f for f, _ in _lib.GemmArgs._fields_]
    prog = tmp_path / "lay.c"
    body = "".join(f'printf("%zu\\n", offsetof(dp_gemm_args, {f}));' for f in fields)
    prog.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\n'
                    f'int main(void){{printf("%zu\\n", sizeof(dp_gemm_args));{body}return 0;}}\n')
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-std=c11", str(prog), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == ctypes.sizeof(_lib.GemmArgs)
    for f, off in zip(fields, vals[1:]):
        assert getattr(_lib.GemmArgs, f).offset == off, f


def test_argument_errors_are_reported_before_launch():
    """Shape/alignment errors return DP_ERR_* without touching the GPU (null stream, no device)."""
    lib = _lib.load()
    a = _lib.GemmArgs()
    a.M, a.N, a.K = 16, 16, 60  # K % 64 != 0
    a.A = a.B = a.C = 16
    a.lda = a.ldb = 64
    assert lib.dp_gemm(ctypes.byref(a), None) == 1001
    a.K = 64
    a.ldb = 12
    assert lib.dp_gemm(ctypes.byref(a), None) == 1002
    assert lib.dp_attention(16, 16, 1, 577, 16, 128, 0.1, 0, None) == 1001
    with pytest.raises(_lib.DPError, match="DP_ERR_SHAPE"):
        _lib.check(1001, "x")


def test_gemm_plan_tile_choice():
    """dp_gemm_plan (host-only): engine choice for the frame's GEMM shapes (tile, workgroups)."""
    lib = _lib.load()
    t, g = ctypes.c_int32(), ctypes.c_int32()

    def plan(M, N, K, **kw):
        a = _lib.GemmArgs()
        a.M, a.N, a.K = M, N, K
        a.A = a.B = a.C = 256
        a.lda, a.ldb, a.ldc = K, K, N
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.dp_gemm_plan(ctypes.byref(a), ctypes.byref(t), ctypes.byref(g))
        return rc, t.value, g.value

    # ViT-L patch encoder (M = 35 x 577 = 20195 = 64 tiles of 320 rows)
    # qkv / proj: the 8-phase 320 x 256 engine; fc1: the persistent 8-phase engine (one workgroup per CU)
    assert plan(20195, 3072, 1024)[1:] == (_lib.DP_TILE_8PH_320x256, 64 * 12)
    assert plan(20195, 1024, 1024)[1:] == (_lib.DP_TILE_8PH_320x256, 64 * 4)     # one round on 256 CUs
    assert plan(20195, 4096, 1024)[1:] == (_lib.DP_TILE_P8PH_256x256, 256)
    # the previous engines stay reachable (A/B switches in the planner, explicit tile hints)
    assert plan(20195, 4096, 1024, tile=_lib.DP_TILE_8PH_256x256)[1:] == (_lib.DP_TILE_8PH_256x256, 79 * 16)
    assert plan(20195, 1024, 1024, tile=_lib.DP_TILE_BIG_320x256)[1:] == (_lib.DP_TILE_BIG_320x256, 64 * 4)
    assert plan(577, 3072, 1024)[1:] == (_lib.DP_TILE_BIG_256x128, 3 * 24)       # side encoders
    assert plan(768 * 768, 128, 2304)[1:] == (_lib.DP_TILE_BIG_512x128, 1152)     # head.0 conv (N = 128)
    # past 2^31 elements of A (M * lda) or B (N * ldb): only the engines with 64-bit operand
    # pointers (the 8-phase 320 x 256 and the persistent engines keep 32-bit element offsets)
    big_m = (1 << 21) + 5                                   # 2097157 x 1024 >= 2^31
    assert plan(big_m, 1024, 1024)[1:] == (_lib.DP_TILE_BIG_320x256, 6554 * 4)
    off32 = {_lib.DP_TILE_8PH_320x256, _lib.DP_TILE_P8PH_256x256, _lib.DP_TILE_PBIG_320x256,
             _lib.DP_TILE_PBIG_256x256}
    assert plan(big_m, 4096, 1024)[1] not in off32
    assert plan(big_m, 1024, 1024, tile=_lib.DP_TILE_8PH_320x256)[0] == 1000
    assert plan(big_m, 4096, 1024, tile=_lib.DP_TILE_P8PH_256x256)[0] == 1000
    assert plan(big_m - 8, 1024, 1024)[1] in off32                      # 2097149 x 1024 < 2^31
    # stream-K is opt-in and needs a workspace
    assert plan(20195, 3072, 1024, tile=_lib.DP_TILE_STREAMK_256x256)[0] == 1000
    ws = lib.dp_gemm_workspace_size()
    rc, tile, wgs = plan(20195, 3072, 1024, tile=_lib.DP_TILE_STREAMK_256x256, workspace=256, workspace_bytes=ws)
    assert rc == 0 and tile == _lib.DP_TILE_STREAMK_256x256 and 1 <= wgs <= 256

    # decoder 3x3 convs: long-K projections with < 1 tile per CU go to stream-K with
    # split K ranges (needs a workspace); K = 2304 small grids stay data-parallel
    def conv(S, cin, **kw):
        return plan(S * S, 256, 9 * cin, a_mode=_lib.DP_A_CONV, in_h=S, in_w=S, in_c=cin, k_h=3, k_w=3,
                    stride=1, pad=1, out_h=S, out_w=S, **kw)
    wsk = dict(workspace=256, workspace_bytes=ws)
    assert conv(48, 1024, **wsk)[1:] == (_lib.DP_TILE_STREAMK_256x256, 9 * 6)     # 9 tiles x split 6
    assert conv(96, 1024, **wsk)[1:] == (_lib.DP_TILE_STREAMK_256x256, 36 * 6)    # 36 tiles x split 6
    # 192^2 x 512 channels: 144 tiles of 16 x 16 px would leave 112 CUs idle -- 12-row patch-conv tiles
    # (192 workgroups, one round; the planner rule of DP_TILE_CV3_192x256)
    assert conv(192, 512, **wsk)[1:] == (_lib.DP_TILE_CV3_192x256, 192)
    assert conv(48, 1024)[1] != _lib.DP_TILE_STREAMK_256x256                        # no workspace
    assert conv(48, 256, **wsk)[1] == _lib.DP_TILE_BIG_256x128                     # K = 2304
    # split-K + reduce: an explicit hint (needs a workspace); split = min(CUs / tiles, K steps / 2,
    # workspace slabs, 32)
    SPK = _lib.DP_TILE_SPLITK_256x256
    assert conv(48, 1024, tile=SPK, **wsk)[1:] == (SPK, 9 * 28)
    assert conv(96, 1024, tile=SPK, **wsk)[1:] == (SPK, 36 * 7)                      # 7 slabs of 9.4 MB
    assert conv(48, 256, tile=SPK, **wsk)[1:] == (SPK, 9 * 18)                       # 36 K steps / 2
    assert conv(48, 256, tile=SPK)[0] == 1000                                        # no workspace
    assert conv(768, 256, tile=SPK, **wsk)[0] == 1001                                # 2304 tiles: no split
    # the 768^2 ResidualBlock convs (2304 tiles of 256 pixels): the 3x3 patch-conv engine; 384^2 not
    assert conv(768, 256, **wsk)[1:] == (_lib.DP_TILE_CV3_256x256, 2304)
    assert conv(384, 256, **wsk)[1] != _lib.DP_TILE_CV3_256x256
    # the head convs at 768^2 (128 output channels): the composed out_conv∘head.0 with its border
    # correction on the patch-conv engine (debug 4096: the 512 x 128 engine); the composed depth
    # head (HEAD_PS) on the 512 x 128 engine unless the patch-conv engine is asked for
    def head(**kw):
        return plan(768 * 768, 128, 9 * kw.pop("cin"), a_mode=_lib.DP_A_CONV, in_h=768, in_w=768, k_h=3, k_w=3,
                    stride=1, pad=1, out_h=768, out_w=768, head_corr=256, **kw)
    h0c = dict(cin=256, in_c=256)
    hps = dict(cin=128, in_c=128, store_mode=_lib.DP_STORE_HEAD_PS, head_w=256, c_dtype=_lib.DP_F32)
    assert head(**h0c)[1:] == (_lib.DP_TILE_CV3_384x128, 1536)                       # 24 x 16-pixel tiles
    assert head(**h0c, tile=_lib.DP_TILE_CV3_256x256)[1:] == (_lib.DP_TILE_CV3_256x256, 2304)
    assert head(**hps)[1:] == (_lib.DP_TILE_BIG_512x128, 1152)
    assert head(**hps, tile=_lib.DP_TILE_CV3_256x256)[1:] == (_lib.DP_TILE_CV3_256x256, 2304)
    assert head(**hps, tile=_lib.DP_TILE_CV3_384x128)[1:] == (_lib.DP_TILE_CV3_384x128, 1536)
    assert head(**hps, tile=_lib.DP_TILE_BIG_256x128)[1:] == (_lib.DP_TILE_BIG_256x128, 2304)
    assert head(**hps, tile=_lib.DP_TILE_BIG_256x256)[1:] == (_lib.DP_TILE_BIG_512x128, 1152)    # not a HEAD_PS engine
    # the decoder's 2x2 deconvs with >= 128 tiles of 256 x 256: the persistent 8-phase engine with
    # the pixel-shuffle store; fewer tiles stay where they were
    def deconv(S, cin, cout, **kw):
        return plan(S * S, 4 * cout, cin, store_mode=_lib.DP_STORE_DECONV2X2, dc_h=S, dc_w=S, dc_cout=cout,
                    ldc=cout, dtype=_lib.DP_F16, c_dtype=_lib.DP_F16, bias=256, **kw)
    assert deconv(384, 256, 256, **wsk)[1:] == (_lib.DP_TILE_P8PH_256x256, 256)
    assert deconv(192, 256, 256, **wsk)[1:] == (_lib.DP_TILE_P8PH_256x256, 256)
    assert deconv(96, 512, 512, **wsk)[1:] == (_lib.DP_TILE_P8PH_256x256, 256)     # 288 tiles
    assert deconv(96, 256, 256, **wsk)[1:] == (_lib.DP_TILE_P8PH_256x256, 144)     # 144 tiles, one round
    assert deconv(48, 256, 256, **wsk)[1] != _lib.DP_TILE_P8PH_256x256             # 36 tiles
    assert deconv(384, 256, 256, act=_lib.DP_ACT_RELU, **wsk)[1] != _lib.DP_TILE_P8PH_256x256
    lib.dp_gemm_debug_flags(4096)
    try:
        assert head(**h0c)[1:] == (_lib.DP_TILE_BIG_512x128, 1152)
        assert head(**hps)[1:] == (_lib.DP_TILE_BIG_512x128, 1152)
    finally:
        lib.dp_gemm_debug_flags(0)
    lib.dp_gemm_debug_flags(1 << 23)
    try:
        assert deconv(384, 256, 256, **wsk)[1] == _lib.DP_TILE_STREAMK_256x256
    finally:
        lib.dp_gemm_debug_flags(0)


def test_gemm_epilogue_alignment_and_column_chunk_rules():
    """dp_mi355x.h, 'Alignment of the epilogue operands' (host only, null stream, no launch): ldc / ldr1 /
    ldr2 / ldpos % 4 on every engine; N % 8, dc_cout % 8 (DP_ERR_SHAPE) and ldr1 / ldr2 / 16-bit ldc % 8
    (DP_ERR_ALIGN) for a hint from DP_TILE_BIG_256x256 up, while DP_TILE_AUTO takes the 4-column
    128 x 128 engine instead of failing."""
    lib = _lib.load()
    t, g = ctypes.c_int32(), ctypes.c_int32()
    SHAPE, ALIGN = 1001, 1002
    BIG = (_lib.DP_TILE_BIG_256x256, _lib.DP_TILE_BIG_256x128, _lib.DP_TILE_8PH_256x256, _lib.DP_TILE_BIG_320x256,
           _lib.DP_TILE_BIG_512x128, _lib.DP_TILE_DUAL_256x128, _lib.DP_TILE_DEEP_256x128)

    def args(M=300, N=136, K=128, **kw):
        a = _lib.GemmArgs()
        a.M, a.N, a.K = M, N, K
        a.A = a.B = a.C = 256
        a.lda, a.ldb, a.ldc = K, K, N
        a.dtype = a.c_dtype = _lib.DP_BF16
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def plan(**kw):
        rc = lib.dp_gemm_plan(ctypes.byref(args(**kw)), ctypes.byref(t), ctypes.byref(g))
        return rc, t.value

    # % 4 on every engine, for the operands in use only; dp_gemm itself reports the same before any launch
    for tile in (0, _lib.DP_TILE_128x128, _lib.DP_TILE_256x64, _lib.DP_TILE_BIG_256x128):
        assert plan(tile=tile)[0] == 0
        assert plan(tile=tile, ldc=138)[0] == ALIGN
        assert plan(tile=tile, R1=256, ldr1=138)[0] == ALIGN
        assert plan(tile=tile, R2=256, ldr2=142)[0] == ALIGN
        assert plan(tile=tile, pos=256, pos_group=7, ldpos=138)[0] == ALIGN
        assert plan(tile=tile, ldr1=138, ldr2=3, ldpos=1)[0] == 0            # no R1 / R2 / pos: not looked at
        assert lib.dp_gemm(ctypes.byref(args(tile=tile, ldc=138)), None) == ALIGN
    assert plan(N=32, head_w=256, c_dtype=_lib.DP_F32, ldc=1)[0] == 0       # the fused head's C is a vector
    # % 8 for the 8-column engines: 16-bit C, R1, R2 (an fp32 C and pos keep % 4)
    for tile in BIG:
        assert plan(tile=tile)[:2] == (0, tile)
        assert plan(tile=tile, ldc=140)[0] == ALIGN
        assert plan(tile=tile, ldc=140, c_dtype=_lib.DP_F32)[0] == 0
        assert plan(tile=tile, R1=256, ldr1=140)[0] == ALIGN
        assert plan(tile=tile, R2=256, ldr2=140)[0] == ALIGN
        assert plan(tile=tile, R1=256, ldr1=144, R2=256, ldr2=152, pos=256, pos_group=7, ldpos=140, ldc=144)[0] == 0
        assert plan(tile=tile, N=132, ldc=136)[0] == SHAPE                  # N % 8
    # ... which DP_TILE_AUTO serves on the 4-column engine
    assert plan()[1] == _lib.DP_TILE_BIG_256x128
    for kw in (dict(ldc=140), dict(R1=256, ldr1=140), dict(R2=256, ldr2=140), dict(N=132)):
        assert plan(**kw) == (0, _lib.DP_TILE_128x128), kw
    assert plan(ldc=140, c_dtype=_lib.DP_F32)[1] == _lib.DP_TILE_BIG_256x128

    # the 2x2 deconv store: one sub-pixel per column chunk -- dc_cout % 4 always, % 8 on the 8-column engines
    def deconv(cout, S=16, **kw):
        kw.setdefault("ldc", cout)
        kw.setdefault("K", 64)
        return plan(M=S * S, N=4 * cout, store_mode=_lib.DP_STORE_DECONV2X2, dc_h=S, dc_w=S, dc_cout=cout, **kw)
    assert deconv(18, ldc=24)[0] == SHAPE
    assert deconv(20) == (0, _lib.DP_TILE_128x128)                           # N = 80: a chunk of 8 would straddle
    assert deconv(20, c_dtype=_lib.DP_F32) == (0, _lib.DP_TILE_128x128)
    assert deconv(24)[1] == _lib.DP_TILE_BIG_256x128
    ws = dict(workspace=256, workspace_bytes=lib.dp_gemm_workspace_size())
    for tile in BIG + (_lib.DP_TILE_STREAMK_256x256, _lib.DP_TILE_P8PH_256x256):
        assert deconv(20, tile=tile, **ws)[0] == SHAPE, tile
        assert deconv(20, tile=tile, c_dtype=_lib.DP_F32, **ws)[0] == SHAPE, tile
    assert deconv(24, tile=_lib.DP_TILE_BIG_256x128)[0] == 0
    assert deconv(20, tile=_lib.DP_TILE_128x128)[0] == 0
    # the model's own deconvs plan exactly as before (cout 256 / 512 / 1024: test_gemm_plan_tile_choice)
    assert deconv(256, S=384, K=256, dtype=_lib.DP_F16, c_dtype=_lib.DP_F16, bias=256, **ws) == \
        (0, _lib.DP_TILE_P8PH_256x256)
    # a patch-conv hint the engine cannot serve is refused by the plan, not at launch
    for tile in (_lib.DP_TILE_CV3_256x256, _lib.DP_TILE_CV3_192x256, _lib.DP_TILE_CV3_384x128):
        assert plan(N=256, tile=tile)[0] == 1000                              # dense A
        assert plan(M=40 * 40, N=256, K=576, tile=tile, a_mode=_lib.DP_A_CONV, in_h=40, in_w=40, in_c=64, k_h=3,
                    k_w=3, stride=1, pad=1, out_h=40, out_w=40)[0] == 1000    # side % 16


def test_empty_inputs_are_refused_before_launch():
    """Zero-size inputs (no rows / images / pixels) return DP_ERR_SHAPE (DP_ERR_ARG for an empty
    group list) from every entry point that takes a size, before any launch (no GPU here: a launch
    would return a HIP error instead).  The reference's torch ops raise on these shapes too."""
    lib = _lib.load()
    P = 4096                      # a dummy non-null pointer: never dereferenced on the host
    f32, f64 = ctypes.c_float, ctypes.c_double
    a = _lib.GemmArgs()
    a.M, a.N, a.K = 0, 64, 64
    a.A = a.B = a.C = P
    a.lda = a.ldb = a.ldc = 64
    calls = {
        "gemm M=0": lambda: lib.dp_gemm(ctypes.byref(a), None),
        "attention batch=0": lambda: lib.dp_attention(P, P, 0, 577, 16, 64, f32(0.125), 0, None),
        "attention seq=0": lambda: lib.dp_attention(P, P, 1, 0, 16, 64, f32(0.125), 0, None),
        "attention_log2q heads=0": lambda: lib.dp_attention_log2q(P, P, 1, 577, 0, 64, 0, None),
        "layernorm rows=0": lambda: lib.dp_layernorm(P, 1024, P, P, P, 1024, 0, 1024, f32(1e-6), 0, None),
        "layernorm_stats rows=0": lambda: lib.dp_layernorm_stats(P, 1024, 0, 1024, P, 1024, None, P, 0, None),
        "normalize_u8 H=0": lambda: lib.dp_normalize_u8(P, 0, 100, P, 0, None),
        "resize_bilinear OH=0": lambda: lib.dp_resize_bilinear(P, 0, 3, 10, 10, P, 0, 10, None),
        "resize H=0": lambda: lib.dp_resize(P, 0, 3, 0, 10, P, 10, 10, 0, None),
        "vit_cls_rows n=0": lambda: lib.dp_vit_cls_rows(P, P, P, 0, None),
        "infer_epilogue H=0": lambda: lib.dp_infer_epilogue(P, 1536, 1536, P, 0, f64(0), 0, 10, P, P, P, None),
        "resize_u8_cv OH=0": lambda: lib.dp_resize_u8_cv(P, 10, 10, P, 0, 5, 3, None),
        "depth_to_points H=0": lambda: lib.dp_depth_to_points(P, 0, 10, P, f64(1.0), 1, P, P, P, P, None),
        "depth_to_image n=0": lambda: lib.dp_depth_to_image(P, 0, P, P, 256, 0, P, None),
    }
    for name, call in calls.items():
        assert call() == 1001, name
    a.M, a.N = 64, 0
    assert lib.dp_gemm(ctypes.byref(a), None) == 1001
    a.N = 64
    assert lib.dp_gemm_grouped(ctypes.byref(a), 0, None) == 1000


def test_attention_and_layernorm_arguments_are_refused_before_launch():
    """dp_mi355x.h, dp_attention / dp_layernorm*: the pointer alignments every 16-B (8-B) load and
    store needs, head_dim, the dtype code, null pointers and the 2^31 grid limit come back as
    DP_ERR_* from the host (no GPU here: a launch would return a HIP error instead)."""
    lib = _lib.load()
    ARG, SHAPE, ALIGN, DTYPE = 1000, 1001, 1002, 1003
    P = 4096                      # dummy, 16-B aligned, never dereferenced on the host
    f32 = ctypes.c_float
    sc = f32(0.125)

    def attn(qkv=P, out=P, batch=1, seq=577, heads=16, hd=64, scale=sc, dt=0):
        return (lib.dp_attention(qkv, out, batch, seq, heads, hd, scale, dt, None),
                lib.dp_attention_log2q(qkv, out, batch, seq, heads, hd, dt, None))

    for off in (2, 4, 8):
        assert attn(qkv=P + off) == (ALIGN, ALIGN), off
        assert attn(out=P + off) == (ALIGN, ALIGN), off
    for hd in (32, 63, 128):
        assert attn(hd=hd) == (SHAPE, SHAPE), hd
    assert attn(dt=_lib.DP_F32) == (DTYPE, DTYPE)
    assert attn(dt=7) == (DTYPE, DTYPE)
    assert attn(qkv=None) == (ARG, ARG) and attn(out=None) == (ARG, ARG)
    # ceil(seq / 128) * heads * batch workgroups: 2^31 is refused (2^31 - 1 would be launched)
    assert attn(batch=1 << 20, seq=1, heads=1 << 11) == (SHAPE, SHAPE)
    assert attn(batch=1 << 20, seq=129, heads=1 << 10) == (SHAPE, SHAPE)
    assert attn(batch=(1 << 31) - 1, seq=128 * 3, heads=1) == (SHAPE, SHAPE)
    for bad in (-0.125, float("nan"), float("inf")):
        assert lib.dp_attention(P, P, 1, 577, 16, 64, f32(bad), 0, None) == ARG, bad

    def ln(x=P, w=P, b=P, y=P, cols=1024, ldx=None, ldy=None, dt=0, rows=5):
        return lib.dp_layernorm(x, cols if ldx is None else ldx, w, b, y, cols if ldy is None else ldy, rows, cols,
                                f32(1e-6), dt, None)

    def lng(x=P, w=(P, P), b=(P, P), y=P, cols=1024, dt=0, rpg=3):
        pw, pb = (ctypes.c_void_p * len(w))(*w), (ctypes.c_void_p * len(b))(*b)
        return lib.dp_layernorm_grouped(x, cols, pw, pb, len(w), y, cols, rpg, cols, f32(1e-6), dt, None)

    for cols in (256, 512, 1024, 2048):
        for off in (4, 8):
            assert ln(x=P + off, cols=cols) == ALIGN, (cols, off)
            assert ln(w=P + off, cols=cols) == ALIGN, (cols, off)
            assert ln(b=P + off, cols=cols) == ALIGN, (cols, off)
            assert lng(x=P + off, cols=cols) == ALIGN, (cols, off)
            assert lng(w=(P, P + off), cols=cols) == ALIGN, (cols, off)
            assert lng(b=(P + off, P), cols=cols) == ALIGN, (cols, off)
        for off in (2, 4, 6):
            assert ln(y=P + off, cols=cols) == ALIGN, (cols, off)
            assert lng(y=P + off, cols=cols) == ALIGN, (cols, off)
        if cols > 256:            # (8-B alignment is enough for the 256-column kernel's stores)
            assert ln(y=P + 8, cols=cols) == ALIGN and lng(y=P + 8, cols=cols) == ALIGN, cols
    assert ln(dt=_lib.DP_F32) == DTYPE and lng(dt=_lib.DP_F32) == DTYPE
    for kw in (dict(x=None), dict(w=None), dict(b=None), dict(y=None)):
        assert ln(**kw) == ARG, kw
    assert lng(w=(P, None)) == ARG and lng(x=None) == ARG
    assert ln(cols=768) == SHAPE and ln(ldx=1026) == SHAPE

    def stats(x=P, xb=P, xl=P, part=P, cols=1024, dt=0):
        return lib.dp_layernorm_stats(x, cols, 5, cols, xb, cols, xl, part, dt, None)

    for off in (4, 8):
        assert stats(x=P + off) == ALIGN and stats(xb=P + off) == ALIGN, off
    for off in (1, 2, 4):
        assert stats(xl=P + off) == ALIGN, off
    assert stats(xb=P + 2) == ALIGN and stats(part=P + 4) == ALIGN
    assert stats(dt=_lib.DP_F32) == DTYPE
    assert stats(x=None) == ARG and stats(xb=None) == ARG and stats(part=None) == ARG
    assert stats(cols=256) == SHAPE
