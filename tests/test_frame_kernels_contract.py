"""The kernels that bracket the network on every frame (csrc/dp_misc.hip), at the edges of what
include/dp_mi355x.h says about them, against fp64: dp_normalize_u8, dp_resize, dp_patchify_pyramid,
dp_vit_cls_rows, dp_merge_windows[_range], dp_fov_tail, dp_infer_epilogue[_mode], dp_depth_to_image.

u = 2^-24 (fp32 unit roundoff), u_out = 2^-8 (bf16) / 2^-11 (f16).  Every bound is per element.

dp_resize.  Reference: the header's formula in real arithmetic, evaluated in fp64.  Per axis, output
index d has the source coordinate s = (in / out)(d + 0.5) - 0.5.  Bilinear: s = max(s, 0), i0 = floor s,
i1 = min(i0 + 1, in - 1), weights (1 - t, t), t = s - i0.  Bicubic: s unclamped, i0 = floor s, taps
i0 - 1 .. i0 + 2 clamped to [0, in - 1], the cubic convolution weights with A = -0.75.  A 16-bit source
is upcast exactly.  The bound has a weight term and a coordinate term:

    weight      u (c sum |wy||wx||v| + sum (ey |wx| + |wy| ex)|v|)
        c counts the roundings a tap's value passes through after its weights exist.  Bilinear:
        lx v, the inner sum, ly (.), the outer sum, the rounding of 1 - t on either axis: 6, taken as
        C_BILINEAR = 8 (second order, one more when the epilogue pre-multiplies).  Bicubic: v cx,
        three additions, r cy, three additions: 8, taken as C_BICUBIC = 10 (+ 1 pre-multiplied).
        e is the absolute error of a bicubic coefficient in units of u.  Horner's intermediates do
        not shrink with the coefficient (the outer polynomial passes through magnitudes up to 6 while
        its value is below 0.15), so the error is absolute.  Outer taps, x in [1, 2]: A x (1.5, carried
        by x^2 <= 4: 6), - 5A (3, x 4: 12), . x (6, x 2: 12), + 8A (3, x 2: 6), . x (3.1), the
        rounding of the argument t + 1 or 2 - t (2 u |cc2'| <= 1.5): 41, taken as 48.  Inner taps,
        x in [0, 1]: 1.25 + 2.25 + 2.25 + 2.25 + 1 and the argument 1 - t (1.35): 10.4, taken as 16.
        Bilinear has e = 0 (the rounding of 1 - t is relative and counted in c).
    coordinate  the kernel forms s in fp32 in three roundings: in / out, the product with d + 0.5 (d +
        0.5 is exact), the subtraction.  With p = (in / out)(d + 0.5):
            ds = u (2 p + |s|)(1 + 2^-20)        (+ u for bicubic: t = s - floor s rounds once)
        Both interpolants are continuous and piecewise polynomial in s, across integer boundaries and
        border clamps, so |f(s^) - f(s)| <= ds sup |f'| <= ds sum L_i |v_i| with L_i = sup |dw_i/ds|
        over a cell: 1 for both bilinear taps; 0.75, 1.35, 1.35, 0.75 for the bicubic ones
        (cc1' = 3.75 x^2 - 4.5 x has its extremum -1.35 at x = 0.6, cc2' = -0.75 (3 x - 4)(x - 2) is
        largest, 0.75, at x = 1).  s^ may lie in the neighbouring cell, so L is taken at the taps of
        s - ds, s and s + ds, whichever is larger per source index.
    The sum of the terms carries a factor 1 + 2^-10 (second order) and 16 * 2^-149 (a product that
    underflows).  Same size in and out is a copy: bit for bit, NaN and infinities included.

dp_infer_epilogue.  scale is an fp32 number the test knows exactly: float32(W / f_given) from the double
with use_given, else float32(W) / f_px with the f_px the device returned (checked on its own, below).
inv = resize(canonical * scale) with the bound above on v = canonical * scale and c + 1 (the product);
same size: inv = canonical * scale, bound u |inv|.  clamp is 1-Lipschitz and the division is IEEE
(dp_normalize_u8's bit-exact test pins that for this file), so
    |1 / depth - clamp(inv_ref)| <= B + u clamp(inv_ref) (1 + 2^-10)
compared as inverse depth (near 1e-4 depth itself magnifies ulp-level differences by 1e4).  Where
inv_ref + B <= 1e-4f or inv_ref - B >= 1e4f the clamped value is a bound and depth must equal
1 / 1e-4f or 1 / 1e4f as fp32, bit for bit.  A NaN stays a NaN.  nonfinite counts exactly the NaN
depths plus a non-finite f_px.

f_px = fl(fl(0.5 W) / tanf(0.5 fl(deg c))), c = fl(pi / 180): deg c carries 2 u relative (constant and
product), halving is exact, tan x changes by (2 x / sin 2 x) per unit relative change of x, the division
rounds once, 0.5 W is exact:  |f_px - ref| / ref <= u (1 + 2 (2 x / sin 2 x))(1 + 2^-10) + tanf's own
error, which cannot be derived: TANF_ALLOWANCE below.

dp_normalize_u8: bit-equal to ((u8 / 255) - 0.5) / 0.5 in fp32 with IEEE division; 16-bit outputs are
that value rounded to nearest even.

dp_patchify_pyramid: rows of windows 0..24 are the input pixels rounded to nearest even.  Rows of
windows 25..34 against the fp64 mean of the four taps the kernel's comment names ({2d, 2d+1} and
{4d+1, 4d+2} per axis).  0.5 (0.5 a + 0.5 b) + 0.5 (0.5 c + 0.5 d): the halvings are exact, every tap
passes through two additions, then the 16-bit rounding of the computed value:
    |out - ref| <= u_out |ref| + 2 (1 + 2^-7) u (|a| + |b| + |c| + |d|) / 4 + sub,
sub = 2^-25 (f16) / 2^-134 (bf16): below the 16-bit normal range a value is rounded on the subnormal
grid, to half its spacing (the ramp crosses zero).

dp_vit_cls_rows, dp_merge_windows[_range]: bit-exact (one fp32 addition; a gather, rounded to nearest
even from an fp32 source).  dp_fov_tail: fp64 dot product, bound (1152 + 8) u (sum |x||w| + |bias|).
dp_depth_to_image: byte-equal to generate_depth_maps.colorize_depth / raw_depth_u16.

Canaries: every output is a slice of a larger allocation with 64 elements before and after the
documented store set; 16-bit elements outside the set hold 0x5A5A, fp32 elements NaN, bytes 0xA5
(int32 words 0x5A5A5A5A) and must be bit-identical after the call.  Inputs carry the same margins.

The CPU self-checks (no GPU) show the bounds are not too tight (a plain fp32 numpy evaluation of the
header formula and CPU F.interpolate pass every case) and not too loose (each seeded mutation of the
fp32 evaluation fails at least one case).
"""

import functools
import math
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from depth_pro import _lib, ops

U = 2.0 ** -24
MARGIN = 64
DT16 = [torch.bfloat16, torch.float16]
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
SUB_OUT = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}
SLACK = 1 + 2.0 ** -10
C_BILINEAR, C_BICUBIC = 8, 10
CUBIC_L = (0.75, 1.35, 1.35, 0.75)
CUBIC_E = (48.0, 16.0, 16.0, 48.0)
CLAMP_LO, CLAMP_HI = np.float32(1e-4), np.float32(1e4)

# The device tanf's own error cannot be derived from the formats.  Measured on MI355X over the sweep of
# test_infer_epilogue_f_px_sweep (FOV 1 deg .. 170 deg in 64 steps, W = 5): the largest value of
# |f_px - ref| / ref minus the derived bound was -1.41 u (profiles/frame_kernels_contract/README.md), i.e.
# no angle exceeds the derived bound and the measured excess is 0; the allowance is twice it.
TANF_EXCESS_MEASURED = 0.0
TANF_ALLOWANCE = 2.0 * TANF_EXCESS_MEASURED


# ------------------------------------------------------------------------ buffers with canary margins
_BITS = {4: torch.int32, 2: torch.int16, 1: torch.uint8}


def _fill_bits(dtype):
    if dtype == torch.float32:
        return 0x7FC00000
    if dtype == torch.int32:
        return 0x5A5A5A5A
    if dtype == torch.uint8:
        return 0xA5
    return 0x5A5A


class Guarded:
    """n elements of `dtype` at element offset MARGIN + shift of a canary-filled allocation (MARGIN
    elements are a multiple of 16 bytes, so `shift` is the misalignment); `t` is the device view."""

    def __init__(self, n, dtype, dev, shift=0, data=None):
        self.n, self.dtype, self.off = n, dtype, MARGIN + shift
        bits = _BITS[torch.empty(0, dtype=dtype).element_size()]
        host = torch.full((self.off + n + MARGIN,), _fill_bits(dtype), dtype=bits)
        if data is not None:
            host[self.off:self.off + n] = data.contiguous().view(-1).view(bits)
        self.host = host
        self.dev = host.to(dev)
        self.t = self.dev[self.off:self.off + n].view(dtype)
        assert self.t.data_ptr() % 16 == (shift * self.t.element_size()) % 16

    def result(self, stored=None):
        """(the n elements after the call, on the CPU; how many canaries changed).  `stored`: bool
        mask of the elements the call may write (default all n)."""
        got = self.dev.cpu()
        keep = torch.ones(got.numel(), dtype=torch.bool)
        keep[self.off:self.off + self.n] = False if stored is None else ~stored.reshape(-1)
        changed = int((got[keep] != self.host[keep]).sum())
        return got[self.off:self.off + self.n].view(self.dtype), changed


def _bits(t):
    return t.contiguous().view(_BITS[t.element_size()])


def _upcast_bits(x):
    """int32 bits of the exact fp32 upcast of x, a NaN's payload included (bf16: the bits shifted up;
    f16: numpy's conversion, which keeps the payload at every position of the array)."""
    if x.dtype == torch.float32:
        return _bits(x)
    if x.dtype == torch.bfloat16:
        return _bits(x).to(torch.int32) << 16
    return torch.from_numpy(_bits(x).numpy().view(np.float16).astype(np.float32).view(np.int32))


def _viol(got, ref, bound):
    """Elements outside the bound (a NaN on either side counts)."""
    return int((~(np.abs(np.asarray(got, dtype=np.float64) - ref) <= bound)).sum())


# --------------------------------------------------------------------- resize: reference and bound
def _cubic_w(t, A=-0.75):
    def cc1(x):
        return ((A + 2) * x - (A + 3)) * x * x + 1

    def cc2(x):
        return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return [cc2(t + 1), cc1(t), cc1(1 - t), cc2(2 - t)]


def _taps64(s, n_in, mode):
    if mode == "bilinear":
        s = np.maximum(s, 0.0)
        i0 = np.floor(s).astype(np.int64)
        t = s - i0
        return [i0, np.minimum(i0 + 1, n_in - 1)], [1 - t, t]
    f = np.floor(s)
    i0 = f.astype(np.int64)
    return [np.clip(i0 - 1 + k, 0, n_in - 1) for k in range(4)], _cubic_w(s - f)


@functools.lru_cache(maxsize=None)
def _axis(n_in, n_out, mode):
    """[n_out][n_in] fp64 matrices of one axis: the weights, their magnitudes, ds * L and e."""
    d = np.arange(n_out, dtype=np.float64)
    p = (n_in / n_out) * (d + 0.5)
    s = p - 0.5
    ds = U * (2 * p + np.abs(s)) * (1 + 2.0 ** -20) + (U if mode == "bicubic" else 0.0)
    rows = np.arange(n_out)

    def scatter(idx, vals):
        m = np.zeros((n_out, n_in))
        for i, v in zip(idx, vals):
            np.add.at(m, (rows, i), np.broadcast_to(v, (n_out,)))
        return m
    idx, w = _taps64(s, n_in, mode)
    L = (1.0, 1.0) if mode == "bilinear" else CUBIC_L
    E = (0.0, 0.0) if mode == "bilinear" else CUBIC_E
    Dm = np.zeros((n_out, n_in))
    for sv in (s - ds, s, s + ds):
        Dm = np.maximum(Dm, scatter(_taps64(sv, n_in, mode)[0], L))
    return scatter(idx, w), scatter(idx, [np.abs(x) for x in w]), Dm * ds[:, None], scatter(idx, E)


def resize_ref(v, OH, OW, mode, premul=False):
    """(ref, bound) fp64 [C][OH][OW] of the finite planes v [C][H][W]."""
    v = np.asarray(v, dtype=np.float64)
    Wy, Ay, Dy, Ey = _axis(v.shape[1], OH, mode)
    Wx, Ax, Dx, Ex = _axis(v.shape[2], OW, mode)
    a = np.abs(v)
    c = (C_BILINEAR if mode == "bilinear" else C_BICUBIC) + (1 if premul else 0)
    ref = Wy @ v @ Wx.T
    bound = U * (c * (Ay @ a @ Ax.T) + Ey @ a @ Ax.T + Ay @ a @ Ex.T) + Dy @ a @ Ax.T + Ay @ a @ Dx.T
    return ref, bound * SLACK + 16 * 2.0 ** -149


RESIZE_MUTATIONS = ["align_corners", "cubic_clamp0", "i1_unclamped", "A_-0.5", "no_half_pixel"]


def resize_eval32(v, OH, OW, mode, mut=None, mul=None):
    """The header formula in plain fp32 numpy, in the kernel's order; `mut` seeds one mistake."""
    f = np.float32
    v = np.asarray(v, dtype=f)
    vp = np.pad(v, ((0, 0), (0, 1), (0, 1)))              # a zero row / column for the unclamped i1

    def coord(n_in, n_out):
        d = np.arange(n_out, dtype=f)
        if mut == "align_corners":
            return d * (f(n_in - 1) / f(max(n_out - 1, 1)))
        if mut == "no_half_pixel":
            return (f(n_in) / f(n_out)) * d
        return (f(n_in) / f(n_out)) * (d + f(0.5)) - f(0.5)

    def ld(yi, xi):
        x = vp[:, yi[:, None], xi[None, :]]
        return x if mul is None else x * f(mul)

    if mode == "bilinear":
        def axis(n_in, n_out):
            s = np.maximum(coord(n_in, n_out), f(0))
            i0 = np.minimum(s.astype(np.int64), n_in - 1)
            i1 = i0 + 1 if mut == "i1_unclamped" else i0 + (i0 < n_in - 1)
            l1 = s - i0.astype(f)
            return i0, i1, f(1) - l1, l1
        y0, y1, ly0, ly1 = axis(v.shape[1], OH)
        x0, x1, lx0, lx1 = axis(v.shape[2], OW)
        ly0, ly1 = ly0[:, None], ly1[:, None]
        return ly0 * (lx0 * ld(y0, x0) + lx1 * ld(y0, x1)) + ly1 * (lx0 * ld(y1, x0) + lx1 * ld(y1, x1))
    A = f(-0.5) if mut == "A_-0.5" else f(-0.75)

    def axis(n_in, n_out):
        s = coord(n_in, n_out)
        if mut == "cubic_clamp0":
            s = np.maximum(s, f(0))
        fl = np.floor(s)
        i0 = fl.astype(np.int64)
        t = s - fl
        cc1 = lambda x: ((A + f(2)) * x - (A + f(3))) * x * x + f(1)            # noqa: E731
        cc2 = lambda x: ((A * x - f(5) * A) * x + f(8) * A) * x - f(4) * A     # noqa: E731
        return ([np.clip(i0 - 1 + k, 0, n_in - 1) for k in range(4)],
                [cc2(t + f(1)), cc1(t), cc1(f(1) - t), cc2(f(2) - t)])
    yi, cy = axis(v.shape[1], OH)
    xi, cx = axis(v.shape[2], OW)
    out = None
    for k in range(4):
        r = ld(yi[k], xi[0]) * cx[0] + ld(yi[k], xi[1]) * cx[1] + ld(yi[k], xi[2]) * cx[2] + ld(yi[k], xi[3]) * cx[3]
        out = r * cy[k][:, None] if out is None else out + r * cy[k][:, None]
    return out


# (H, W) -> (OH, OW): the smallest shapes at which the kernel can go wrong, plus one whose total is
# one more than a multiple of 256 at C = 1 (257 x 1)
RESIZE_SHAPES = [((1, 1), (5, 7)), ((1, 9), (3, 2)), ((5, 1), (1, 33)), ((2, 3), (64, 65)), ((3, 3), (200, 1)),
                 ((8, 8), (16, 16)), ((16, 16), (8, 8)), ((37, 53), (19, 11)), ((100, 100), (99, 101)),
                 ((300, 517), (64, 96)), ((3, 3), (257, 1))]
RESIZE_IDS = [f"{a[0]}x{a[1]}_to_{b[0]}x{b[1]}" for a, b in RESIZE_SHAPES]
RESIZE_C = (1, 2, 5)
MODES = ["bilinear", "bicubic"]
SRC_DT = [torch.float32, torch.bfloat16, torch.float16]


@functools.lru_cache(maxsize=None)
def resize_source(si, C, dt):
    """[C][H][W] CPU tensor of `dt`: unit noise round an offset, with a few values 1000 times larger."""
    (H, W), _ = RESIZE_SHAPES[si]
    g = torch.Generator().manual_seed(9100 + 10 * si + C)
    x = torch.randn(C, H, W, generator=g) + 0.25
    flat = x.view(-1)
    flat[::17] *= 1000.0
    return x.to(dt)


@functools.lru_cache(maxsize=None)
def resize_reference(si, C, dt, mode):
    _, (OH, OW) = RESIZE_SHAPES[si]
    return resize_ref(resize_source(si, C, dt).double().numpy(), OH, OW, mode)


def _resize_cases():
    for si in range(len(RESIZE_SHAPES)):
        for C in RESIZE_C:
            for dt in SRC_DT:
                yield si, C, dt


# ------------------------------------------------------------------ infer epilogue: cases, reference
EPI_CANON = [(16, 16), (24, 40), (7, 5)]
EPI_OUT = ["same", (33, 17), (5, 64)]
EPI_SCALES = ["unit", "given", "fov", "tiny"]
F_GIVEN = 1234.5678901
FOV_DEG = 41.7
EPI_MUTATIONS = ["scale_after", "clamp_first"]


def _epi_hw(shape, out):
    return shape if out == "same" else out


@functools.lru_cache(maxsize=None)
def epi_canon(ci, oi, kind):
    """fp32 numpy canonical map.  `tiny`: subnormal values that the scale 1e38 brings to 1e-3 .. 3e-3
    (the product must come before the resize).  Otherwise magnitudes over twelve decades, a tenth
    negative; same size adds values on, next to and far beyond both clamp bounds (scale 1 lands them
    exactly), the multiplier 32 that pins the given scale, and +-inf / NaN."""
    SH, SW = EPI_CANON[ci]
    rng = np.random.default_rng(500 + 10 * ci + oi)
    if kind == "tiny":
        return ((1 + 2 * rng.random((SH, SW))) * 1e-41).astype(np.float32)
    c = (10.0 ** rng.uniform(-6, 6, (SH, SW))).astype(np.float32)
    c[rng.random((SH, SW)) < 0.1] *= -1
    if EPI_OUT[oi] == "same":
        f = c.reshape(-1)
        lo, hi = CLAMP_LO, CLAMP_HI
        f[:12] = [32.0, lo, np.nextafter(lo, np.float32(0)), np.nextafter(lo, np.float32(1)), hi,
                  np.nextafter(hi, np.float32(0)), np.nextafter(hi, np.float32(1e9)), 1e-9, 1e9, -3.0,
                  0.0, -0.0]
        f[12:15] = [np.inf, -np.inf, np.nan]
    return c


def epi_given(W, kind):
    """f_given of a use_given case (None: the FOV path)."""
    return {"unit": float(W), "given": F_GIVEN, "tiny": W * 1e-38, "fov": None}[kind]


def epi_reference(canon, scale, H, W, mode):
    """(inv_ref, B) fp64: the unclamped inverse depth and its bound; scale an fp32 number."""
    c64, s64 = canon.astype(np.float64), float(scale)
    if canon.shape == (H, W):
        with np.errstate(invalid="ignore"):
            inv = c64 * s64
        return inv, np.where(np.isfinite(inv), U * np.abs(inv), 0.0) + 2.0 ** -149
    ref, b = resize_ref((c64 * s64)[None], H, W, mode, premul=True)
    return ref[0], b[0]


def epi_violations(depth, inv_ref, B):
    """Elements of the fp32 depth map that break the contract (see the module docstring)."""
    depth = np.asarray(depth, dtype=np.float32)
    lo, hi = float(CLAMP_LO), float(CLAMP_HI)
    nan = np.isnan(inv_ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        cl = np.clip(inv_ref, lo, hi)
        close = np.abs(1.0 / depth.astype(np.float64) - cl) <= B + U * cl * SLACK
        sure_lo, sure_hi = inv_ref + B <= lo, inv_ref - B >= hi
    ok = np.where(nan, np.isnan(depth), close)
    ok = np.where(sure_lo, depth == np.float32(1) / CLAMP_LO, ok)
    ok = np.where(sure_hi, depth == np.float32(1) / CLAMP_HI, ok)
    return int((~ok).sum())


def epi_eval32(canon, scale, H, W, mode, mut=None):
    """depth in plain fp32 numpy: 1 / clamp(resize(canonical * scale)); `mut` seeds one mistake."""
    f = np.float32
    scale = f(scale)
    same = canon.shape == (H, W)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        if mut == "clamp_first":
            x = np.clip(canon * scale, CLAMP_LO, CLAMP_HI)
            v = x if same else resize_eval32(x[None], H, W, mode)[0]
        elif mut == "scale_after":
            v = (canon if same else resize_eval32(canon[None], H, W, mode)[0]) * scale
        else:
            v = canon * scale if same else resize_eval32(canon[None], H, W, mode, mul=scale)[0]
        v = np.where(np.isnan(v), v, np.minimum(np.maximum(v, CLAMP_LO), CLAMP_HI)).astype(f)
        return f(1) / v


def _epi_cases():
    for ci in range(len(EPI_CANON)):
        for oi in range(len(EPI_OUT)):
            for mode in MODES:
                for kind in EPI_SCALES:
                    yield ci, oi, mode, kind


def _epi_scale_cpu(W, kind):
    """The fp32 scale of a case on the CPU (the FOV path with numpy's fp32 tan)."""
    fg = epi_given(W, kind)
    if fg is not None:
        return np.float32(W / fg)
    fpx = (np.float32(0.5) * np.float32(W)) / np.tan(np.float32(0.5) * (np.float32(FOV_DEG) * np.float32(math.pi / 180)))
    return np.float32(W) / np.float32(fpx)


# ----------------------------------------------------------------------- patchify: reference, bound
@functools.lru_cache(maxsize=None)
def patchify_input():
    """[3][1536][1536] fp32: a ramp that encodes (c, y, x) plus noise of amplitude 0.25, so a tap
    shifted by one pixel moves a value by far more than the bound."""
    g = torch.Generator().manual_seed(77)
    y = torch.arange(1536, dtype=torch.float32)
    ramp = (torch.arange(3, dtype=torch.float32) - 1).view(3, 1, 1) * 0.5 + (y / 1536 - 0.5).view(1, -1, 1) + \
        0.37 * (y / 1536).view(1, 1, -1)
    return ramp + 0.25 * torch.randn(3, 1536, 1536, generator=g)


def _im2col(wins):
    """[n][3][384][384] -> [n * 576][768], row = window * 576 + py * 24 + px, column = c * 256 + ky * 16 + kx."""
    n = wins.shape[0]
    return wins.reshape(n, 3, 24, 16, 24, 16).permute(0, 2, 4, 1, 3, 5).reshape(n * 576, 768)


def _windows(level, steps, stride):
    return torch.stack([level[:, j * stride:j * stride + 384, i * stride:i * stride + 384]
                        for j in range(steps) for i in range(steps)])


def _box(x, a, step):
    """The four taps {a, a + 1} x {a, a + 1} at stride `step` of each plane."""
    return [x[:, a + dy::step, a + dx::step] for dy in (0, 1) for dx in (0, 1)]


@functools.lru_cache(maxsize=None)
def patchify_reference():
    """(exact fp32 rows of windows 0..24, fp64 ref and tap magnitude of the rows of windows 25..34)."""
    x = patchify_input()
    x64 = x.double()
    exact = _im2col(_windows(x, 5, 288))
    ref, mag = [], []
    for a, step, steps in ((0, 2, 3), (1, 4, 1)):
        taps = _box(x64, a, step)
        ref.append(_im2col(_windows(sum(taps) / 4, steps, 192)))
        mag.append(_im2col(_windows(sum(t.abs() for t in taps) / 4, steps, 192)))
    return exact, torch.cat(ref).numpy(), torch.cat(mag).numpy()


def patchify_bound(dt):
    _, ref, mag = patchify_reference()
    return U_OUT[dt] * np.abs(ref) + 2 * (1 + 2.0 ** -7) * U * mag + SUB_OUT[dt]


def patchify_eval32(dt, mut=None):
    """Rows of windows 25..34 in fp32 in the kernel's order, rounded to `dt`."""
    x = patchify_input()
    rows = []
    for a, step, steps in ((0, 2, 3), (0 if mut == "patchify_taps_4d" else 1, 4, 1)):
        t = _box(x, a, step)
        lvl = 0.5 * (0.5 * t[0] + 0.5 * t[1]) + 0.5 * (0.5 * t[2] + 0.5 * t[3])
        rows.append(_im2col(_windows(lvl, steps, 192)))
    return torch.cat(rows).to(dt).double().numpy()


# ------------------------------------------------------------------------------ fov tail: cases
FOV_KINDS = ["random", "cancel", "f16_max"]


@functools.lru_cache(maxsize=None)
def fov_problem(kind, dt):
    """x6 [1152] of `dt` (NHWC: (ky * 6 + kx) * 32 + ci), w fp32 [32][36], bias; (ref, bound) fp64."""
    g = torch.Generator().manual_seed(4000 + FOV_KINDS.index(kind))
    x = torch.randn(1152, generator=g)
    w = torch.randn(32, 36, generator=g) * 0.05
    bias = 0.3
    if kind == "cancel":                                   # large terms of opposite sign that cancel
        x = 1000.0 * (1 - 2 * (torch.arange(1152) % 2).float()) + x
        w = torch.ones(32, 36) + 0.001 * torch.randn(32, 36, generator=g)
        bias = -0.125
    elif kind == "f16_max":                                # 16-bit values next to f16's largest, 65504
        x = (65504.0 - 32.0 * torch.randint(0, 8, (1152,), generator=g).float()) * (1 - 2 * (torch.arange(1152) % 3 == 0).float())
        bias = 1e4
    x = x.to(dt)
    wk = w.t().reshape(-1)                                 # [tap][ci], the order of x6
    prod = x.double() * wk.double()
    ref = float(prod.sum() + bias)
    bound = (1152 + 8) * U * (float(prod.abs().sum()) + abs(bias))
    return x, w.contiguous(), bias, ref, bound


# ================================================================================== CPU self-checks
def test_selfcheck_resize_fp32_and_interpolate_pass():
    """Not too tight: the plain fp32 evaluation and CPU F.interpolate (fp32) pass every case."""
    worst = 0.0
    for si, C, dt in _resize_cases():
        _, (OH, OW) = RESIZE_SHAPES[si]
        src = resize_source(si, C, dt).float()
        for mode in MODES:
            ref, bound = resize_reference(si, C, dt, mode)
            ev = resize_eval32(src.numpy(), OH, OW, mode)
            assert _viol(ev, ref, bound) == 0, (RESIZE_IDS[si], C, dt, mode, "fp32 evaluation")
            ti = F.interpolate(src[None], size=(OH, OW), mode=mode, align_corners=False)[0].numpy()
            assert _viol(ti, ref, bound) == 0, (RESIZE_IDS[si], C, dt, mode, "F.interpolate")
            worst = max(worst, float((np.abs(ti - ref) / bound).max()))
    assert worst > 0.01, worst          # the bound is within two orders of what correct code reaches


@pytest.mark.parametrize("mut", RESIZE_MUTATIONS)
def test_selfcheck_resize_mutation_is_caught(mut):
    """Not too loose: the seeded mistake breaks the bound in at least one case."""
    caught = []
    for si, C, dt in _resize_cases():
        if dt != torch.float32:
            continue
        _, (OH, OW) = RESIZE_SHAPES[si]
        for mode in MODES:
            ref, bound = resize_reference(si, C, dt, mode)
            if _viol(resize_eval32(resize_source(si, C, dt).numpy(), OH, OW, mode, mut=mut), ref, bound):
                caught.append((RESIZE_IDS[si], C, mode))
    assert caught, mut


def test_selfcheck_epilogue_fp32_and_interpolate_pass():
    for ci, oi, mode, kind in _epi_cases():
        H, W = _epi_hw(EPI_CANON[ci], EPI_OUT[oi])
        canon, scale = epi_canon(ci, oi, kind), _epi_scale_cpu(W, kind)
        inv_ref, B = epi_reference(canon, scale, H, W, mode)
        tag = (EPI_CANON[ci], EPI_OUT[oi], mode, kind)
        assert epi_violations(epi_eval32(canon, scale, H, W, mode), inv_ref, B) == 0, tag
        inv = torch.from_numpy(canon)[None, None] * float(scale)
        if canon.shape != (H, W):
            inv = F.interpolate(inv, size=(H, W), mode=mode, align_corners=False)
        assert epi_violations((1.0 / torch.clamp(inv, 1e-4, 1e4))[0, 0].numpy(), inv_ref, B) == 0, tag


@pytest.mark.parametrize("mut", EPI_MUTATIONS)
def test_selfcheck_epilogue_mutation_is_caught(mut):
    caught = []
    for ci, oi, mode, kind in _epi_cases():
        H, W = _epi_hw(EPI_CANON[ci], EPI_OUT[oi])
        canon, scale = epi_canon(ci, oi, kind), _epi_scale_cpu(W, kind)
        inv_ref, B = epi_reference(canon, scale, H, W, mode)
        if epi_violations(epi_eval32(canon, scale, H, W, mode, mut=mut), inv_ref, B):
            caught.append((ci, oi, mode, kind))
    assert caught, mut


def test_selfcheck_given_scale_is_the_double_quotient():
    """The pixel that pins scale = float32(W / f_given) at W = 40: canonical 32 puts 32 * scale in
    [1, sqrt 2), where 1 / v moves by more than one fp32 step per step of v, so the depth there
    differs for either neighbouring fp32 scale and the bit-exact check pins every bit of it."""
    right = np.float32(40 / F_GIVEN)
    one, c = np.float32(1), np.float32(32)
    assert 1 <= c * right < math.sqrt(2)
    for wrong in (np.nextafter(right, np.float32(0)), np.nextafter(right, one)):
        assert one / (c * right) != one / (c * wrong)


@pytest.mark.parametrize("dt", DT16)
def test_selfcheck_patchify(dt):
    from oracle import depth_pro_oracle as O

    _, ref, _ = patchify_reference()
    bound = patchify_bound(dt)
    assert _viol(patchify_eval32(dt), ref, bound) == 0
    _, x1, x2 = O.pyramid(patchify_input()[None])            # F.interpolate's levels
    tor = torch.cat((_im2col(O.split(x1, 0.5)), _im2col(x2))).to(dt).double().numpy()
    assert _viol(tor, ref, bound) == 0
    assert _viol(patchify_eval32(dt, mut="patchify_taps_4d"), ref, bound) > 0


@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("kind", FOV_KINDS)
def test_selfcheck_fov_tail(kind, dt):
    x, w, bias, ref, bound = fov_problem(kind, dt)
    acc = np.float32(0)
    for v, c in zip(x.float().numpy(), w.t().reshape(-1).numpy()):
        acc = np.float32(acc + v * c)
    assert abs(float(np.float32(acc + np.float32(bias))) - ref) <= bound
    conv = F.conv2d(x.float().view(6, 6, 32).permute(2, 0, 1)[None], w.view(1, 32, 6, 6), torch.tensor([bias]))
    assert abs(conv.item() - ref) <= bound


# ======================================================================================== GPU tests
# ------------------------------------------------------------------------------------ dp_normalize_u8
@pytest.mark.gpu
@pytest.mark.parametrize("HW", [(1, 1), (3, 85), (1, 257), (17, 31)])
def test_normalize_u8_bit_exact(cuda, HW):
    """Pixel i holds (i (2 c + 1) + 85 c + 7) mod 256 in channel c: from 256 pixels on (1 x 257, 17 x 31)
    every byte value in every channel."""
    H, W = HW
    i = np.arange(H * W, dtype=np.int64)[:, None]
    img = ((i * (2 * np.arange(3) + 1) + 85 * np.arange(3) + 7) % 256).astype(np.uint8).reshape(H, W, 3)
    if H * W >= 256:
        assert all(len(np.unique(img[..., c])) == 256 for c in range(3))
    f = np.float32
    ref = torch.from_numpy(((img.astype(f) / f(255) - f(0.5)) / f(0.5)).transpose(2, 0, 1).copy())
    src = Guarded(H * W * 3, torch.uint8, cuda, data=torch.from_numpy(img))
    for dt in [torch.float32] + DT16:
        out = Guarded(3 * H * W, dt, cuda)
        ops.normalize_u8(src.t.view(H, W, 3), out.t.view(3, H, W))
        got, changed = out.result()
        assert changed == 0, dt
        assert torch.equal(_bits(got), _bits(ref.to(dt)).view(-1)), dt      # .to: round to nearest even


# ------------------------------------------------------------------------------------------ dp_resize
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("si", range(len(RESIZE_SHAPES)), ids=RESIZE_IDS)
def test_resize_against_fp64(cuda, si, mode, record):
    _, (OH, OW) = RESIZE_SHAPES[si]
    worst = 0.0
    for C in RESIZE_C:
        for dt in SRC_DT:
            x = resize_source(si, C, dt)
            src = Guarded(x.numel(), dt, cuda, data=x)
            dst = Guarded(C * OH * OW, torch.float32, cuda)
            ops.resize(src.t.view(x.shape), dst.t.view(C, OH, OW), mode)
            got, changed = dst.result()
            ref, bound = resize_reference(si, C, dt, mode)
            got = got.view(C, OH, OW).numpy()
            worst = max(worst, float(np.nanmax(np.abs(got - ref) / bound)))
            assert changed == 0, (C, dt)
            assert _viol(got, ref, bound) == 0, (C, dt)
    print(f"resize {RESIZE_IDS[si]} {mode}: max |d| / bound {worst:.3f}")
    record("max_err_over_bound", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", SRC_DT)
def test_resize_same_size_copies_at_any_alignment(cuda, dt, mode):
    """Same size in and out is a copy whatever the element alignment of the two bases (16 B, and + 4 B
    for fp32 / + 2 B for a 16-bit source), NaN and +-inf included: at the first and last element, at
    both neighbours of a float4 boundary (3, 4) and of the 1024-element block boundary."""
    C, H, W = 3, 37, 53
    n = C * H * W                                           # 5883 = 4 * 1470 + 3: a scalar tail
    x = torch.randn(n, generator=torch.Generator().manual_seed(31))
    for k, v in zip((0, 3, 4, 1023, 1024, n - 1), (float("nan"), float("inf"), float("nan"), -float("inf"),
                                                   float("nan"), float("nan"))):
        x[k] = v
    x = x.to(dt)
    want = _upcast_bits(x)
    for s_shift in (0, 1):
        for d_shift in (0, 1):
            src = Guarded(n, dt, cuda, shift=s_shift, data=x)
            dst = Guarded(n, torch.float32, cuda, shift=d_shift)
            ops.resize(src.t.view(C, H, W), dst.t.view(C, H, W), mode)
            got, changed = dst.result()
            assert changed == 0, (s_shift, d_shift)
            bad = (_bits(got) != want).nonzero().view(-1)
            assert bad.numel() == 0, (s_shift, d_shift, bad[:8].tolist())


# ------------------------------------------------------------------------------- dp_patchify_pyramid
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DT16)
def test_patchify_pyramid_strict(cuda, dt, record):
    exact, ref, _ = patchify_reference()
    x = patchify_input()
    src = Guarded(x.numel(), torch.float32, cuda, data=x)
    cols = Guarded(35 * 576 * 768, dt, cuda)
    ops.patchify_pyramid(src.t.view(3, 1536, 1536), cols.t.view(35 * 576, 768))
    got, changed = cols.result()
    got = got.view(35 * 576, 768)
    assert changed == 0
    assert torch.equal(_bits(got[:25 * 576]), _bits(exact.to(dt)))
    low = got[25 * 576:].double().numpy()
    bound = patchify_bound(dt)
    record("max_err_over_bound", (np.abs(low - ref) / bound).max())
    print(f"patchify {dt}: max |d| / bound {(np.abs(low - ref) / bound).max():.3f}")
    assert _viol(low, ref, bound) == 0


# ----------------------------------------------------------------------------------- dp_vit_cls_rows
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 35])
def test_vit_cls_rows_touch_only_the_cls_rows(cuda, n):
    g = torch.Generator().manual_seed(n)
    cls, pos = torch.randn(1024, generator=g), torch.randn(1024, generator=g)
    rows = (n - 1) * 577 + 1
    x = Guarded(rows * 1024, torch.float32, cuda)
    c, p = Guarded(1024, torch.float32, cuda, data=cls), Guarded(1024, torch.float32, cuda, data=pos)
    ops.vit_cls_rows(x.t, c.t, p.t, n)
    stored = torch.zeros(rows, 1024, dtype=torch.bool)
    stored[::577] = True
    got, changed = x.result(stored)
    assert changed == 0                                     # every other row of x included
    assert torch.equal(_bits(got.view(rows, 1024)[::577]), _bits((cls + pos).expand(n, 1024)))


# ------------------------------------------------------------------------- dp_merge_windows[_range]
MERGE_GRIDS = [(1, 7), (2, 0), (2, 11), (3, 6), (4, 5)]     # (steps, pad); (1, 7) must ignore the pad
MERGE_MAX_ROWS = (3 + 16) * 577


@functools.lru_cache(maxsize=None)
def merge_pool():
    """fp32 [19 * 577][1032]: every token row of every case, the cls rows and the [1024, ld) padding
    columns included, all different."""
    return torch.randn(MERGE_MAX_ROWS, 1032, generator=torch.Generator().manual_seed(23))


def merge_source(steps, ld, w0, src_dt):
    rows = (w0 + steps * steps) * 577
    return merge_pool()[:rows, :ld].contiguous().to(src_dt)


def merge_expected(src, steps, pad, w0, dt):
    """([S * S][1024] of `dt`, [S * S] window of every pixel) by oracle.depth_pro_oracle.merge."""
    from oracle import depth_pro_oracle as O

    n = steps * steps
    tok = src[w0 * 577:(w0 + n) * 577, :1024].float().reshape(n, 577, 1024)
    ref = O.merge(O.tokens_to_nchw(tok), 1, pad)[0]
    ids = O.merge(torch.arange(n).view(n, 1, 1, 1).expand(n, 1, 24, 24).contiguous(), 1, pad)[0, 0]
    S = ref.shape[-1]
    assert S == (24 if steps == 1 else steps * 24 - 2 * pad * (steps - 1))
    return ref.permute(1, 2, 0).reshape(S * S, 1024).to(dt), ids.reshape(-1)


def _merge_case(i):
    """(ld, first_window, fp32 source?) of the i-th case: all combinations come up."""
    return (1024, 1032)[i % 2], (0, 3)[(i // 2) % 2], (i // 4) % 2 == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("src_f32", [True, False])
@pytest.mark.parametrize("gi", range(len(MERGE_GRIDS)), ids=[f"s{s}_p{p}" for s, p in MERGE_GRIDS])
def test_merge_windows_bit_exact(cuda, gi, src_f32, dt):
    steps, pad = MERGE_GRIDS[gi]
    for ld, w0 in ((1024, 0), (1032, 3)) if (gi + src_f32) % 2 else ((1032, 0), (1024, 3)):
        s = merge_source(steps, ld, w0, torch.float32 if src_f32 else dt)
        want, _ = merge_expected(s, steps, pad, w0, dt)
        src = Guarded(s.numel(), s.dtype, cuda, data=s)
        dst = Guarded(want.numel(), dt, cuda)
        ops.merge_windows(src.t.view(s.shape), w0, steps, pad, dst.t, ld=ld)
        got, changed = dst.result()
        assert changed == 0, (ld, w0)
        assert torch.equal(_bits(got), _bits(want).view(-1)), (ld, w0)


def _merge_ranges(steps):
    n = steps * steps
    mid = n // 2
    return [(0, 1), (mid, mid + 1), (steps - 1, 2 * steps - 1), (n - 1, n)]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("gi", [3, 4], ids=["s3_p6", "s4_p5"])
def test_merge_windows_range_writes_only_its_windows(cuda, gi, dt):
    steps, pad = MERGE_GRIDS[gi]
    n = steps * steps
    ld, w0, f32 = _merge_case(gi + (dt == torch.float16))
    s = merge_source(steps, ld, w0, torch.float32 if f32 else dt)
    want, ids = merge_expected(s, steps, pad, w0, dt)
    src = Guarded(s.numel(), s.dtype, cuda, data=s)
    for lo, hi in _merge_ranges(steps):
        dst = Guarded(want.numel(), dt, cuda)
        ops.merge_windows(src.t.view(s.shape), w0, steps, pad, dst.t, ld=ld, windows=(lo, hi))
        inside = (ids >= lo) & (ids < hi)
        assert 0 < int(inside.sum()) < ids.numel()
        stored = inside[:, None].expand(-1, 1024)
        got, changed = dst.result(stored)
        assert changed == 0, (lo, hi)                       # pixels of the other windows keep the canary
        assert torch.equal(_bits(got.view(-1, 1024)[inside]), _bits(want[inside])), (lo, hi)
    # disjoint ranges that cover the grid, out of order, into one canary-filled dst == the full merge
    dst = Guarded(want.numel(), dt, cuda)
    for lo, hi in ((steps + 1, n - 1), (n - 1, n), (0, 2), (2, steps + 1)):
        ops.merge_windows(src.t.view(s.shape), w0, steps, pad, dst.t, ld=ld, windows=(lo, hi))
    got, changed = dst.result()
    assert changed == 0
    assert torch.equal(_bits(got), _bits(want).view(-1))


@pytest.mark.gpu
def test_merge_windows_rejects(cuda):
    lib = _lib.load()
    BF, F16, F32 = _lib.DP_BF16, _lib.DP_F16, _lib.DP_F32
    src = torch.zeros(9 * 577 * 1032, device=cuda)
    dst = Guarded(48 * 48 * 1024, torch.bfloat16, cuda)
    st = torch.cuda.current_stream().cuda_stream

    def rng(src_dt=F32, ld=1024, steps=3, pad=6, lo=0, hi=9, dt=BF):
        return lib.dp_merge_windows_range(src.data_ptr(), src_dt, ld, 0, steps, pad, lo, hi, dst.t.data_ptr(), dt, st)

    def full(src_dt=F32, ld=1024, steps=3, pad=6, dt=BF):
        return lib.dp_merge_windows(src.data_ptr(), src_dt, ld, 0, steps, pad, dst.t.data_ptr(), dt, st)
    SHAPE, DTYPE = 1001, 1003                               # DP_ERR_SHAPE, DP_ERR_DTYPE
    assert rng(ld=1028) == SHAPE and full(ld=1028) == SHAPE
    assert rng(pad=12) == SHAPE and full(pad=12) == SHAPE and full(steps=2, pad=13) == SHAPE
    assert rng(lo=4, hi=4) == SHAPE and rng(lo=5, hi=4) == SHAPE
    assert rng(hi=10) == SHAPE and rng(lo=-1) == SHAPE
    assert rng(src_dt=F16) == DTYPE and full(src_dt=F16) == DTYPE and rng(src_dt=BF, dt=F16) == DTYPE
    assert rng(dt=F32) == DTYPE and full(dt=F32) == DTYPE
    torch.cuda.synchronize()
    assert dst.result(torch.zeros(dst.n, dtype=torch.bool))[1] == 0     # a reject launches nothing
    assert full(steps=1, pad=12) == 0                       # steps == 1 ignores the pad
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------- dp_fov_tail
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DT16)
@pytest.mark.parametrize("kind", FOV_KINDS)
def test_fov_tail_against_fp64(cuda, kind, dt, record):
    x, w, bias, ref, bound = fov_problem(kind, dt)
    xs = Guarded(1152, dt, cuda, data=x)
    ws = Guarded(1152, torch.float32, cuda, data=w)
    out = Guarded(1, torch.float32, cuda)
    ops.fov_tail(xs.t, ws.t, bias, out.t)
    got, changed = out.result()
    assert changed == 0
    print(f"fov_tail {kind} {dt}: |d| / bound {abs(got.item() - ref) / bound:.4f}")
    record("err_over_bound", abs(got.item() - ref) / bound)
    assert abs(got.item() - ref) <= bound


# --------------------------------------------------------------------------------- dp_infer_epilogue
def _run_epilogue(cuda, canon, fov, f_given, H, W, mode, want_fpx, want_count, count0=None):
    """One call with canaried buffers: (depth numpy, f_px or None, count or None)."""
    src = Guarded(canon.size, torch.float32, cuda, data=torch.from_numpy(canon))
    depth = Guarded(H * W, torch.float32, cuda)
    fpx = Guarded(1, torch.float32, cuda) if want_fpx else None
    cnt = Guarded(1, torch.int32, cuda, data=torch.tensor([count0 or 0], dtype=torch.int32)) if want_count else None
    fv = Guarded(1, torch.float32, cuda, data=torch.tensor([fov], dtype=torch.float32)) if fov is not None else None
    ops.infer_epilogue(src.t.view(canon.shape), fv.t if fv else None, f_given, H, W, depth.t.view(H, W),
                       fpx.t if fpx else None, cnt.t if cnt else None, mode=mode)
    d, changed = depth.result()
    assert changed == 0
    out = [d.view(H, W).numpy(), None, None]
    for k, b in ((1, fpx), (2, cnt)):
        if b is not None:
            v, changed = b.result()
            assert changed == 0
            out[k] = v[0].item() if k == 2 else v.numpy()[0]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("oi", range(len(EPI_OUT)), ids=["same", "33x17", "5x64"])
@pytest.mark.parametrize("ci", range(len(EPI_CANON)), ids=["16x16", "24x40", "7x5"])
def test_infer_epilogue_against_fp64(cuda, ci, oi, mode):
    """unit: f_given = W (scale 1), f_px_out None, nonfinite given.  given: f_given = 1234.5678901,
    f_px_out given, nonfinite None.  fov: the FOV path, both given.  tiny: scale 1e38 on subnormal
    canonical values, both None."""
    H, W = _epi_hw(EPI_CANON[ci], EPI_OUT[oi])
    same = EPI_OUT[oi] == "same"
    for kind in EPI_SCALES:
        canon, fg = epi_canon(ci, oi, kind), epi_given(W, kind)
        depth, fpx, count = _run_epilogue(cuda, canon, FOV_DEG if fg is None else None, fg, H, W, mode,
                                          want_fpx=kind in ("given", "fov"), want_count=kind in ("unit", "fov"))
        if fg is None:
            scale = np.float32(W) / np.float32(fpx)
        else:
            scale = np.float32(W / fg)                       # the double quotient, then one rounding
            if fpx is not None:
                assert np.float32(fpx).tobytes() == np.float32(fg).tobytes()
        inv_ref, B = epi_reference(canon, scale, H, W, mode)
        bad = epi_violations(depth, inv_ref, B)
        assert bad == 0, kind
        if count is not None:
            assert count == int(np.isnan(depth).sum()), kind
            if same:
                assert count == int(np.isnan(canon).sum()) == 1, kind
        if same and kind == "unit":                          # landed exactly on a bound, and beyond
            d = depth.reshape(-1)
            one = np.float32(1)
            assert d[1] == d[2] == d[7] == d[9] == d[10] == d[11] == d[13] == one / CLAMP_LO
            assert d[4] == d[6] == d[8] == d[12] == one / CLAMP_HI
            assert d[3] == one / np.nextafter(CLAMP_LO, one) and d[5] == one / np.nextafter(CLAMP_HI, np.float32(0))
            assert np.isnan(d[14])
        if same and kind == "given" and W == 40:             # scale == float32(W / f_given) bit for bit
            assert depth.reshape(-1)[0] == np.float32(1) / (np.float32(32) * scale)


@pytest.mark.gpu
@pytest.mark.parametrize("fov", [57.3, float("nan")], ids=["finite_fov", "nan_fov"])
def test_infer_epilogue_nonfinite_count_is_exact(cuda, fov):
    """A 9 x 23 map (207 = 3 * 64 + 15 pixels): NaN at lanes 0, 1 (next to thread 0's f_px add) and 63
    of wave 0, three in wave 1, one in the last, partial wave and one in the last pixel.  The count is
    exact and accumulates across two calls without a reset."""
    H, W = 9, 23
    canon = (0.5 + np.random.default_rng(5).random((H, W))).astype(np.float32)
    where = [0, 1, 63, 70, 71, 100, 200, 206]
    canon.reshape(-1)[where] = np.nan
    want = H * W + 1 if math.isnan(fov) else len(where)
    for mode in MODES:
        depth, fpx, c1 = _run_epilogue(cuda, canon, fov, None, H, W, mode, True, True)
        assert c1 == want and int(np.isnan(depth).sum()) == want - math.isnan(fov)
        assert math.isnan(fpx) == math.isnan(fov)
        _, _, c2 = _run_epilogue(cuda, canon, fov, None, H, W, mode, False, True, count0=c1)
        assert c2 == 2 * want
        _, _, c3 = _run_epilogue(cuda, canon, None, 800.0, H, W, mode, False, True, count0=5)
        assert c3 == 5 + len(where)


@pytest.mark.gpu
def test_infer_epilogue_f_px_sweep(cuda, record):
    """f_px over FOV 1 .. 170 degrees in 64 steps (and 0 degrees: tan 0 = 0, f_px = +inf) against fp64."""
    W = 5
    canon = np.ones((1, W), dtype=np.float32)
    excess = -np.inf
    for deg in [0.0] + list(np.linspace(1.0, 170.0, 64)):
        deg32 = float(np.float32(deg))
        _, fpx, count = _run_epilogue(cuda, canon, deg32, None, 1, W, "bilinear", True, True)
        if deg == 0.0:
            assert fpx == np.inf and count == 1             # scale 0 -> clamp -> finite depth
            continue
        x = 0.5 * math.radians(deg32)
        ref = 0.5 * W / math.tan(x)
        derived = U * (1 + 2 * (2 * x / math.sin(2 * x))) * SLACK
        err = abs(float(fpx) - ref) / ref
        excess = max(excess, (err - derived) / U)
        assert count == 0
        assert err <= derived + TANF_ALLOWANCE * U, (deg32, err / U, derived / U)
    print(f"f_px sweep: largest (relative error - derived bound) / u = {excess:.3f}")
    record("tanf_excess_over_derived_in_u", excess)


# --------------------------------------------------------------------------------- dp_depth_to_image
DEPTH_MAPS = ["pos_inf", "neg_inf", "negative", "neg_zero_min", "all_nan", "one_finite"]


def _depth_map(kind, n):
    d = (np.random.default_rng(n).random(n, dtype=np.float32) * 30 + 0.05).astype(np.float32)
    k = n // 2
    if kind == "pos_inf":
        d[k] = np.inf
    elif kind == "neg_inf":
        d[k] = -np.inf
    elif kind == "negative":
        d[::2] *= -1
    elif kind == "neg_zero_min":
        d[k] = -0.0
        d[n - 1] = 0.0 if n > 1 else d[n - 1]
    elif kind == "all_nan":
        d[:] = np.nan
    elif kind == "one_finite":
        d[:] = np.nan
        d[k] = 3.5
    return d


def _depth_images(cuda, d, shift, cmap):
    import generate_depth_maps as G

    n = d.size
    src = Guarded(n, torch.float32, cuda, shift=shift, data=torch.from_numpy(d))
    mm = Guarded(2, torch.int32, cuda)
    col, raw = Guarded(3 * n, torch.uint8, cuda), Guarded(n, torch.int16, cuda)
    ops.depth_to_image(src.t.view(1, n), colored=True, cmap=cmap, out=col.t.view(1, n, 3), scratch=mm.t)
    ops.depth_to_image(src.t.view(1, n), colored=False, out=raw.t.view(1, n), scratch=mm.t)
    (gc, c1), (gr, c2), (_, c3) = col.result(), raw.result(), mm.result(torch.ones(2, dtype=torch.bool))
    assert c1 == 0 and c2 == 0 and c3 == 0
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref_col = G.colorize_depth(d.reshape(1, n), cmap=cmap)
        ref_raw = G.raw_depth_u16(d.reshape(1, n))
    assert np.array_equal(gc.numpy().reshape(1, n, 3), ref_col), (n, shift, "colour")
    assert np.array_equal(gr.numpy().view(np.uint16).reshape(1, n), ref_raw), (n, shift, "raw")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", DEPTH_MAPS + ["plain"])
def test_depth_to_image_heads_tails_and_nonfinite(cuda, kind):
    """(1, n) views of n = 1, 3, 4, 5, 1023, 1025 at + 0, + 4 and + 12 B from a 16-B boundary (the scalar
    head and tail of the min / max pass) == colorize_depth / raw_depth_u16 byte for byte."""
    for n in (1, 3, 4, 5, 1023, 1025):
        for shift in (0, 1, 3):
            _depth_images(cuda, _depth_map(kind, n), shift, "turbo")


@pytest.mark.gpu
def test_depth_to_image_colormap_of_ten_entries(cuda):
    """tab10 has N = 10 (colormap_lut supplies it): trunc(v * N), N -> N - 1 and the bad entry N + 2."""
    lut, N = ops.colormap_lut("tab10", cuda)
    assert N == 10 and tuple(lut.shape) == (13, 3)
    for kind in ("plain", "one_finite", "negative"):
        _depth_images(cuda, _depth_map(kind, 1025), 1, "tab10")
    d = np.linspace(0.0, 1.0, 1001, dtype=np.float32)       # every boundary k / 10 of the table
    _depth_images(cuda, d, 0, "tab10")
