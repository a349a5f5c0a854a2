"""The depth-warped views restated in numpy: the rules of include/dp_mi355x.h ("Depth-warped views"), written from
those rules -- the parallax frames and the anaglyph of the reference's OLD_SCRIPTS/depth_video_effect.py.

Every array step follows NumPy >= 2 promotion as the reference's expressions do (a Python float is weak: `dx * f32`
stays float32; an np.float64 scalar is not: `np.float64 * f32` is float64).  The sampler is OpenCV 4.x's published
fixed-point rule for cv2.remap(INTER_LINEAR) on 8-bit pixels in integers; `make_golden_effects.py` checks it against
scipy.ndimage.map_coordinates.  Two forms of every view are here: `literal=True` hands the maps to the sampler
transposed, as the reference does (a (W, H) picture), `literal=False` is what the GPU builds; for any input
`literal.transpose(1, 0, 2) == ours`.
"""

import numpy as np

SHIFT, SHIFT_F32, ZOOM = 0, 1, 2


def scene(H, W, seed=0):
    """A test frame: random RGB (uint8 (H, W, 3)) and a random depth in [1, 5) m with a step edge to 8 m across the
    right part of the lower half (float32 (H, W))."""
    rng = np.random.default_rng(seed)
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    depth = rng.uniform(1.0, 5.0, (H, W)).astype(np.float32)
    depth[H // 2:, W // 3:] += np.float32(3.0)
    return image, depth


def normalise(depth):
    """(depth - min) / (max - min) in float32, min and max over the finite values (all of them in the reference)."""
    depth = np.asarray(depth, np.float32)
    fin = depth[np.isfinite(depth)]
    if fin.size == 0:
        return np.full(depth.shape, np.nan, np.float32)
    lo, hi = fin.min(), fin.max()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (depth - lo) / (hi - lo)


def view_params(motion, amplitude, W, H, frame, total_frames):
    """(kind, a, b) of one parallax frame, the reference's host arithmetic (np.float64 scalars)."""
    t = 2 * np.pi * frame / total_frames
    if motion == "circle":
        return SHIFT, amplitude * W * np.cos(t), amplitude * H * np.sin(t)
    if motion == "zoom":
        return ZOOM, 1 - (1.0 + amplitude * np.sin(t)), 0.0
    if motion == "swing":
        return SHIFT, amplitude * W * np.sin(t), 0.0
    raise ValueError(f"Unknown motion type: {motion}")


def maps(depth, view):
    """(map_x, map_y) float64 (H, W), not clipped yet, of one view (kind, a, b)."""
    kind, a, b = view
    H, W = np.asarray(depth).shape
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        if kind == ZOOM:
            a = np.float64(a)
            return x + a * (x - W / 2), y + a * (y - H / 2)
        om = 1 - normalise(depth)                                     # float32
        if kind == SHIFT:
            return x + np.float64(a) * om, y + np.float64(b) * om     # float64 * float32 -> float64
        if kind == SHIFT_F32:
            return x + float(a) * om, y.astype(np.float64)            # Python float * float32 -> float32; int64 + f32 -> f64
    raise ValueError(f"unknown kind {kind}")


def remap_linear_u8(src, map_x, map_y):
    """cv2.remap(src, map_x, map_y, INTER_LINEAR) for uint8 (H, W, C) `src` and float32 maps of any common shape whose
    values lie inside the image: coordinates rounded half-even to 1/32, weights 32 (32 - fx | fx)(32 - fy | fy) (their
    sum is 32768), (sum + 16384) >> 15; a tap outside the image counts as 0."""
    assert map_x.dtype == np.float32 and map_y.dtype == np.float32 and src.dtype == np.uint8
    H, W = src.shape[:2]
    sx = np.rint(map_x * np.float32(32)).astype(np.int64)
    sy = np.rint(map_y * np.float32(32)).astype(np.int64)
    ix, fx, iy, fy = sx >> 5, sx & 31, sy >> 5, sy & 31
    pad = np.zeros((H + 1, W + 1) + src.shape[2:], np.int64)
    pad[:H, :W] = src
    acc = np.zeros(map_x.shape + src.shape[2:], np.int64)
    for dy, wy in ((0, 32 - fy), (1, fy)):
        for dx, wx in ((0, 32 - fx), (1, fx)):
            acc += (32 * wx * wy)[..., None] * pad[iy + dy, ix + dx]
    return ((acc + 16384) >> 15).astype(np.uint8)


def warp_view(image, depth, view, literal=False):
    """One view: (picture, number of bad pixels).  literal=False: out[y][x] = sample(map[y][x]), (H, W, 3), a pixel whose
    map coordinate is not finite black and counted.  literal=True: the reference's call on the transposed maps, a
    (W, H, 3) picture (finite depth only)."""
    H, W = depth.shape
    mx, my = maps(depth, view)
    bad = ~(np.isfinite(mx) & np.isfinite(my))
    mx = np.clip(np.where(bad, 0.0, mx), 0, W - 1).astype(np.float32)
    my = np.clip(np.where(bad, 0.0, my), 0, H - 1).astype(np.float32)
    if literal:
        assert not bad.any()
        return remap_linear_u8(image, mx.T, my.T), 0
    out = remap_linear_u8(image, mx, my)
    out[bad] = 0
    return out, int(bad.sum())


def warp_views(image, depth, views):
    """(uint8 (V, H, W, 3), int64 (V,)) of several views."""
    res = [warp_view(image, depth, v) for v in views]
    return np.stack([r[0] for r in res]), np.array([r[1] for r in res], np.int64)


def anaglyph(image, depth, separation, literal=False):
    """Red from the left view (+separation * W), green and blue from the right (-); (picture, bad pixels)."""
    W = depth.shape[1]
    dx = separation * W
    left, bad = warp_view(image, depth, (SHIFT_F32, dx, 0.0), literal)
    right, bad_r = warp_view(image, depth, (SHIFT_F32, -dx, 0.0), literal)
    assert bad == bad_r
    out = np.zeros_like(left)
    out[..., 0] = left[..., 0]
    out[..., 1] = right[..., 1]
    out[..., 2] = right[..., 2]
    return out, bad
