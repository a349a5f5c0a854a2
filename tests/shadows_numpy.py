"""Restatement of the depth-shadow rules of include/dp_mi355x.h ("Depth shadows"; csrc/dp_shadows.hip), written for
this project: the reference's find_depth_shadows as four steps on scipy.ndimage (`find_depth_shadows`), the same Sobel
in pure NumPy in scipy's accumulation order (`sobel_numpy`; `sobel_left_to_right` is the order that is NOT scipy's), a
pure-NumPy 4-connected size filter (`small_region_mask_numpy`), the ground fill in fp64 (`fill_ground_shadows`), and the
synthetic frames the tests and tools/shadows_bench.py share."""

import numpy as np

STATS = ("edge", "shadow", "components", "kept", "largest", "gmax", "nonfinite", "error", "shadow_nonpositive")


# ---------------------------------------------------------------------------------------------- gradient

def _taps(a, axis):
    """(left, centre, right) along `axis` with scipy's mode='reflect': beyond an edge, the edge sample again."""
    n = a.shape[axis]
    idx = np.arange(n)
    return (np.take(a, np.maximum(idx - 1, 0), axis), a, np.take(a, np.minimum(idx + 1, n - 1), axis))


def _pass(a, axis, centre, outer, sign):
    """One 1-D pass of scipy's correlate1d on three taps: fp64, the centre tap times its weight first, then
    (left + sign * right) * outer added to it; rounded to float32 once."""
    l, c, r = (t.astype(np.float64) for t in _taps(a, axis))
    t = c * centre
    t = t + (l + r if sign > 0 else l - r) * outer
    return t.astype(np.float32)


def sobel_numpy(d, axis):
    """scipy.ndimage.sobel(d, axis) for a float32 (H, W) array, bit for bit."""
    out = _pass(np.asarray(d, np.float32), axis, 0.0, -1.0, -1)          # [-1, 0, 1]: 0 c + (l - r) * -1
    return _pass(out, 1 - axis, 2.0, 1.0, +1)                             # [1, 2, 1]:  2 c + (l + r) * 1


def sobel_left_to_right(d, axis):
    """The same filter summed as w0 a + w1 b + w2 c: differs from scipy once the inputs span enough binades."""
    def run(a, ax, w):
        l, c, r = (t.astype(np.float64) for t in _taps(a, ax))
        return ((w[0] * l + w[1] * c) + w[2] * r).astype(np.float32)
    return run(run(np.asarray(d, np.float32), axis, (-1.0, 0.0, 1.0)), 1 - axis, (1.0, 2.0, 1.0))


def gradient_magnitude(d, sobel=None):
    """np.sqrt(dx**2 + dy**2) in float32, each operation rounded on its own."""
    if sobel is None:
        from scipy import ndimage
        sobel = ndimage.sobel
    with np.errstate(all="ignore"):
        dx, dy = sobel(d, 1), sobel(d, 0)
        assert dx.dtype == np.float32
        return np.sqrt(dx ** 2 + dy ** 2)


def edge_mask(d, threshold_factor=0.2, sobel=None):
    """(edge bool, gmax float32, nonfinite).  A frame with a non-finite depth has no edges (the project's definition)."""
    d = np.asarray(d, np.float32)
    g = gradient_magnitude(d, sobel)
    nonfinite = int((~np.isfinite(d)).sum())
    gmax = g.max()
    if nonfinite:
        return np.zeros(d.shape, bool), gmax, nonfinite
    if gmax > 0:
        g = g / gmax
    return g > threshold_factor, gmax, nonfinite          # NumPy >= 2: a Python float compares in float32


# ---------------------------------------------------------------------------------------------- regions

def region_sizes(free):
    """(labels, sizes) of the 4-connected components of `free` with scipy (the default cross structure)."""
    from scipy import ndimage

    labels, n = ndimage.label(np.asarray(free, bool))
    return labels, np.bincount(labels.ravel(), minlength=n + 1)


def small_region_mask(free, min_region_size=100):
    """(mask bool, counts): 1 where not free or in a free component of fewer than min_region_size pixels -- the
    reference's ~np.isin(labels, valid_regions)."""
    free = np.asarray(free, bool)
    labels, sizes = region_sizes(free)
    keep = sizes >= min_region_size
    keep[0] = False
    mask = ~keep[labels]
    counts = {"edge": int((~free).sum()), "shadow": int(mask.sum()), "components": int(len(sizes) - 1),
              "kept": int(keep.sum()), "largest": int(sizes[1:].max()) if len(sizes) > 1 else 0}
    return mask, counts


def small_region_mask_numpy(free, min_region_size=100):
    """The same mask without scipy: every free pixel takes the smallest flat index among itself and its four free
    neighbours, then pointer jumping, until nothing changes; a component's size is the count of its root."""
    free = np.asarray(free, bool)
    h, w = free.shape
    n = h * w
    lab = np.where(free, np.arange(n).reshape(h, w), n)
    while True:
        m = lab.copy()
        m[1:] = np.minimum(m[1:], np.where(free[1:], lab[:-1], n))
        m[:-1] = np.minimum(m[:-1], np.where(free[:-1], lab[1:], n))
        m[:, 1:] = np.minimum(m[:, 1:], np.where(free[:, 1:], lab[:, :-1], n))
        m[:, :-1] = np.minimum(m[:, :-1], np.where(free[:, :-1], lab[:, 1:], n))
        flat = np.append(m.ravel(), n)
        for _ in range(8):
            flat = flat[flat]
        m = flat[:n].reshape(h, w)
        if np.array_equal(m, lab):
            break
        lab = m
    sizes = np.bincount(lab.ravel(), minlength=n + 1)
    sizes[n] = 0
    return ~free | (sizes[lab] < min_region_size)


def find_depth_shadows(depth, threshold_factor=0.2, min_region_size=100):
    """The four steps (gradient, normalisation, threshold, labelling + size filter): (mask bool, stats dict)."""
    depth = np.asarray(depth, np.float32)
    edge, gmax, nonfinite = edge_mask(depth, threshold_factor)
    mask, counts = small_region_mask(~edge, min_region_size)
    with np.errstate(invalid="ignore"):
        nonpos = int((mask & (depth <= 0)).sum())
    return mask, {**counts, "gmax": float(gmax), "nonfinite": nonfinite, "error": int(nonfinite > 0), "shadow_nonpositive": nonpos}


# ---------------------------------------------------------------------------------------------- ground fill

def fill_ground_shadows(depth, shadow, normal, d, ground_rows=0.7):
    """The reference's interpolation for shadow pixels of the rows >= int(ground_rows * h), fp64 in its order."""
    depth = np.asarray(depth, np.float32)
    h, w = depth.shape
    out = depth.copy()
    ground = np.zeros((h, w), bool)
    ground[min(max(int(ground_rows * h), 0), h):] = True
    pts = np.where((np.asarray(shadow) != 0).ravel() & ground.ravel())[0]
    if len(pts) == 0:
        return out
    yi, xi = pts // w, pts % w
    cx, cy = w / 2, h / 2
    f = max(w, h)
    one = np.ones_like(xi, dtype=float)
    x = (xi - cx) * one / f
    y = (yi - cy) * one / f
    normal = [float(c) for c in normal]
    d = float(d)
    with np.errstate(all="ignore"):
        if abs(normal[2]) > 1e-6:
            z = (-normal[0] * x - normal[1] * y - d) / normal[2]
        elif abs(normal[0]) > 1e-6:
            raise ValueError("x-aligned ground normal: the reference's depth search is not built")
        else:
            plane_y = -d / normal[1]
            den = yi - cy
            den[np.abs(den) < 1e-6] = 1e-6
            z = plane_y * f / den
        z = np.maximum(z, 0.1)
        out.flat[pts] = z
    return out


# ---------------------------------------------------------------------------------------------- frames

def wide_field(h, w, seed):
    """float32 values spread over 2^-40 ... 2^40 with random signs: where the summation order of a pass shows."""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], (h, w)) * rng.uniform(1, 2, (h, w)) * 2.0 ** rng.integers(-40, 41, (h, w))).astype(np.float32)


def scene(h, w, seed, noise=0.0):
    """Boxes at different depths on a ramp (a floor receding towards the top of the frame), float32 in about 1...12."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    d = (12.0 - 10.0 * yy / max(h - 1, 1) + 0.5 * xx / max(w - 1, 1)).astype(np.float64)
    for _ in range(6 + (h * w) // 40000):
        bh, bw = int(rng.integers(max(h // 12, 2), max(h // 3, 3))), int(rng.integers(max(w // 12, 2), max(w // 3, 3)))
        y0, x0 = int(rng.integers(0, max(h - bh, 1))), int(rng.integers(0, max(w - bw, 1)))
        d[y0:y0 + bh, x0:x0 + bw] = rng.uniform(1.0, 8.0) + 0.01 * (xx[y0:y0 + bh, x0:x0 + bw] - x0) / bw
    if noise:
        d += rng.normal(0, noise, (h, w))
    return d.astype(np.float32)


def blobs(h, w, seed, density=0.62):
    """A random free mask with structure at several scales: one giant component and thousands of slivers."""
    rng = np.random.default_rng(seed)
    f = rng.random((h, w))
    for s in (4, 16):
        c = rng.random((h // s + 2, w // s + 2))
        f = f + np.kron(c, np.ones((s, s)))[:h, :w]
    return (f < np.quantile(f, density)).astype(np.uint8)


def spiral(h, w):
    """A one-pixel-wide free spiral that fills the frame: walls and corridor alternate, one component."""
    free = np.zeros((h, w), np.uint8)
    y0, x0, y1, x1 = 0, 0, h - 1, w - 1
    free[0, :] = 1
    while True:
        free[y0:y1 + 1, x1] = 1                     # down the right side
        free[y1, x0:x1 + 1] = 1                     # along the bottom to the left
        y0 += 2
        if y0 > y1:
            break
        free[y0:y1 + 1, x0] = 1                     # up the left side
        x1 -= 2
        y1 -= 2
        if x0 > x1 or y0 > y1:
            break
        free[y0, x0:x1 + 1] = 1                     # along the top to the right
        x0 += 2
        if x0 > x1:
            break
    return free


def comb(h, w):
    """Teeth on every other column that join only along the last row."""
    free = np.zeros((h, w), np.uint8)
    free[:, ::2] = 1
    free[h - 1, :] = 1
    return free
