"""The point-cloud views of DESIGN.md section 22, restated in numpy: the rule csrc/dp_render.hip follows, in fp64 in
the order written here (every product, sum, quotient and square root rounded on its own).  The GPU result is compared
with this byte for byte: pictures, camera records and counts.

A view is `(front, up, zoom)` (the reference's Open3D presets, `VIEW_PRESETS`) or the string "plan" (the main
pipeline's top-down picture).  `render_views` returns what `depth_pro.render.render_views` returns, on the host."""

import math

import numpy as np

VIEW_PRESETS = {
    "front": ((0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 0.4),
    "top": ((0.0, 1.0, 0.0), (0.0, 0.0, -1.0), 0.4),         # the reference has [0, -1, 0]: the eye under a y-up cloud
    "side": ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.4),
    "isometric": ((1.0, -1.0, -1.0), (0.0, 1.0, 0.0), 0.35),
}
SHEET = ("front", "top", "isometric", "side")       # top-left, top-right, bottom-left, bottom-right
TAN_HALF_FOV = math.tan(math.radians(30.0))
BACKGROUND, PLAN_BACKGROUND, GREY = (255, 255, 255), (240, 240, 240), (128, 128, 128)
MAX_VIEWS, MAX_SIZE = 4, 15
CAMERA_DOUBLES = 24
# a camera record: kind (0 perspective, 1 plan), degenerate, then
#   perspective: eye 2:5, s 5:8, u 8:11, F 11:14, near, far, dist, extent, centre 18:21, t * (W / H), t, 0
#   plan:        centre x', centre z, scale, y_top, min_height (NaN: none), (W - 1) / 2, (H - 1) / 2, zeros
GLOBAL_STATS = ("live", "nonfinite", "degenerate", "error")
VIEW_STATS = ("drawn", "clipped", "outside", "covered_pixels")
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _view(v):
    return v if isinstance(v, str) and v == "plan" else (VIEW_PRESETS[v] if isinstance(v, str) else v)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], np.float64)


def _norm(a):
    return np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])


def _dot(a, q):
    """a . q for every row of q, summed left to right."""
    return a[0] * q[:, 0] + a[1] * q[:, 1] + a[2] * q[:, 2]


def live_rows(points, count=None):
    """(the live rows, the mask of the finite ones)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    n = len(p) if count is None else max(0, min(int(count), len(p)))
    p = p[:n]
    return p, np.isfinite(p).all(axis=1)


def perspective_camera(p, fin, view, W, H):
    front, up, zoom = (np.asarray(view[0], np.float64), np.asarray(view[1], np.float64), np.float64(view[2]))
    cam = np.zeros(CAMERA_DOUBLES)
    t = np.float64(TAN_HALF_FOV)
    cam[21], cam[22] = t * (np.float64(W) / np.float64(H)), t
    if not fin.any():
        cam[1] = 1.0
        return cam
    mn, mx = p[fin].min(axis=0) + 0.0, p[fin].max(axis=0) + 0.0        # -0 counts as +0 in every bound
    center = (mn + mx) / 2.0
    extent = (mx - mn).max()
    cam[17], cam[18:21] = extent, center
    if not extent > 0.0:                                       # 0, or not comparable (an overflow): nothing divides by it
        cam[1] = 1.0
        return cam
    f = front / _norm(front)
    dist = zoom * extent / t
    eye = center + f * dist
    F = -f
    s = _cross(F, up)
    s = s / _norm(s)
    u = _cross(s, F)
    near = max(0.01 * extent, dist - 3.0 * extent)
    far = dist + 3.0 * extent
    cam[2:5], cam[5:8], cam[8:11], cam[11:14] = eye, s, u, F
    cam[14], cam[15], cam[16] = near, far, dist
    return cam


def plan_camera(p, fin, min_height, W, H):
    cam = np.zeros(CAMERA_DOUBLES)
    cam[0] = 1.0
    cam[6] = np.nan if min_height is None else np.float64(min_height)
    cam[7], cam[8] = (np.float64(W) - 1.0) / 2.0, (np.float64(H) - 1.0) / 2.0
    shown = fin if min_height is None else fin & (p[:, 1] >= np.float64(min_height))
    if not shown.any():
        cam[1] = 1.0
        return cam, shown
    q = p[shown]
    x = -q[:, 0]
    x0, x1, z0, z1 = x.min() + 0.0, x.max() + 0.0, q[:, 2].min() + 0.0, q[:, 2].max() + 0.0
    span_x, span_z = x1 - x0, z1 - z0
    span_x = 1.0 if span_x == 0.0 else span_x
    span_z = 1.0 if span_z == 0.0 else span_z
    cam[2], cam[3] = (x0 + x1) / 2.0, (z0 + z1) / 2.0
    cam[4] = min((np.float64(W) - 1.0) / span_x, (np.float64(H) - 1.0) / span_z)
    cam[5] = q[:, 1].max() + 0.0
    return cam, shown


def _project(p, fin, cam, W, H, size, shown=None):
    """Per live row: (ok, px, py, depth as float32); and the counts drawn, clipped, outside."""
    n, R = len(p), (size - 1) // 2
    ok = np.zeros(n, bool)
    px, py = np.zeros(n, np.int64), np.zeros(n, np.int64)
    depth = np.zeros(n, np.float32)
    if cam[1] != 0.0:
        return ok, px, py, depth, (0, 0, 0)
    with np.errstate(all="ignore"):
        if cam[0] == 0.0:
            q = p - cam[2:5]
            xc, yc, w = _dot(cam[5:8], q), _dot(cam[8:11], q), _dot(cam[11:14], q)
            inside = fin & (w >= cam[14]) & (w <= cam[15])
            clipped = int((fin & ~inside).sum())
            dy = w * cam[22]
            dx = dy * (np.float64(W) / np.float64(H))
            ndc_x, ndc_y = xc / dx, yc / dy
            fx = np.floor((ndc_x * 0.5 + 0.5) * np.float64(W))
            fy = np.floor((0.5 - ndc_y * 0.5) * np.float64(H))
            d = w
        else:
            inside = shown
            clipped = int((fin & ~shown).sum())
            fx = np.floor(((-p[:, 0]) - cam[2]) * cam[4] + cam[7] + 0.5)
            fy = np.floor(cam[8] - (p[:, 2] - cam[3]) * cam[4] + 0.5)
            d = cam[5] - p[:, 1]
        reach = inside & (fx >= -R) & (fx <= W - 1 + R) & (fy >= -R) & (fy <= H - 1 + R)
    outside = int((inside & ~reach).sum())
    ok = reach
    px[ok], py[ok] = fx[ok].astype(np.int64), fy[ok].astype(np.int64)
    with np.errstate(all="ignore"):
        depth[ok] = d[ok].astype(np.float32)
    return ok, px, py, depth, (int(ok.sum()), clipped, outside)


def centre_pixels(points, view, W, H, count=None, min_height=None):
    """(ok, px, py) of every live row for one view, splat size 1 (what the independent camera is compared with)."""
    p, fin = live_rows(points, count)
    v = _view(view)
    if v == "plan":
        cam, shown = plan_camera(p, fin, min_height, W, H)
        return _project(p, fin, cam, W, H, 1, shown)[:3]
    return _project(p, fin, perspective_camera(p, fin, v, W, H), W, H, 1)[:3]


def _picture(ok, px, py, depth, colors, W, H, size, background):
    """The z-buffered splats of one view: the smallest (float32 depth, row) of the size x size window per pixel."""
    R = (size - 1) // 2
    buf = np.full((H + size - 1, W + size - 1), EMPTY, np.uint64)
    rows = np.nonzero(ok)[0]
    keys = (depth[rows].view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)
    np.minimum.at(buf, (py[rows] + R, px[rows] + R), keys)
    best = np.full((H, W), EMPTY, np.uint64)
    for dy in range(size):
        for dx in range(size):
            np.minimum(best, buf[dy:dy + H, dx:dx + W], out=best)
    hit = best != EMPTY
    img = np.empty((H, W, 3), np.uint8)
    img[:] = np.asarray(background, np.uint8)
    win = (best[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    img[hit] = np.asarray(GREY, np.uint8) if colors is None else np.asarray(colors, np.uint8).reshape(-1, 3)[win]
    return img, int(hit.sum())


def render_views(points, colors=None, views=("front",), size=(1280, 720), point_size=7, background=BACKGROUND, count=None,
                 sheet=False, min_height=None):
    """{"image": uint8 (V, H, W, 3), or (2H, 2W, 3) with sheet=True; "cameras": fp64 (V, 24); "stats": {name: int} with
    the per-view entries as lists}.  The perspective views come first, in the order given, the plan last."""
    W, H = size
    p, fin = live_rows(points, count)
    vs = [_view(v) for v in views]
    persp = [v for v in vs if v != "plan"]
    order = persp + (["plan"] if len(persp) < len(vs) else [])
    cams, imgs, per = [], [], {k: [] for k in VIEW_STATS}
    for v in order:
        if v == "plan":
            cam, shown = plan_camera(p, fin, min_height, W, H)
            ok, px, py, depth, counts = _project(p, fin, cam, W, H, point_size, shown)
            bg = PLAN_BACKGROUND
        else:
            cam = perspective_camera(p, fin, v, W, H)
            ok, px, py, depth, counts = _project(p, fin, cam, W, H, point_size)
            bg = background
        img, covered = _picture(ok, px, py, depth, colors, W, H, point_size, bg)
        cams.append(cam)
        imgs.append(img)
        for k, c in zip(VIEW_STATS, counts + (covered,)):
            per[k].append(c)
    image = np.stack(imgs)
    if sheet:
        image = np.concatenate([np.concatenate([image[0], image[1]], axis=1), np.concatenate([image[2], image[3]], axis=1)], axis=0)
    ext = (p[fin].max(axis=0) - p[fin].min(axis=0)).max() if fin.any() else 0.0
    stats = {"live": len(p), "nonfinite": int((~fin).sum()), "degenerate": int(not ext > 0.0), "error": int((~fin).any()), **per}
    return {"image": image, "cameras": np.stack(cams), "stats": stats}


def scene(n, seed, box=True):
    """A box on a floor with a wall behind, n rows with colours: (points fp64 (n, 3), colours uint8 (n, 3))."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 3, n)
    u, v = rng.random(n), rng.random(n)
    floor = np.stack([4.0 * u - 2.0, 0.02 * v, 3.0 * v + 1.0], axis=1)
    wall = np.stack([4.0 * u - 2.0, 2.5 * v, np.full(n, 4.0) + 0.01 * u], axis=1)
    face = rng.integers(0, 3, n)
    bx = np.stack([np.where(face == 0, 0.0, u) * 0.8 - 0.4, np.where(face == 1, 1.0, v) * 1.2, np.where(face == 2, 0.0, u * v) * 0.8 + 2.0], axis=1)
    pts = np.where((k == 0)[:, None], floor, np.where((k == 1)[:, None], wall, bx if box else floor))
    return np.ascontiguousarray(pts, np.float64), rng.integers(0, 256, (n, 3), dtype=np.uint8)
