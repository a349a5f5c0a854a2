"""The shape overlays of DESIGN.md section 23, restated in numpy: the rule csrc/dp_overlay.hip follows (the numbered list
of include/dp_mi355x.h, "Shape overlays on the plan view"), in fp64 in the order written here, every product, sum and
quotient rounded on its own.  The GPU picture is compared with `draw` byte for byte and its counts exactly; its records
with `records`, where only cos and sin (the device's own) may differ in the last places.

    1. frame      u = -x, v = z; with a plan camera record (cx = [2], cz = [3], scale = [4], hw = [7], hh = [8])
                  X = (u - cx) * scale + hw, Y = hh - (v - cz) * scale; pixel (i, j) is the point (i, j); a camera that is
                  not a plan record, is degenerate or holds a non-finite value lists and draws nothing (error word 2)
    2. the list   the rectangles in list order, then the rows of the shapes table with kind 2, in table order, as circles;
                  rectangle i: record i, number i + 1, colour i mod 8 of the first palette; circle k: record nr + k, number
                  nr + k + 1, colour k mod 8 of the second
    3. skipped    a non-finite column, a negative w, h or r, or X, Y, a, b (R), ex, ey not finite: flags 8, nothing else
    4. rectangle  a = w * scale / 2, b = h * scale / 2, t = stroke / 2, c, s = cos, sin(angle * pi / 180); for a pixel
                  x' = dx * c - dy * s, y' = dx * s + dy * c; on the stroke iff |x'| <= a + t and |y'| <= b + t and not
                  (|x'| < a - t and |y'| < b - t); box: ex = |c| (a + t) + |s| (b + t), ey = |s| (a + t) + |c| (b + t),
                  floor(X - ex) .. ceil(X + ex), floor(Y - ey) .. ceil(Y + ey)
    5. circle     R = r * scale; on the stroke iff max(R - t, 0)^2 <= dx dx + dy dy <= (R + t)^2; box: floor(X - (R + t)) ..
                  ceil(X + (R + t)); a pixel outside a shape's box is not on its stroke
    6. blending   out = (A * c + (255 - A) * p + 127) // 255 per channel; per pixel every covering shape in list order
    7. labels     after all strokes, in the same order: a block of (6 n - 1) L x 7 L pixels for n digits, its corner at
                  floor(X + 0.5) - ((6 n - 1) L) // 2, floor(Y + 0.5) - (7 L) // 2; the block grown by L on every side is
                  blended white at 179, then the digits' pixels (FONT, 5 x 7, one column between digits, every font pixel
                  L x L) are set to the shape's colour; L = 0: no labels; a number above 9999: none, counted (flags 4)
    8. off-screen a shape whose stroke box and label box both miss the picture: counted, never drawn
"""

import numpy as np

RECT_PALETTE = ("#4285F4", "#34A853", "#FBBC05", "#EA4335", "#8E44AD", "#16A085", "#D35400", "#7F8C8D")
CIRCLE_PALETTE = ("#3498DB", "#2ECC71", "#F1C40F", "#E74C3C", "#9B59B6", "#1ABC9C", "#E67E22", "#95A5A6")
RECORD_DOUBLES = 20
# kind, flags, X, Y, a | R, b, cos, sin, colour, number, stroke box (4), label box (4), digits, 0
REAL_FIELDS = (2, 3, 4, 5, 6, 7)
BOX_FIELDS = tuple(range(10, 18))
INT_FIELDS = (0, 1, 8, 9, 18, 19)
F_STROKE, F_LABEL, F_DROPPED, F_SKIPPED = 1, 2, 4, 8
STATS = ("rectangles", "circles", "skipped", "offscreen", "labels_dropped", "pixels_painted", "error", "spare")
LABEL_ALPHA = 179
PI = 3.14159265358979323846
FONT = ((14, 17, 19, 21, 25, 17, 14), (4, 12, 4, 4, 4, 4, 14), (14, 17, 1, 2, 4, 8, 31), (31, 2, 4, 2, 1, 17, 14),
        (2, 6, 10, 18, 31, 2, 2), (31, 16, 30, 1, 1, 17, 14), (6, 8, 16, 30, 17, 17, 14), (31, 1, 2, 4, 8, 8, 8),
        (14, 17, 17, 14, 17, 17, 14), (14, 17, 17, 15, 1, 2, 12))


def palette(rect=RECT_PALETTE, circle=CIRCLE_PALETTE):
    """uint8 (16, 3): the rectangle palette, then the circle palette."""
    return np.array([[int(h[1:3], 16), int(h[3:5], 16), int(h[5:7], 16)] for h in tuple(rect) + tuple(circle)], np.uint8)


def plan_camera(cx, cz, scale, W, H, degenerate=0.0):
    """A plan camera record as dp_render_points writes it (kind 1)."""
    cam = np.zeros(24)
    cam[0], cam[1], cam[2], cam[3], cam[4] = 1.0, degenerate, cx, cz, scale
    cam[6], cam[7], cam[8] = np.nan, (np.float64(W) - 1.0) / 2.0, (np.float64(H) - 1.0) / 2.0
    return cam


def camera_ok(cam):
    cam = np.asarray(cam, np.float64)
    return bool(cam[0] == 1.0 and cam[1] == 0.0 and np.isfinite(cam[[2, 3, 4, 7, 8]]).all())


def _live(rows, n, width):
    rows = np.zeros((0, width)) if rows is None else np.asarray(rows, np.float64).reshape(-1, width)
    k = len(rows) if n is None else max(0, min(int(n), len(rows)))
    return rows[:k]


def digit_block(number, L):
    """bool ((7 L), (6 n - 1) L): the digits' pixels of a label."""
    ds = [int(ch) for ch in str(int(number))]
    cells = np.zeros((7, 6 * len(ds) - 1), bool)
    for k, d in enumerate(ds):
        for r in range(7):
            for c in range(5):
                cells[r, 6 * k + c] = bool((FONT[d][r] >> (4 - c)) & 1)
    return np.repeat(np.repeat(cells, L, axis=0), L, axis=1)


def records(camera, rects=None, n_rects=None, shapes=None, n_clusters=None, size=(1280, 720), stroke=3.0, label_scale=2,
            pal=None):
    """(records fp64 (nr + nc, 20), stats {name: int} without pixels_painted)."""
    W, H = size
    pal = palette() if pal is None else np.asarray(pal, np.uint8).reshape(16, 3)
    stats = {k: 0 for k in STATS}
    if not camera_ok(camera):
        stats["error"] = 2
        return np.zeros((0, RECORD_DOUBLES)), stats
    cam = np.asarray(camera, np.float64)
    cx, cz, scale, hw, hh = cam[2], cam[3], cam[4], cam[7], cam[8]
    R = _live(rects, n_rects, 8)
    T = _live(shapes, n_clusters, 16)
    C = T[T[:, 0] == 2.0]
    nr, L, t = len(R), int(label_scale), np.float64(stroke) / 2.0
    out = np.zeros((nr + len(C), RECORD_DOUBLES))
    wm, hm = np.float64(W - 1), np.float64(H - 1)
    for i in range(len(out)):
        o = out[i]
        rect = i < nr
        if rect:
            u, v, p0, p1, ang = R[i, :5]
            col = pal[i % 8]
        else:
            (u, v, p0), p1, ang = C[i - nr, 8:11], np.float64(0.0), np.float64(0.0)
            col = pal[8 + (i - nr) % 8]
        number = i + 1
        o[0], o[8], o[9] = 1.0 if rect else 2.0, float(int(col[0]) + 256 * int(col[1]) + 65536 * int(col[2])), float(number)
        o[12] = o[13] = o[16] = o[17] = -1.0
        skip = not np.isfinite([u, v, p0, p1, ang]).all() or p0 < 0.0 or p1 < 0.0
        X = Y = a = b = np.float64(0.0)
        c, s = np.float64(1.0), np.float64(0.0)
        if not skip:
            with np.errstate(all="ignore"):
                X = (u - cx) * scale + hw
                Y = hh - (v - cz) * scale
                if rect:
                    a, b = p0 * scale / 2.0, p1 * scale / 2.0
                    rad = ang * PI / 180.0
                    c, s = np.cos(rad), np.sin(rad)
                    ac, as_ = abs(c), abs(s)
                    ex, ey = ac * (a + t) + as_ * (b + t), as_ * (a + t) + ac * (b + t)
                else:
                    a = p0 * scale
                    ex = ey = a + t
            skip = not np.isfinite([X, Y, a, b, ex, ey]).all()
        if skip:
            o[1] = F_SKIPPED
            stats["skipped"] += 1
            stats["error"] |= 1
            continue
        with np.errstate(all="ignore"):
            x0, x1, y0, y1 = np.floor(X - ex), np.ceil(X + ex), np.floor(Y - ey), np.ceil(Y + ey)
        flags = F_STROKE if (x1 >= 0.0 and x0 <= wm and y1 >= 0.0 and y0 <= hm) else 0
        o[2:8] = X, Y, a, b, c, s
        o[10:14] = x0, y0, x1, y1
        if L > 0:
            if number > 9999:
                flags |= F_DROPPED
                stats["labels_dropped"] += 1
            else:
                nd = len(str(number))
                bw, bh = (6 * nd - 1) * L, 7 * L
                lx, ly = np.floor(X + 0.5) - float(bw // 2), np.floor(Y + 0.5) - float(bh // 2)
                l0, l1, l2, l3 = lx - float(L), ly - float(L), lx + float(bw - 1 + L), ly + float(bh - 1 + L)
                if l2 >= 0.0 and l0 <= wm and l3 >= 0.0 and l1 <= hm:
                    flags |= F_LABEL
                o[14:18] = l0, l1, l2, l3
                o[18] = float(nd)
        o[1] = float(flags)
        stats["offscreen" if not flags & (F_STROKE | F_LABEL) else ("rectangles" if rect else "circles")] += 1
    return out, stats


def blend(p, c, A):
    """out = (A * c + (255 - A) * p + 127) // 255 on integers (arrays or scalars)."""
    return (int(A) * np.asarray(c, np.int64) + (255 - int(A)) * np.asarray(p, np.int64) + 127) // 255


def _clip(lo, hi, last):
    """The integer range [lo, hi] of a box's side cut to [0, last]; empty: (0, -1)."""
    lo, hi = max(lo, 0.0), min(hi, float(last))
    return (int(lo), int(hi)) if lo <= hi else (0, -1)


def draw(image, recs, stroke=3.0, alpha=230, label_scale=2):
    """(the picture with the records drawn on a copy of `image` (H, W, 3) uint8, pixels painted)."""
    img = np.array(image, np.uint8).astype(np.int64)
    H, W = img.shape[:2]
    recs = np.asarray(recs, np.float64).reshape(-1, RECORD_DOUBLES)
    t, L, A = np.float64(stroke) / 2.0, int(label_scale), int(alpha)
    hit = np.zeros((H, W), bool)
    for o in recs:
        if not int(o[1]) & F_STROKE:
            continue
        (i0, i1), (j0, j1) = _clip(o[10], o[12], W - 1), _clip(o[11], o[13], H - 1)
        if i0 > i1 or j0 > j1:
            continue
        X, Y, a, b, c, s = o[2:8]
        dx = (np.arange(i0, i1 + 1, dtype=np.float64) - X)[None, :]
        dy = (np.arange(j0, j1 + 1, dtype=np.float64) - Y)[:, None]
        if o[0] == 1.0:
            xr, yr = np.abs(dx * c - dy * s), np.abs(dx * s + dy * c)
            on = (xr <= a + t) & (yr <= b + t) & ~((xr < a - t) & (yr < b - t))
        else:
            d2 = dx * dx + dy * dy
            lo = max(a - t, 0.0)
            on = (lo * lo <= d2) & (d2 <= (a + t) * (a + t))
        col = np.array([int(o[8]) & 255, (int(o[8]) >> 8) & 255, (int(o[8]) >> 16) & 255], np.int64)
        view = img[j0:j1 + 1, i0:i1 + 1]
        view[on] = blend(view[on], col, A)
        hit[j0:j1 + 1, i0:i1 + 1] |= on
    for o in recs:
        if L <= 0 or not int(o[1]) & F_LABEL:
            continue
        (i0, i1), (j0, j1) = _clip(o[14], o[16], W - 1), _clip(o[15], o[17], H - 1)
        if i0 > i1 or j0 > j1:
            continue
        img[j0:j1 + 1, i0:i1 + 1] = blend(img[j0:j1 + 1, i0:i1 + 1], 255, LABEL_ALPHA)
        hit[j0:j1 + 1, i0:i1 + 1] = True
        block = digit_block(int(o[9]), L)
        lx, ly = int(o[14]) + L, int(o[15]) + L
        col = np.array([int(o[8]) & 255, (int(o[8]) >> 8) & 255, (int(o[8]) >> 16) & 255], np.int64)
        oy, ox = np.nonzero(block)
        i, j = lx + ox, ly + oy
        ok = (i >= 0) & (i < W) & (j >= 0) & (j < H)
        img[j[ok], i[ok]] = col
    return img.astype(np.uint8), int(hit.sum())


def draw_shapes(image, camera, rects=None, n_rects=None, shapes=None, n_clusters=None, stroke=3.0, alpha=230, label_scale=2,
                pal=None):
    """What depth_pro.overlay.draw_shapes returns, on the host: {"image", "records", "stats" {name: int}}."""
    H, W = np.asarray(image).shape[:2]
    recs, stats = records(camera, rects, n_rects, shapes, n_clusters, (W, H), stroke, label_scale, pal)
    img, painted = draw(image, recs, stroke, alpha, label_scale)
    stats["pixels_painted"] = painted
    return {"image": img, "records": recs, "stats": stats}


def stats_of(recs, painted, degenerate=False):
    """The counts that follow from a list of records (the device's own, say) and the painted pixels."""
    recs = np.asarray(recs, np.float64).reshape(-1, RECORD_DOUBLES)
    fl = recs[:, 1].astype(np.int64)
    drawn = (fl & (F_STROKE | F_LABEL)) != 0
    skipped = (fl & F_SKIPPED) != 0
    return {"rectangles": int((drawn & (recs[:, 0] == 1.0)).sum()), "circles": int((drawn & (recs[:, 0] == 2.0)).sum()),
            "skipped": int(skipped.sum()), "offscreen": int((~drawn & ~skipped).sum()),
            "labels_dropped": int(((fl & F_DROPPED) != 0).sum()), "pixels_painted": int(painted),
            "error": 2 if degenerate else int(skipped.any()), "spare": 0}
