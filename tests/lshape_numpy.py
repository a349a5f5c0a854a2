"""numpy restatement of the L-shape split's specification (include/dp_mi355x.h, "L-shape split"): the
rectangle list and rules 1-10, one rectangle at a time, with a flood fill for the components.  Tests
compare the device against it; the golden fixture (tests/golden/golden_lshape.npz, made a second way
with scipy.ndimage and matplotlib) pins the restatement itself.  The minimum-area rectangle of rule 9
is rule 3 of "Cluster shapes", restated in shapes_numpy.  No code shared with the package.

Every fp64 operation is written out one at a time, so numpy rounds each on its own as the header asks.
"""

import math

import numpy as np

import shapes_numpy as SN

MAX_SIDE = 1024
CELL = 0.2
STATUS = ("split", "small", "few_points", "thin", "no_empty_region", "empty_ratio", "one_part", "few_parts",
          "area_ratio", "capacity")
INT_BIG = 2 ** 31 - 1


def rectangle_list(shapes):
    """The rectangle list (R, 8) of the (K, 16) shape table."""
    out = []
    for c, row in enumerate(np.asarray(shapes, dtype=np.float64).reshape(-1, 16)):
        if row[0] != 1.0:
            continue
        cu, cv, w, h, ang = (float(v) for v in row[2:7])
        if w * h > 100.0 and row[1] > 1000.0:
            a = ang * math.pi / 180.0
            ca, sa = math.cos(a), math.sin(a)
            if w > h:
                d = w / 4.0
                out.append([cu - d * ca, cv - d * sa, w / 2.0, h, ang, c, 1.0, 0.0])
                out.append([cu + d * ca, cv + d * sa, w / 2.0, h, ang, c, 1.0, 0.0])
            else:
                d = h / 4.0
                out.append([cu - d * sa, cv + d * ca, w, h / 2.0, ang, c, 1.0, 0.0])
                out.append([cu + d * sa, cv - d * ca, w, h / 2.0, ang, c, 1.0, 0.0])
        else:
            out.append([cu, cv, w, h, ang, c, 0.0, 0.0])
    return np.array(out, dtype=np.float64).reshape(-1, 8)


def grid_side(side):
    q = side / CELL
    return int(q) + 1 if -2.0e9 < q < 2.0e9 else INT_BIG


def rotated(uv, rect):
    """Rule 2: (x', y') of every point, and c, s."""
    cu, cv, _, _, ang = rect[:5]
    a = -ang * math.pi / 180.0
    c, s = math.cos(a), math.sin(a)
    du, dv = uv[:, 0] - cu, uv[:, 1] - cv
    return du * c - dv * s, du * s + dv * c, c, s


def components(mask):
    """4-connected components of a boolean grid by flood fill: (labels from 1 in row-major order of the
    first cell, 0 elsewhere; list of sizes)."""
    gh, gw = mask.shape
    lab = np.zeros((gh, gw), np.int64)
    sizes = []
    for y in range(gh):
        for x in range(gw):
            if not mask[y, x] or lab[y, x]:
                continue
            k = len(sizes) + 1
            lab[y, x] = k
            stack, n = [(y, x)], 0
            while stack:
                cy, cx = stack.pop()
                n += 1
                for ny, nx in ((cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)):
                    if 0 <= ny < gh and 0 <= nx < gw and mask[ny, nx] and not lab[ny, nx]:
                        lab[ny, nx] = k
                        stack.append((ny, nx))
            sizes.append(n)
    return lab, sizes


def split_one(rect, uv, grid_ok=True):
    """Rules 1-10 for one rectangle: (info row (8,), list of part rows (8,)); `grid_ok` False: rule 4's
    capacity is used up.  The trace of the grids rides along as a dict (for the fixture)."""
    cu, cv, w, h, ang = (float(v) for v in rect[:5])
    info = np.zeros(8)
    tr = {}
    if w * h < 10.0:
        info[0] = 1
        return info, [], tr
    xr, yr, c, s = rotated(uv, rect)
    hw, hh = w / 2.0, h / 2.0
    inside = (-hw < xr) & (xr < hw) & (-hh < yr) & (yr < hh)
    gw, gh = grid_side(w), grid_side(h)
    info[1], info[2], info[3] = inside.sum(), gw, gh
    tr["inside"] = inside
    if inside.sum() < 50:
        info[0] = 2
        return info, [], tr
    if gw <= 2 or gh <= 2:
        info[0] = 3
        return info, [], tr
    if gw > MAX_SIDE or gh > MAX_SIDE or not grid_ok:
        info[0], info[7] = 9, 1
        return info, [], tr
    gx = ((xr[inside] + hw) / CELL).astype(np.int64)
    gy = ((yr[inside] + hh) / CELL).astype(np.int64)
    ok = (gx >= 0) & (gx < gw) & (gy >= 0) & (gy < gh)
    b = np.zeros((gh, gw), bool)
    b[gy[ok], gx[ok]] = True
    d = b.copy()
    d[:, 1:] |= b[:, :-1]
    d[1:, :] |= b[:-1, :]
    d[1:, 1:] |= b[:-1, :-1]
    elab, esz = components(~d)
    big = [k + 1 for k, n in enumerate(esz) if n >= 6]
    empty_mask = np.isin(elab, big)
    tr.update(b=b, d=d, empty_mask=empty_mask)
    info[4] = empty_mask.sum()
    if not big:
        info[0] = 4
        return info, [], tr
    ratio = float(empty_mask.sum()) / float(gw * gh)
    if ratio < 0.2 or ratio > 0.6:
        info[0] = 5
        return info, [], tr
    olab, osz = components(~empty_mask)
    tr["olab"] = olab
    info[5] = len(osz)
    if len(osz) < 2:
        info[0] = 6
        return info, [], tr
    parts, area = [], 0.0
    for k, n in enumerate(osz):
        if n < 6:
            continue
        ys, xs = np.nonzero(olab == k + 1)
        p = np.c_[xs * CELL - hw, ys * CELL - hh]
        sx, sy, sw, sh, sa, _ = SN.min_area_rect(p[SN.hull(p)])
        if sw * sh > 1.0:
            parts.append(np.array([(sx * c - sy * s) + cu, (sx * s + sy * c) + cv, sw, sh, math.fmod(sa + ang, 180.0),
                                   rect[5], rect[6] + 2.0, 0.0]))
            area = area + sw * sh
    info[6] = len(parts)
    if len(parts) < 2:
        info[0] = 7
        return info, [], tr
    q = area / (w * h)
    if not (0.4 < q < 1.3):
        info[0] = 8
        return info, [], tr
    return info, parts, tr


def participants(points, labels):
    """points_2d of the reference: (u, v) of the rows with label >= -1."""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    keep = np.asarray(labels).reshape(-1) >= -1
    return np.c_[-P[keep, 0], P[keep, 2]]


def split_l_shapes(points, labels, rects, max_cells=1 << 20, max_out=None, trace=None):
    """(rects_out (rows, 8), (rows, error word), info (R, 8)) for the rectangle list `rects` (R, 8)."""
    rects = np.asarray(rects, dtype=np.float64).reshape(-1, 8)
    uv = participants(points, labels)
    out, info, used = [], np.zeros((len(rects), 8)), 0
    for r, rect in enumerate(rects):
        grid_ok = True
        w, h = float(rect[2]), float(rect[3])
        if not w * h < 10.0:
            gw, gh = grid_side(w), grid_side(h)
            if gw > 2 and gh > 2 and gw <= MAX_SIDE and gh <= MAX_SIDE:
                used += gw * gh                  # capacity goes in list order, whatever rule 3 says
                grid_ok = used <= max_cells
        info[r], parts, tr = split_one(rect, uv, grid_ok)
        if trace is not None:
            trace.append(tr)
        out.extend(parts if info[r, 0] == 0 else [rect.copy()])
    rows = len(out)
    if max_out is not None and rows > max_out:
        return np.array(out[:max_out]).reshape(-1, 8), (max_out, 1), info
    return np.array(out, dtype=np.float64).reshape(-1, 8), (rows, 0), info
