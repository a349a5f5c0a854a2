"""Sequential numpy restatement of "Height-sliced floor plan" (include/dp_mi355x.h, rules R1-R4, C1-C2, M1-M2 and the
two simplification parameters), written from the header.  It composes tests/floorplan_numpy.py (raster, morphology,
labels, regions) and tests/outline_numpy.py (outlines, Douglas-Peucker, validity, snap, the file's coordinates); no code
is shared with the package.  tests/test_slices.py pins it to numpy's literal masks, to the reference's float formula for
the closing size and to scipy.ndimage.label.
"""

import math

import numpy as np

import floorplan_numpy as FN
import outline_numpy as ON

SLICE_MAX = 32
STATUS = ("ok", "too_few_points", "too_large")
DROP_REASONS = ("kept", "too_small", "fewer_than_3_vertices", "invalid", "overflow")
REGION_STATS = ("set_cells", "regions", "rows", "overflow", "height", "width", "reserved0", "reserved1")
OUTLINE_STATS = ("regions", "rows", "vertices", "vertices_written", "vertex_overflow", "region_overflow", "height", "width")
POLYGON_STATS = ("rows", "polygons", "vertices", "vertices_written", "overflow", "too_small", "too_few", "invalid")


def bounds(height_min, height_max, num_slices):
    """R1: (S, 3) = lo, hi, mid, every operation an fp64 operation of its own."""
    h = (float(height_max) - float(height_min)) / num_slices
    out = np.zeros((num_slices, 3))
    for s in range(num_slices):
        lo = float(height_min) + s * h
        hi = lo + h
        out[s] = (lo, hi, (lo + hi) / 2)
    return out


def masks(points, b):
    """R2: one boolean row mask per slice; each slice's two comparisons on their own."""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    fin = np.isfinite(pts).all(axis=1)
    out = []
    for lo, hi, _ in b:
        m = np.zeros(len(pts), bool)
        for i in range(len(pts)):
            m[i] = bool(fin[i]) and pts[i, 1] >= lo and pts[i, 1] < hi
        out.append(m)
    return out


def slice_grids(points, count=None, height_min=0.1, height_max=2.5, num_slices=5, resolution=0.05, padding=0.5, min_points=10,
                max_cells=1 << 20):
    """R1-R4: {"bounds", "stats" (S, 8), "dims" (S, 2), "origin" (S, 2), "grids": per slice floorplan_numpy's dict}."""
    pts = np.asarray(points, np.float64).reshape(-1, 3)[:count]
    b = bounds(height_min, height_max, num_slices)
    stats, dims, origin, grids = np.zeros((num_slices, 8)), np.zeros((num_slices, 2), np.int32), np.zeros((num_slices, 2)), []
    for s, m in enumerate(masks(pts, b)):
        n = int(m.sum())
        stats[s, 0] = n
        if n == 0 or n < min_points:
            stats[s, 5] = 1
            grids.append(None)
            continue
        g = FN.occupancy_grid(pts[m], None, None, float("nan"), resolution, padding, max_cells)      # rules 2-5 on the participants
        origin[s] = g["origin"]
        if g["stats"][7] == 2:
            stats[s, 5] = 2
            grids.append(None)
            continue
        dims[s] = g["dims"]
        stats[s, 1:5] = (g["stats"][3], g["stats"][4], g["dims"][0], g["dims"][1])
        grids.append(g)
    return {"bounds": b, "stats": stats, "dims": dims, "origin": origin, "grids": grids}


def components(grid):
    """C1: (set cells, 8-connected components)."""
    g = np.asarray(grid)
    return int(np.count_nonzero(g)), (FN.label(g)[1] if g.size else 0)


def closing_size(cells, comps):
    """C2, in Python's exact integers."""
    cells, comps = int(cells), int(comps)
    if comps == 0 or cells < 400 * comps:
        return 3
    if cells < 900 * comps:
        return 5
    if cells < 1600 * comps:
        return 7
    if cells < 2500 * comps:
        return 9
    return 11


def closing_size_float(cells, comps):
    """The reference's arithmetic: max(3, min(11, int(sqrt(mean) / 5))), made odd."""
    if comps == 0:
        return 3
    k = max(3, min(11, int(np.sqrt(np.float64(cells) / np.float64(comps)) / 5)))
    return k + 1 if k % 2 == 0 else k


def device_size(k):
    """M1: what a size read on the device acts as."""
    return int(k) if 1 <= k <= FN.MAX_KERNEL and k % 2 == 1 else 1


def slice_morphology(grid, close_size, close_iters=1, open_size=3):
    """M1-M2 for one slice."""
    return FN.morphology(grid, device_size(close_size), close_iters, open_size)


def simplify_one_with(v, area, per, resolution, area_floor, alpha):
    """outline_numpy.simplify_one with S1' and S2'."""
    eps = alpha * per
    if area * (resolution * resolution) < area_floor:
        return ON.DROP_SMALL, None, 0, 0.0, eps
    if v is None:
        return ON.DROP_OVERFLOW, None, 0, 0.0, eps
    idx = ON.douglas_peucker(v, eps)
    if len(idx) < 3:
        return ON.DROP_FEW, None, 0, 0.0, eps
    ring = [tuple(int(c) for c in v[i]) for i in idx]
    if not ON.ring_valid(ring):
        return ON.DROP_INVALID, None, 0, 0.0, eps
    s = ON.snap(ring)
    if s is not None:
        return ON.DROP_NONE, s[0], 1, s[1], eps
    return ON.DROP_NONE, np.array(ring, np.float64), 0, abs(ON.shoelace(ring)) / 2.0, eps


def simplify_outlines_with(out, resolution, area_floor, alpha, max_polygon_vertices=1 << 20):
    """dp_simplify_outlines_with on a region_outlines result: outline_numpy.simplify_outlines' dict."""
    rows = len(out["columns"])
    pol = np.zeros((rows, ON.POLYGON_COLUMNS))
    offsets = np.zeros(rows + 1, np.int32)
    verts, counts = [], np.zeros(5, np.int64)
    total = written = 0
    for r in range(rows):
        nv = int(out["columns"][r, 0])
        lo, hi = int(out["offsets"][r]), int(out["offsets"][r + 1])
        v = out["vertices"][lo:hi] if nv > 0 and hi - lo == nv else None
        reason, p, snapped, area, eps = simplify_one_with(v, out["measures"][r, 0], out["measures"][r, 1], resolution, area_floor, alpha)
        n = 0 if reason else len(p)
        total += n
        if n and total > max_polygon_vertices:
            reason, n = ON.DROP_OVERFLOW, 0
        elif n:
            verts.extend(p.tolist())
            written = total
        offsets[r + 1] = written
        counts[reason] += 1
        pol[r] = (r + 1, n, snapped, area, area * (resolution * resolution), eps, reason, nv)
    stats = np.array([rows, counts[0], total, written, counts[4], counts[1], counts[2], counts[3]], np.float64)
    return {"offsets": offsets, "vertices": np.array(verts, np.float64).reshape(-1, 2), "polygons": pol, "stats": stats}


def sliced_floor_plan(points, count=None, height_min=0.1, height_max=2.5, num_slices=5, resolution=0.05, padding=0.5, min_points=10,
                      min_area=0.1, alpha=0.01, open_size=3, max_cells=1 << 20, max_regions=4096, max_vertices=1 << 20,
                      max_polygon_vertices=1 << 18):
    """`PC.sliced_floor_plan`: slice_grids' dict with per-slice lists "counts", "close_size", "cleaned", "region_stats",
    "outlines", "polygons" added."""
    out = slice_grids(points, count, height_min, height_max, num_slices, resolution, padding, min_points, max_cells)
    out.update(counts=[], close_size=[], cleaned=[], region_stats=[], outlines=[], polygons=[], resolution=resolution)
    for s, g in enumerate(out["grids"]):
        occ = g["occupied"] if g is not None else np.zeros((0, 0), np.uint8)
        cells, comps = components(occ)
        k = closing_size(cells, comps)
        cleaned = slice_morphology(occ, k, 1, open_size)
        dens = g["density"] if g is not None else np.zeros((0, 0), np.uint32)
        hgt = g["height"] if g is not None else np.zeros((0, 0), np.float32)
        labels, n, _, rstats, _ = FN.regions(cleaned, dens, hgt, out["origin"][s], resolution, max_regions)
        o = ON.region_outlines(labels, n, max_regions, max_vertices)
        out["counts"].append((cells, comps))
        out["close_size"].append(k)
        out["cleaned"].append(cleaned)
        out["region_stats"].append(rstats)
        out["outlines"].append(o)
        out["polygons"].append(simplify_outlines_with(o, resolution, min_area, alpha, max_polygon_vertices))
    return out


def summary(plan):
    """`PC.sliced_floor_plan_summary`'s "slices" list from a `sliced_floor_plan` result of this module."""
    res, slices = plan["resolution"], []
    for s in range(len(plan["grids"])):
        st, pol, origin = plan["stats"][s], plan["polygons"][s], [float(v) for v in plan["origin"][s]]
        polygons, dropped = [], []
        for r, row in enumerate(pol["polygons"]):
            if row[6] != 0 or row[1] < 1:
                dropped.append({"label": r + 1, "reason": DROP_REASONS[int(row[6])]})
                continue
            xy = pol["vertices"][pol["offsets"][r]:pol["offsets"][r + 1]]
            polygons.append({"label": r + 1, "snapped": bool(row[2]), "flags": int(row[2]), "area_cells": float(row[3]),
                             "area": float(row[4]), "epsilon": float(row[5]), "outline_vertices": int(row[7]),
                             "vertices_grid": xy.tolist(), "vertices": (np.asarray(origin) + xy * res).tolist(),
                             "vertices_reference": ON.world_reference(xy, origin, res).tolist()})
        slices.append({"index": s, "lo": float(plan["bounds"][s, 0]), "hi": float(plan["bounds"][s, 1]),
                       "height": float(plan["bounds"][s, 2]), "participants": int(st[0]), "dropped_rows": int(st[1]),
                       "occupied_cells": int(st[2]), "status": STATUS[int(st[5])], "grid": [int(st[3]), int(st[4])],
                       "origin": origin, "set_cells": int(plan["counts"][s][0]), "components": int(plan["counts"][s][1]),
                       "close_size": int(plan["close_size"][s]),
                       "region_stats": {k: float(v) for k, v in zip(REGION_STATS, plan["region_stats"][s])},
                       "outline_stats": {k: float(v) for k, v in zip(OUTLINE_STATS, plan["outlines"][s]["stats"])},
                       "polygon_stats": {k: float(v) for k, v in zip(POLYGON_STATS, pol["stats"])},
                       "polygons": polygons, "dropped": dropped})
    return slices


def floorplan_text(slices):
    """save_floorplan_data over all slices: ascending height, within a slice last-found first."""
    lines = ["# Floor Plan Data\n", "# Units: meters\n\n", "# Shapes by height\n",
             "# Format: height, num_points, x1, z1, x2, z2, ...\n"]
    for sl in slices:
        for p in sl["polygons"][::-1]:
            xy = p["vertices_reference"]
            lines.append(f"{sl['height']:.3f}, {len(xy)}" + "".join(f", {x:.3f}, {z:.3f}" for x, z in xy) + "\n")
    return "".join(lines)


def room(seed=11):
    """The synthetic room of the end-to-end tests, about 20 000 rows: a floor, four boxes of different heights (every
    slice sees a different set), nothing between 1.06 m and 1.54 m (slice 2 is empty), and one box whose upper part is
    split by a 0.17 m gap that a 3 x 3 closing leaves open and the larger closing of a big region closes."""
    g = np.random.default_rng(seed)

    def box(x0, x1, z0, z1, y0, y1, n):
        return np.column_stack([g.uniform(x0, x1, n), g.uniform(y0, y1, n), g.uniform(z0, z1, n)])

    parts = [box(0.0, 5.0, 0.0, 4.0, -0.02, 0.05, 1500),                  # the floor: below every slice
             box(0.5, 2.0, 0.5, 1.5, 0.12, 1.05, 4200),                   # a table block: slices 0 and 1
             box(3.0, 3.5, 0.6, 1.1, 0.12, 0.55, 450),                    # a low stool: slice 0
             box(3.0, 4.2, 2.2, 3.2, 0.12, 1.05, 3800),                   # a cupboard, lower part: slices 0 and 1
             box(3.0, 4.2, 2.2, 3.2, 1.56, 2.45, 3800),                   # ... upper part: slices 3 and 4
             box(0.5, 1.45, 2.0, 3.4, 1.56, 2.45, 3400),                  # a tall shelf's upper part, left of the gap
             box(1.62, 2.57, 2.0, 3.4, 1.56, 2.45, 3400)]                 # ... and right of it
    return np.concatenate(parts)


def polygon_lists_close(got, want, rel=1e-12):
    """Two "polygons" lists: everything equal but a snapped rectangle's corners and area, within rel of the diagonal."""
    if [p["label"] for p in got] != [p["label"] for p in want]:
        return False
    for a, b in zip(got, want):
        for k in ("snapped", "flags", "epsilon", "outline_vertices"):
            if a[k] != b[k]:
                return False
        if not a["snapped"]:
            if any(a[k] != b[k] for k in ("area_cells", "area", "vertices_grid", "vertices", "vertices_reference")):
                return False
            continue
        w = np.asarray(b["vertices_grid"])
        diag = float(np.hypot(*(w.max(axis=0) - w.min(axis=0))))
        if np.asarray(a["vertices_grid"]).shape != w.shape or np.linalg.norm(np.asarray(a["vertices_grid"]) - w, axis=1).max() > rel * diag:
            return False
        if abs(a["area_cells"] - b["area_cells"]) > rel * b["area_cells"] or not math.isclose(a["area"], b["area"], rel_tol=2 * rel):
            return False
    return True
