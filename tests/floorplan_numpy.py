"""Numpy restatement of the occupancy floor plan's specification (include/dp_mi355x.h, "Occupancy floor plan
(ABI 20)", rules 1-15), written from the header, not from the kernels.  Plain loops where that is the clearest
form; tests/test_floorplan.py pins it to scipy.ndimage through tests/golden/golden_floorplan.npz."""

import numpy as np

MAX_DIM, MAX_KERNEL, COLUMNS = 8192, 15, 13


def occupancy_grid(points, colors=None, count=None, height_threshold=1.3, resolution=0.1, padding=0.2, max_cells=1 << 22):
    """Rules 1-6.  Returns a dict: density, height, color (or None), occupied (H x W arrays), dims, origin, stats."""
    pts = np.asarray(points, np.float64)[:len(points) if count is None else count]
    fin = np.isfinite(pts).all(axis=1)
    part = fin.copy() if np.isnan(height_threshold) else fin & (pts[:, 1] >= height_threshold)
    stats = np.zeros(8)
    stats[0], stats[1], stats[2] = part.sum(), (~fin).sum(), (fin & ~part).sum()
    empty = {"density": np.zeros((0, 0), np.uint32), "height": np.zeros((0, 0), np.float32), "occupied": np.zeros((0, 0), np.uint8),
             "color": None if colors is None else np.zeros((0, 0, 3), np.uint8), "dims": (0, 0), "origin": (0.0, 0.0), "stats": stats}
    if not part.any():
        stats[7] = 1
        return empty
    rows = np.flatnonzero(part)
    x, y, z = pts[rows, 0], pts[rows, 1], pts[rows, 2]
    min_x, max_x = x.min() - padding, x.max() + padding
    min_z, max_z = z.min() - padding, z.max() + padding
    with np.errstate(over="ignore", invalid="ignore"):
        wf, hf = np.ceil((max_x - min_x) / resolution), np.ceil((max_z - min_z) / resolution)
    empty["origin"] = (min_x, min_z)
    if not (wf <= MAX_DIM and hf <= MAX_DIM) or int(wf) * int(hf) > max_cells:
        stats[7] = 2
        return empty
    W, H = int(wf), int(hf)
    density = np.zeros((H, W), np.uint32)
    height = np.zeros((H, W), np.float32)
    owner = np.full((H, W), -1, np.int64)
    color = None if colors is None else np.zeros((H, W, 3), np.uint8)
    yf = y.astype(np.float32)
    for k, row in enumerate(rows):                      # ascending rows: a later row needs a strictly larger height
        gx, gz = int((x[k] - min_x) / resolution), int((z[k] - min_z) / resolution)
        if gx >= W or gz >= H:
            stats[3] += 1
            continue
        density[gz, gx] += 1
        if owner[gz, gx] < 0 or yf[k] > height[gz, gx]:
            owner[gz, gx], height[gz, gx] = row, yf[k]
    height[density == 0] = 0
    if color is not None:
        color[owner >= 0] = np.asarray(colors, np.uint8)[owner[owner >= 0]]
    stats[4], stats[5], stats[6] = (density > 0).sum(), H, W
    return {"density": density, "height": height, "color": color, "occupied": (density > 0).astype(np.uint8), "owner": owner,
            "dims": (H, W), "origin": (min_x, min_z), "stats": stats}


def _window(grid, size, outside, combine):
    """combine (or / and) over the size x size window around every cell; cells outside the grid read `outside`."""
    g = np.asarray(grid) != 0
    H, W = g.shape
    r = size // 2
    padded = np.full((H + 2 * r, W + 2 * r), bool(outside))
    padded[r:r + H, r:r + W] = g
    out = padded[r:r + H, r:r + W].copy()
    for dz in range(size):                              # one shifted copy of the grid per element of the square
        for dx in range(size):
            out = combine(out, padded[dz:dz + H, dx:dx + W])
    return out.astype(np.uint8)


def dilate(grid, size):
    """Rule 8: a cell is set iff any cell of its window is; outside reads 0."""
    return _window(grid, size, 0, np.logical_or)


def erode(grid, size):
    """Rule 8: a cell is set iff every cell of its window is; outside reads 1."""
    return _window(grid, size, 1, np.logical_and)


def morphology(grid, close_size=7, close_iters=2, open_size=3):
    """Rule 7."""
    g = (np.asarray(grid) != 0).astype(np.uint8)
    if close_size > 1:
        for _ in range(close_iters):
            g = erode(dilate(g, close_size), close_size)
    if open_size > 1:
        g = dilate(erode(g, open_size), open_size)
    return g


def label(grid):
    """Rule 9: 8-connected components, numbered in row-major order of their first cell (flood fill)."""
    g = np.asarray(grid) != 0
    H, W = g.shape
    labels = np.zeros((H, W), np.int32)
    n = 0
    for z0 in range(H):
        for x0 in range(W):
            if not g[z0, x0] or labels[z0, x0]:
                continue
            n += 1
            labels[z0, x0] = n
            stack = [(z0, x0)]
            while stack:
                z, x = stack.pop()
                for dz in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        zz, xx = z + dz, x + dx
                        if 0 <= zz < H and 0 <= xx < W and g[zz, xx] and not labels[zz, xx]:
                            labels[zz, xx] = n
                            stack.append((zz, xx))
    return labels, n


def regions(grid, density, height, origin, resolution, max_regions=4096):
    """Rules 9-11.  Returns (labels, n, table (min(n, max_regions), 13), stats, height-sum bound per row)."""
    labels, n = label(grid)
    H, W = labels.shape
    rows = min(n, max_regions)
    table = np.zeros((rows, COLUMNS))
    bound = np.zeros(rows)
    zz, xx = np.indices((H, W)) if H * W else (np.zeros((0, 0), int),) * 2
    for r in range(rows):
        m = labels == r + 1
        cells = int(m.sum())
        gx, gz = xx[m], zz[m]
        cx, cz = float(int(gx.sum())) / cells, float(int(gz.sum())) / cells
        occ = m & (density > 0)
        hs = height[occ].astype(np.float64)
        table[r] = [cells, cells * (resolution * resolution), gx.min(), gz.min(), gx.max(), gz.max(), cx, cz,
                    origin[0] + (cx + 0.5) * resolution, origin[1] + (cz + 0.5) * resolution, int(density[m].sum()),
                    hs.max() if len(hs) else 0.0, hs.sum() / len(hs) if len(hs) else 0.0]
        bound[r] = cells * 2.0 ** -52 * (np.abs(hs).max() if len(hs) else 0.0)
    stats = np.array([np.count_nonzero(np.asarray(grid)), n, rows, float(n > max_regions), H, W, 0, 0], np.float64)
    return labels, n, table, stats, bound


def image(labels, table, resolution, min_area=0.025, max_height=2.5, color_by_height=True):
    """Rules 12-15."""
    H, W = labels.shape
    img = np.full((H, W, 3), 255, np.uint8)
    sat = lambda v: int(min(255, max(0, int(v))))      # noqa: E731
    for z in range(H):
        for x in range(W):
            l = labels[z, x]
            if l < 1 or l > len(table) or not table[l - 1, 1] >= min_area:
                continue
            nb = [(z, x - 1), (z, x + 1), (z - 1, x), (z + 1, x)]
            if any(not (0 <= a < H and 0 <= b < W) or labels[a, b] != l for a, b in nb):
                img[z, x] = 0
            elif not color_by_height:
                img[z, x] = 180
            else:
                h = min(1.0, table[l - 1, 12] / max_height)
                img[z, x] = [sat(255 * h), sat(255 * (1 - abs(2 * h - 1))), sat(255 * (1 - h))]
    L = int(1.0 / resolution)
    x0, z0 = min(W - 50 - L, W - 10), min(H - 50, H - 10)
    if x0 > 0 and z0 > 0 and z0 < H and x0 + L < W:
        img[z0:z0 + 20, x0:x0 + L] = 0
    return img


def floor_plan(points, colors=None, count=None, height_threshold=1.3, resolution=0.1, padding=0.2, close_size=7, close_iters=2,
               open_size=3, min_area=0.025, max_height=2.5, max_cells=1 << 22, max_regions=4096):
    """The four stages in a row, as `PC.floor_plan`."""
    g = occupancy_grid(points, colors, count, height_threshold, resolution, padding, max_cells)
    cleaned = morphology(g["occupied"], close_size, close_iters, open_size)
    labels, n, table, rstats, bound = regions(cleaned, g["density"], g["height"], g["origin"], resolution, max_regions)
    return {"grid": g, "cleaned": cleaned, "labels": labels, "n_regions": n, "table": table, "region_stats": rstats,
            "bound": bound, "image": image(labels, table, resolution, min_area, max_height)}
