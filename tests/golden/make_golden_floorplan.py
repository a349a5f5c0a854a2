"""Makes tests/golden/golden_floorplan.npz: the inputs of tests/test_floorplan.py and what scipy.ndimage says about
them (binary dilation / erosion with OpenCV's border values, 8-connected labels, sums, boxes, centres of mass).
Run from the repository root: python tests/golden/make_golden_floorplan.py"""

import os

import numpy as np
from scipy import ndimage

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden_floorplan.npz")
MORPH_SHAPES = [(1, 1), (3, 5), (37, 63), (37, 64), (37, 65), (70, 130), (129, 200)]
MORPH_SIZES = (3, 7, 15)
ONES3 = np.ones((3, 3), bool)


def raster_cloud(g):
    """About 5 000 rows: a few furniture-like boxes and blobs over a 7.3 m x 5.1 m floor, loose rows between them,
    heights on a coarse lattice (so cells hold equal heights), pairs that differ below float32 resolution, rows below
    the threshold, NaN / inf rows, and 200 rows past the live count."""
    parts = []
    for (x0, z0, w, d, n) in ((0.5, 0.4, 1.6, 0.9, 1400), (3.1, 0.6, 0.5, 0.5, 500), (4.6, 2.2, 2.2, 1.3, 1500),
                              (1.0, 3.3, 0.32, 0.31, 160), (2.6, 3.9, 0.33, 0.3, 160)):
        xy = g.uniform([x0, z0], [x0 + w, z0 + d], (n, 2))
        parts.append(np.column_stack([xy[:, 0], np.round(g.uniform(1.3, 2.4, n) * 8) / 8, xy[:, 1]]))
    loose = g.uniform([0.0, 0.0], [7.3, 5.1], (380, 2))
    parts.append(np.column_stack([loose[:, 0], g.uniform(1.3, 2.9, 380), loose[:, 1]]))
    low = g.uniform([0.0, 0.0], [7.3, 5.1], (900, 2))
    parts.append(np.column_stack([low[:, 0], g.uniform(-0.2, 1.29, 900), low[:, 1]]))
    pts = np.concatenate(parts)
    pts[:, 0] -= 3.4                                     # both signs of x: no flip may be hidden by symmetry
    g.shuffle(pts)
    pts = pts[:5000]
    twins = g.choice(5000, 60, replace=False)            # same cell, heights equal in float32 but not in float64
    pts[twins[:30]] = pts[twins[30:]] + [1e-4, 1e-9, 1e-4]
    bad = g.choice(5000, 12, replace=False)
    pts[bad[:4], 0], pts[bad[4:8], 1], pts[bad[8:], 2] = np.nan, np.inf, -np.inf
    extra = np.column_stack([g.uniform(-9, 9, 200), g.uniform(1.5, 2.0, 200), g.uniform(-9, 9, 200)])   # past the live count
    return np.concatenate([pts, extra]), 5000, bad


def morph_grids(g):
    grids = {}
    for (h, w) in MORPH_SHAPES:
        a = (g.random((h, w)) < 0.03).astype(np.uint8)
        a[0, g.integers(0, w)] = a[h - 1, g.integers(0, w)] = a[g.integers(0, h), 0] = a[g.integers(0, h), w - 1] = 1
        a[0, 0] = a[h - 1, w - 1] = 1
        grids[f"random_{h}x{w}"] = a
    frame = np.zeros((37, 65), np.uint8)
    frame[0, :] = frame[-1, :] = frame[:, 0] = frame[:, -1] = 1
    plus = np.zeros((70, 130), np.uint8)
    plus[33:37, :] = plus[:, 62:67] = 1
    holes = np.ones((37, 64), np.uint8)
    holes[g.random((37, 64)) < 0.03] = 0
    grids.update(frame_37x65=frame, plus_70x130=plus, holes_37x64=holes, full_3x5=np.ones((3, 5), np.uint8))
    return grids


def spiral(h, w):
    """A one-cell-wide rectangular spiral with one empty cell between its turns: one long chain."""
    a = np.zeros((h, w), np.uint8)
    top, left, bottom, right = 0, 0, h - 1, w - 1
    a[top, left:right + 1] = 1
    while True:
        if bottom - top < 2 or right - left < 2:
            break
        a[top:bottom + 1, right] = 1
        a[bottom, left:right + 1] = 1
        if bottom - top < 4 or right - left < 4:
            break
        a[top + 2:bottom + 1, left] = 1
        a[top + 2, left:right - 1] = 1
        top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
    return a


def region_grids(g):
    combs = np.zeros((40, 67), np.uint8)
    combs[0, :] = combs[-1, :] = 1
    combs[0:37, 0::4] = 1                                # teeth down from the top bar ...
    combs[3:40, 2::4] = 1                                # ... and up from the bottom bar, never touching
    diag = np.zeros((33, 70), np.uint8)
    for k in range(33):
        diag[k, k] = diag[k, 69 - k] = 1                 # two diagonals crossing: corner contacts only
        diag[k, (k * 2 + 40) % 70] = 1
    checker = (np.indices((65, 130)).sum(axis=0) % 2).astype(np.uint8)
    many = np.zeros((66, 131), np.uint8)
    many[0::2, 0::2] = 1                                 # 33 x 66 = 2178 single cells, none touching
    blobs = (g.random((70, 130)) < 0.3).astype(np.uint8)
    return {"spiral": spiral(65, 130), "combs": combs, "diagonals": diag, "checkerboard": checker, "empty": np.zeros((9, 70), np.uint8),
            "full": np.ones((20, 66), np.uint8), "many": many, "blobs": blobs}


def main():
    g = np.random.default_rng(20)
    out = {}
    pts, count, bad = raster_cloud(g)
    out["cloud_points"], out["cloud_count"], out["cloud_bad"] = pts, np.int64(count), bad
    out["cloud_colors"] = g.integers(0, 256, (len(pts), 3), dtype=np.uint8)
    names = []
    for name, a in morph_grids(g).items():
        names.append(name)
        out[f"morph_{name}"] = a
        for k in MORPH_SIZES:
            s = np.ones((k, k), bool)
            dil = ndimage.binary_dilation(a, structure=s, border_value=0)
            ero = ndimage.binary_erosion(a, structure=s, border_value=1)
            out[f"morph_{name}_dilate{k}"] = np.packbits(dil)
            out[f"morph_{name}_erode{k}"] = np.packbits(ero)
            out[f"morph_{name}_close{k}"] = np.packbits(ndimage.binary_erosion(dil, structure=s, border_value=1))
            out[f"morph_{name}_open{k}"] = np.packbits(ndimage.binary_dilation(ero, structure=s, border_value=0))
    out["morph_names"] = np.array(names)
    names = []
    for name, a in region_grids(g).items():
        names.append(name)
        lab, n = ndimage.label(a, structure=ONES3)
        idx = np.arange(1, n + 1)
        out[f"region_{name}"] = a
        out[f"region_{name}_labels"] = lab.astype(np.int32)
        out[f"region_{name}_sum"] = np.asarray(ndimage.sum(a, lab, idx), np.float64).reshape(-1)
        out[f"region_{name}_com"] = np.asarray(ndimage.center_of_mass(a, lab, idx), np.float64).reshape(-1, 2)   # (z, x)
        out[f"region_{name}_box"] = np.array([[s[1].start, s[0].start, s[1].stop - 1, s[0].stop - 1]
                                              for s in ndimage.find_objects(lab)], np.int64).reshape(-1, 4)
    out["region_names"] = np.array(names)
    assert out["region_spiral_labels"].max() == 1 and out["region_spiral"].sum() > 4000
    assert out["region_combs_labels"].max() == 2 and out["region_checkerboard_labels"].max() == 1
    assert out["region_many_labels"].max() == 2178 and ndimage.label(out["region_diagonals"])[1] > 50
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
