"""Makes tests/golden/golden_outline.npz: the small grids of tests/test_outline.py, their scipy.ndimage labels, and the
outlines and polygons tests/outline_numpy.py gives for them (the expected values the restatement is held to).
Run from the repository root: python tests/golden/make_golden_outline.py"""

import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import outline_numpy as ON  # noqa: E402

OUT = os.path.join(HERE, "golden_outline.npz")
ONES3 = np.ones((3, 3), bool)
RES = 0.1
MIN_AREAS = (0.025, 0.0)


def shapes_grid():
    """One region per case of S1-S6, none touching: see SHAPES for what each becomes."""
    a = np.zeros((44, 72), np.uint8)
    a[2:8, 2:12] = 1                                     # 1 rect: 4 vertices, snapped
    for k in range(9):
        a[2 + k, 16:17 + k] = 1                          # 2 triangle: 3 vertices
    for k in range(-5, 6):
        a[8 + k, 36 - (5 - abs(k)):36 + (5 - abs(k)) + 1] = 1    # 3 diamond: 4 vertices, snapped at 45 degrees
    a[2:12, 46:50] = a[8:12, 46:58] = 1                  # 4 L: 6 vertices, not snapped
    a[2:4, 62:64] = 1                                    # 5 block 2 x 2: area 1 cell, kept at 0.1 m
    a[16:24, 2:14] = 1
    a[16, 2] = a[23, 13] = 0                             # 6 rect less two corners: 6 vertices, snapped
    a[16:24, 18:30] = 1
    a[16, 18] = a[23, 29] = a[16, 29] = 0                # 7 rect less three corners: 7 vertices
    a[16, 34] = 1                                        # 8 single cell
    a[16, 38:45] = 1                                     # 9 horizontal line
    a[18:25, 34] = 1                                     # 10 vertical line
    a[16:22, 48:54] = 1
    a[18, 54:60] = 1                                     # 11 square with an antenna: a spike, invalid
    a[28:36, 2] = a[35, 2:10] = 1                        # 12 one-cell-wide L: the ring runs back over itself, invalid
    a[28:40, 14:34] = 1
    a[30:33, 16:20] = a[35:38, 24:31] = 0                # 13 rect with two holes: the holes are ignored
    a[28:41, 40:53] = 1
    a[28:41, 40:53] &= (np.hypot(*np.indices((13, 13)) - 6) <= 6.3).astype(np.uint8)     # 14 disc: many vertices
    return a


def more_grids(g):
    plus = np.zeros((21, 33), np.uint8)
    plus[8:13, :] = plus[:, 14:19] = 1                   # touches all four grid edges
    dots = np.zeros((30, 48), np.uint8)
    for z in range(0, 28, 4):
        for x in range(0, 44, 4):
            dots[z:z + 3, x:x + 3] = 1                   # 7 x 11 = 77 regions of 3 x 3
    dots[1, 1] = 0                                       # one of them with a hole
    blob = ndimage.binary_closing(g.random((67, 127)) < 0.42, structure=ONES3, iterations=1).astype(np.uint8)
    h1 = np.array([[1, 1, 0, 1, 0, 0, 1, 1, 1]], np.uint8)
    return {"shapes": shapes_grid(), "plus": plus, "dots": dots, "blob": blob, "h1": h1, "w1": h1.T.copy(),
            "empty": np.zeros((5, 9), np.uint8), "full": np.ones((6, 70), np.uint8)}


def main():
    g = np.random.default_rng(31)
    out, names = {}, []
    for name, a in more_grids(g).items():
        names.append(name)
        lab = ndimage.label(a, structure=ONES3)[0].astype(np.int32)
        o = ON.region_outlines(lab)
        out[f"{name}_grid"], out[f"{name}_labels"] = a, lab
        for k in ("offsets", "vertices", "columns", "measures", "stats"):
            out[f"{name}_{k}"] = o[k]
        for i, ma in enumerate(MIN_AREAS):
            p = ON.simplify_outlines(o, RES, ma)
            for k in ("offsets", "vertices", "polygons", "stats"):
                out[f"{name}_poly{i}_{k}"] = p[k]
    out["names"] = np.array(names)
    out["resolution"], out["min_areas"] = np.float64(RES), np.array(MIN_AREAS)
    pol = out["shapes_poly1_polygons"]
    print("shapes: vertices", pol[:, 1].astype(int).tolist(), "flags", pol[:, 2].astype(int).tolist(), "reasons",
          pol[:, 6].astype(int).tolist(), "outline", pol[:, 7].astype(int).tolist())
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
