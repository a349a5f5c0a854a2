"""Builds tests/golden/golden_slices.npz from the project's own restatement (tests/slices_numpy.py) and scipy:

    python tests/golden/make_golden_slices.py

The file holds the synthetic room of the end-to-end tests (tests/slices_numpy.py: room) and what the restatement makes
of it at the defaults of `PC.sliced_floor_plan`: bounds, per-slice statistics, sizes, origins, (set cells, components),
closing sizes, and every slice's cleaned grid, polygon rows, offsets and vertices.  The component counts are checked
against scipy.ndimage.label here, before anything is written.
"""

import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import slices_numpy as SL  # noqa: E402


def main():
    pts = SL.room()
    plan = SL.sliced_floor_plan(pts)
    out = {"room_points": pts, "bounds": plan["bounds"], "stats": plan["stats"], "dims": plan["dims"], "origin": plan["origin"],
           "counts": np.array(plan["counts"], np.int64), "close_size": np.array(plan["close_size"], np.int32)}
    for s, g in enumerate(plan["grids"]):
        occ = g["occupied"] if g is not None else np.zeros((0, 0), np.uint8)
        assert plan["counts"][s][1] == (ndimage.label(occ, structure=np.ones((3, 3)))[1] if occ.size else 0)
        out[f"slice{s}_cleaned"] = plan["cleaned"][s]
        for k in ("polygons", "offsets", "vertices", "stats"):
            out[f"slice{s}_poly_{k}"] = plan["polygons"][s][k]
    np.savez_compressed(os.path.join(HERE, "golden_slices.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
