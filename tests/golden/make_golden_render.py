"""Writes golden_render.npz: a small box-and-floor cloud and what tests/render_numpy.py makes of it (data only).

    python tests/golden/make_golden_render.py

The scene is chosen so that no point's centre lies within 1e-9 of a pixel boundary in any preset (test_render.py checks
that the share of such points is 0 before it compares the restatement with the independent camera)."""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import render_numpy as RN  # noqa: E402

N, SEED, SIZE, POINT_SIZE, MIN_HEIGHT = 600, 7, (64, 40), 7, 0.5
VIEWS = ("front", "top", "side", "isometric", "plan")


def main():
    pts, cols = RN.scene(N, SEED)
    res = RN.render_views(pts, cols, VIEWS, SIZE, POINT_SIZE, min_height=MIN_HEIGHT)
    sheet = RN.render_views(pts, None, RN.SHEET, (16, 9), 3, sheet=True)
    keys = RN.GLOBAL_STATS + RN.VIEW_STATS
    np.savez_compressed(os.path.join(HERE, "golden_render.npz"), points=pts, colors=cols, image=res["image"], cameras=res["cameras"],
                        stats=np.array([np.ravel(res["stats"][k]).tolist() + [0] * (5 - np.size(res["stats"][k])) for k in keys], np.int64),
                        sheet=sheet["image"])


if __name__ == "__main__":
    main()
