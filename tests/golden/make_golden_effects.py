"""Builds tests/golden/golden_effects.npz from the project's own restatement (tests/effects_numpy.py) and scipy:

    python tests/golden/make_golden_effects.py

The file holds a 37 x 53 frame (tests/effects_numpy.py: scene) and what the restatement makes of it: the three motions
at five phases of a 150-frame cycle (amplitude 0.05), the anaglyph at separation 0.05, and the literal (transposed)
form of both.  Checked here, before anything is written: the integer sampler agrees with
scipy.ndimage.map_coordinates(order=1) on the 1/32-quantised coordinates within one grey level everywhere, and the
literal form is the transpose of ours.
"""

import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import effects_numpy as FX  # noqa: E402

H, W, TOTAL, AMPLITUDE, SEPARATION = 37, 53, 150, 0.05, 0.05
PHASES = (0, 19, 37, 75, 113)
MOTIONS = ("circle", "zoom", "swing")


def sampler_vs_scipy(image, map_x, map_y):
    """Largest difference in grey levels between the integer sampler and scipy's linear interpolation at the same
    1/32-quantised coordinates."""
    qx = np.rint(map_x * np.float32(32)).astype(np.int64) / 32.0
    qy = np.rint(map_y * np.float32(32)).astype(np.int64) / 32.0
    ours = FX.remap_linear_u8(image, map_x, map_y).astype(np.float64)
    worst = 0.0
    for c in range(image.shape[2]):
        ref = ndimage.map_coordinates(image[..., c].astype(np.float64), [qy, qx], order=1, mode="nearest")
        worst = max(worst, float(np.abs(ours[..., c] - ref).max()))
    return worst


def views():
    return [FX.view_params(m, AMPLITUDE, W, H, f, TOTAL) for m in MOTIONS for f in PHASES]


def main():
    image, depth = FX.scene(H, W, 0)
    vs = views()
    out, bad = FX.warp_views(image, depth, vs)
    assert not bad.any()
    worst = 0.0
    for v, ours in zip(vs, out):
        mx, my = FX.maps(depth, v)
        mx, my = np.clip(mx, 0, W - 1).astype(np.float32), np.clip(my, 0, H - 1).astype(np.float32)
        worst = max(worst, sampler_vs_scipy(image, mx, my))
        literal = FX.warp_view(image, depth, v, literal=True)[0]
        assert literal.shape == (W, H, 3) and np.array_equal(literal.transpose(1, 0, 2), ours)
    assert worst <= 1.0, worst
    ana, ana_bad = FX.anaglyph(image, depth, SEPARATION)
    ana_literal = FX.anaglyph(image, depth, SEPARATION, literal=True)[0]
    assert ana_bad == 0 and np.array_equal(ana_literal.transpose(1, 0, 2), ana)
    np.savez_compressed(os.path.join(HERE, "golden_effects.npz"), image=image, depth=depth,
                        views=np.array(vs, np.float64), phases=np.array(PHASES), out=out, anaglyph=ana,
                        literal_first=FX.warp_view(image, depth, vs[1], literal=True)[0], anaglyph_literal=ana_literal,
                        parameters=np.array([TOTAL, AMPLITUDE, SEPARATION]))
    print(f"sampler vs scipy: {worst:.4f} grey levels at the most; views {out.shape}")


if __name__ == "__main__":
    main()
