"""Golden vectors for the ground stages, from the REFERENCE's own functions.

Run in the build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ground.py

`img_to_normalized_pointcloud.py` imports open3d / cv2 at module level (absent here), so
`depth_to_3d`, `grid_based_ground_plane_fit`, `point_plane_distances`,
`normalize_point_cloud_to_ground`, `grid_based_ground_adjustment` and `apply_rotation_to_plane`
are lifted out of the reference file with `ast` at run time (numpy + sklearn's RANSACRegressor)
and run on synthetic pinhole views of a tilted floor with a far wall and a box.  No reference text
is stored.  Output: golden_ground.npz -- per scene the depth, f, the fitted model, the normalised
points and the adjusted y column for (grid_size, percentile) in {(20, 5), (7, 50)} (the adjustment
changes y only; in the no-rotation scenes the normalisation does too, so x and z are not stored).

The generator asserts what the tests rely on:
 (a) the reference fit gives the same model for 20 np.random.seed values (its RANSAC is stochastic);
 (b) no point lies within 1e-6 of a discontinuous decision threshold (tests/ground_numpy.py margins);
 (c) no two points tie at a lowest-5 % cut.
"""

import ast
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(REPO, "ml-depth-pro-video_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
REF_PC = "/root/reference/img_to_normalized_pointcloud.py"
NAMES = ("depth_to_3d", "grid_based_ground_plane_fit", "point_plane_distances", "normalize_point_cloud_to_ground",
         "grid_based_ground_adjustment", "apply_rotation_to_plane")
ADJUST_CASES = ((20, 5), (7, 50))
ROT = [1.5, -2.0, 0.5]


def lift_all():
    tree = ast.parse(open(REF_PC).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    ns = {"np": np}
    exec(compile(ast.Module(body=fns, type_ignores=[]), REF_PC, "exec"), ns)
    return ns


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def scene(h, w, f, tilt_deg, side_deg, cam_h, wall, seed, rows_from=0.0):
    """Depth of a pinhole view: floor n . p + cam_h = 0 tilted by tilt (about x) and side (about z),
    a wall at z = wall, a box standing on the floor; a few NaN / 0 pixels."""
    g = np.random.default_rng(seed)
    v, u = np.indices((h, w)).astype(np.float64)
    v = v + rows_from * h                                   # a strip from the lower part of a taller image
    H = h * (1 + rows_from)
    rx, ry = -(u - w / 2) / f, -(v - H / 2) / f             # ray = (rx, ry, 1) * z
    t, s = np.radians(tilt_deg), np.radians(side_deg)
    n = np.array([np.sin(s), np.cos(s) * np.cos(t), np.cos(s) * np.sin(t)])
    nr = n[0] * rx + n[1] * ry + n[2]
    zf = np.where(nr < -1e-9, -cam_h / np.minimum(nr, -1e-9), np.inf)
    depth = np.minimum(zf, wall)
    zb = 0.45 * wall                                        # box front face
    xb, yb = rx * zb, ry * zb
    floor_y = -(cam_h + n[0] * xb + n[2] * zb) / n[1]
    box = (xb > -0.9) & (xb < 0.1) & (yb > floor_y) & (yb < floor_y + 0.8) & (depth > zb)
    depth = np.where(box, zb, depth)
    depth = depth * (1 + 2e-3 * g.standard_normal((h, w)))  # sensor noise: no exact ties, no exact plane
    depth = depth.astype(np.float32)
    bad = g.random((h, w))
    depth[bad < 0.004] = np.nan
    depth[(bad > 0.004) & (bad < 0.008)] = 0.0
    return depth


SCENES = {
    # name: (h, w, f, tilt, side, camera height, wall, first noise seed, rows_from)
    "flat": (96, 128, 110.0, 3.0, 0.0, 1.5, 9.0, 1, 0.0),        # |n . y| > 0.99: no-rotation branch
    "side": (37, 300, 60.0, 4.0, 9.0, 0.5, 7.0, 2, 0.0),         # n . y < 0.99: Rodrigues branch
    "strip": (12, 128, 30.0, 2.0, 0.0, 0.4, 5.0, 3, 0.0),        # 12 rows: < 10 trace bins -> fallback
}


def main():
    import ground_numpy as G

    ref = lift_all()
    out = {"scenes": np.array(list(SCENES))}
    for name, spec in SCENES.items():
        # conditions (a)-(c) are properties of the fixture: take the first noise seed that meets them
        for seed in range(spec[7], spec[7] + 50):
            try:
                one_scene(ref, G, out, name, *spec[:7], seed, spec[8])
                print(name, "seed", seed)
                break
            except AssertionError as e:
                print(name, "seed", seed, "rejected:", e)
        else:
            raise SystemExit(f"no seed meets the fixture conditions for {name}")
    out["rot_offset"] = np.array(ROT)
    path = os.path.join(HERE, "golden_ground.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


def one_scene(ref, G, out, name, h, w, f, tilt, side, cam_h, wall, seed, rows_from):
    depth = scene(h, w, f, tilt, side, cam_h, wall, seed, rows_from)
    pts, _ = ref["depth_to_3d"](depth, f, w, h)
    models = []
    for sd in range(20):
        np.random.seed(sd)
        models.append(quiet(ref["grid_based_ground_plane_fit"], pts, None))
    vec = np.array([np.concatenate([m["normal"], [m["d"]], m["origin"]]) for m in models])
    spread = np.abs(vec - vec[0]).max()
    assert spread == 0.0, (name, "fit varies with the seed", spread)            # (a)
    model = models[0]
    ours, info = G.fit(pts)
    assert info["tie_free"], (name, "tie at a lowest-5% cut")                     # (c)
    assert info["margin"] > 1e-6, (name, "z at a bin edge", info["margin"])       # (b)
    assert info["pushdown_safe"], (name, "push-down count at its threshold")       # (b)
    normed = quiet(ref["normalize_point_cloud_to_ground"], pts, model)
    _, nstats, margin = G.normalize(pts, model)
    assert margin > 1e-6, (name, "normalise margin", margin)                      # (b)
    rotated = bool(G.ground_rotation(model)[14])
    out[f"{name}_depth"], out[f"{name}_f"] = depth, np.array(f)
    out[f"{name}_model"] = vec[0]
    out[f"{name}_rotated"] = np.array(rotated)
    out[f"{name}_fallback"] = np.array(info["fallback"])
    out[f"{name}_normalized"] = normed if rotated else normed[:, 1].copy()
    if not rotated:
        assert (normed[:, [0, 2]] == pts[:, [0, 2]]).all()
    for gs, pc in ADJUST_CASES:
        adj = quiet(ref["grid_based_ground_adjustment"], normed, grid_size=gs, percentile=pc)
        _, astats, margin = G.adjust(normed, gs, pc)
        assert margin > 1e-6, (name, gs, pc, "adjust margin", margin)             # (b)
        assert (adj[:, [0, 2]] == normed[:, [0, 2]]).all()
        out[f"{name}_adjusted_{gs}_{pc}"] = adj[:, 1].copy()
        print(name, gs, pc, "cells adjusted", int(astats[4]), "points adjusted", int(astats[5]))
    rot = quiet(ref["apply_rotation_to_plane"], model, ROT)
    out[f"{name}_rot_model"] = np.concatenate([rot["normal"], [rot["d"]]])
    print(name, "points", len(pts), "model", vec[0][:4], "rotated", rotated, "fallback", info["fallback"],
          "trace bins", int(info["valid"].sum()), "norm stats", nstats)


if __name__ == "__main__":
    main()
