"""Golden vectors for the cleaning stage, from the REFERENCE's own functions.

Run in the build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_clean.py

`pointcloud_cleaner.py` imports open3d at module level (absent here), so `remove_stray_points` and
`clean_shadows` are lifted out of the reference file with `ast` at run time and given a minimal
stand-in for the `o3d` names they touch: a point-cloud object with `.points` / `.colors`,
`Vector3dVector = np.asarray`, and a `KDTreeFlann` whose radius search is the strict-`<` brute force
of the header's restatement.  No reference text is stored.  They run on small synthetic levelled
scenes (floor, wall, box, isolated specks, thin vertical curtains behind the box edges, and a few
hand-built columns and clusters that pin the rules).  Output: golden_clean.npz -- per scene the points,
colours, the stray keep mask, the shadow keep mask (over the stray survivors), the shadow cell size
and the counts the reference prints.  x and z are fp32-representable doubles (they compress well).

The generator asserts what the tests rely on:
 (a) no tested column's median angle, and no single angle, lies within 1e-9 degrees of 75;
 (b) no column's height lies within 1e-9 of 0.1;
 (c) every column of more than 16 points has no two equal y values (the reference's argsort is
     unstable there; below that it is an insertion sort, which is stable);
 (d) the fixture holds removed and kept columns, odd and even angle counts, an even-count column
     decided by the c == m/2 case on each side of 75, a column with a duplicated point (NaN median),
     and stray points with exactly nb_points - 1 and exactly nb_points neighbours;
and that tests/clean_numpy.py reproduces the reference's masks exactly.
"""

import ast
import contextlib
import copy
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
REF = "/root/reference/pointcloud_cleaner.py"
NAMES = ("remove_stray_points", "clean_shadows")
NB, RADIUS = 20, 0.1


class PointCloud:
    def __init__(self, points, colors):
        self.points, self.colors = points, colors


class KDTreeFlann:
    def __init__(self, pcd):
        self.P = np.asarray(pcd.points)

    def search_radius_vector_3d(self, q, radius):
        d = self.P - np.asarray(q)
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        idx = np.flatnonzero(d2 < radius * radius)
        return len(idx), idx, d2[idx]


def lift():
    tree = ast.parse(open(REF).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    o3d = types.SimpleNamespace(utility=types.SimpleNamespace(Vector3dVector=np.asarray),
                                geometry=types.SimpleNamespace(KDTreeFlann=KDTreeFlann, PointCloud=PointCloud))
    ns = {"np": np, "o3d": o3d, "copy": copy}
    exec(compile(ast.Module(body=fns, type_ignores=[]), REF, "exec"), ns)
    return ns


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def ref_masks(ref, pts):
    """The reference's two functions in sequence; the colours carry the row index, which gives the masks."""
    tag = np.repeat(np.arange(len(pts), dtype=np.float64)[:, None], 3, axis=1)
    a = quiet(ref["remove_stray_points"], PointCloud(pts, tag), nb_points=NB, radius=RADIUS)
    k1 = np.zeros(len(pts), dtype=bool)
    k1[np.asarray(a.colors)[:, 0].astype(np.int64)] = True
    assert np.array_equal(np.asarray(a.points), pts[k1])
    p1 = pts[k1]
    tag1 = np.repeat(np.arange(len(p1), dtype=np.float64)[:, None], 3, axis=1)
    b = quiet(ref["clean_shadows"], PointCloud(p1, tag1))
    k2 = np.zeros(len(p1), dtype=bool)
    k2[np.asarray(b.colors)[:, 0].astype(np.int64)] = True
    assert np.array_equal(np.asarray(b.points), p1[k2])
    return k1, k2


def grid(u0, u1, v0, v1, step):
    u, v = np.meshgrid(np.arange(u0, u1, step), np.arange(v0, v1, step), indexing="ij")
    return u.ravel(), v.ravel()


def zigzag(angles, dy):
    """A column sorted by y whose consecutive steps make the given angles with +y; x swings around 0."""
    x, y, out = 0.0, 0.0, [(0.0, 0.0, 0.0)]
    for a in angles:
        x += (-1.0 if x > 0 else 1.0) * dy * np.tan(np.radians(a))
        y += dy
        out.append((x, y, 0.0))
    return np.array(out)


def hand_columns(g):
    """name -> (points around (0, 0, 0), nominal x): each decides one rule of the column test."""
    def mix(small, large):
        a = np.concatenate([small, large])
        g.shuffle(a)
        return a
    dy = 0.003
    cols = {
        "even_below": mix(np.r_[g.uniform(5, 55, 20), 60.0], np.r_[80.0, g.uniform(80.5, 82, 20)]),   # (60 + 80) / 2 < 75
        "even_above": mix(np.r_[g.uniform(5, 55, 20), 72.0], np.r_[80.0, g.uniform(80.5, 82, 20)]),   # (72 + 80) / 2 > 75
        "odd_removed": mix(g.uniform(5, 50, 25), g.uniform(78, 82, 18)),
        "odd_kept": mix(g.uniform(5, 50, 18), g.uniform(78, 82, 25)),
        "even_clear": mix(g.uniform(5, 50, 30), g.uniform(78, 82, 12)),
    }
    return {k: zigzag(v, dy) for k, v in cols.items()}


def f32_xz(p):
    """x and z rounded to fp32-representable doubles (the file compresses); y keeps all its bits, so
    that heights in a column do not collide."""
    p = np.array(p, dtype=np.float64)
    p[:, [0, 2]] = p[:, [0, 2]].astype(np.float32).astype(np.float64)
    return p


def scene(seed, step, half, depth, wall_h):
    g = np.random.default_rng(seed)
    parts = {}
    fx, fz = grid(-half, half, 1.0, 1.0 + depth, step)
    parts["floor"] = np.c_[fx, 0.002 * g.standard_normal(len(fx)), fz]
    wx, wy = grid(-half, half, 0.0, wall_h, step)
    wy = wy + 1e-3 * g.standard_normal(len(wy))       # no two equal heights in a column
    parts["wall"] = np.c_[wx, wy, np.full(len(wx), 1.0 + depth) + 0.002 * g.standard_normal(len(wx))]
    bx, by = grid(-0.5, 0.1, 0.0, 0.5, step)
    by = by + 1e-3 * g.standard_normal(len(by))
    parts["box_front"] = np.c_[bx, by, np.full(len(bx), 1.0 + 0.45 * depth) + 0.002 * g.standard_normal(len(bx))]
    tx, tz = grid(-0.5, 0.1, 1.0 + 0.45 * depth, 1.0 + 0.45 * depth + 0.4, step)
    parts["box_top"] = np.c_[tx, 0.5 + 0.002 * g.standard_normal(len(tx)), tz]
    cur = []
    for cx in (-0.5, 0.1, -0.2):                      # thin vertical curtains behind the box edges
        yy = np.linspace(0.02, 0.9, 150) + 1e-4 * g.standard_normal(150)
        cur.append(np.c_[cx + 5e-4 * g.standard_normal(150), yy, 1.0 + 0.45 * depth + 0.6 + 5e-4 * g.standard_normal(150)])
    parts["curtains"] = np.concatenate(cur)
    parts["specks"] = np.c_[g.uniform(-half, half, 12), g.uniform(1.2, 2.0, 12), g.uniform(1.2, 1.0 + depth - 0.3, 12)]
    ball = lambda k, c: np.asarray(c) + g.uniform(-0.005, 0.005, (k, 3))   # noqa: E731
    parts["cluster19"] = ball(NB - 1, (-0.9, 1.0, 0.8))
    parts["cluster20"] = ball(NB, (0.9, 1.0, 0.8))
    parts["anchor"] = np.c_[np.zeros(60), 0.5 + 0.003 * np.arange(60), np.full(60, 0.2)]     # z_min of the cloud
    base = f32_xz(np.concatenate(list(parts.values())))
    hands = hand_columns(g)
    nominal = {k: (-1.0 + 0.4 * i, 0.5) for i, k in enumerate(hands)}
    # a 13-point column with one duplicated point, 0.02 from a dense support column in the next cell
    yy = 0.5 + 0.012 * np.arange(12)
    nan_col = np.c_[np.zeros(13), np.r_[yy[:6], yy[5], yy[6:]], np.zeros(13)]
    support = np.c_[np.zeros(60), 0.48 + 0.003 * np.arange(60), np.zeros(60)]
    return g, base, hands, nominal, nan_col, support


def assemble(base, hands, where, nan_col, support, nan_x, z):
    hp = [p + np.array([where[k][0], 0.5, where[k][1]]) for k, p in hands.items()]
    pair = [nan_col + np.array([nan_x - 0.01, 0.0, z]), support + np.array([nan_x + 0.01, 0.0, z])]
    hand = f32_xz(np.concatenate(hp + pair))
    return np.concatenate([base, hand])


def one_scene(ref, C, out, name, seed, step, half, depth, wall_h):
    g, base, hands, nominal, nan_col, support = scene(seed, step, half, depth, wall_h)
    # pass 1: nominal places -> the survivors' grid; pass 2: the hand-built columns moved to the centres of
    # their cells (the duplicated-point column and its support to either side of a cell border).  They are
    # neither at the cloud's x / z extremes nor within the radius of anything else, so the grid stays.
    pts = assemble(base, hands, nominal, nan_col, support, 1.0, 0.5)
    k1, _ = C.stray_mask(pts, NB, RADIUS)
    _, _, info = C.shadow_mask(pts[k1])
    xb, zb, cell = info["x_bins"], info["z_bins"], info["cell"]
    centre = lambda b, v: b[np.digitize(v, b) - 1] + cell / 2        # noqa: E731
    where = {k: (centre(xb, x), centre(zb, z)) for k, (x, z) in nominal.items()}
    nan_x = xb[np.digitize(1.0, xb)]
    zc = centre(zb, 0.5)
    pts = assemble(base, hands, where, nan_col, support, nan_x, zc)
    cols = g.integers(0, 256, (len(pts), 3), dtype=np.uint8)

    rk1, rk2 = ref_masks(ref, pts)
    counts = C.neighbour_counts(pts, RADIUS)
    k1, s1 = C.stray_mask(pts, NB, RADIUS)
    p1 = pts[k1]
    k2, s2, info = C.shadow_mask(p1)
    assert info["cell"] == cell and np.array_equal(info["x_bins"], xb) and np.array_equal(info["z_bins"], zb), "grid moved"
    assert np.array_equal(k1, rk1), (name, "stray mask differs from the reference", int((k1 != rk1).sum()))
    assert np.array_equal(k2, rk2), (name, "shadow mask differs from the reference", int((k2 != rk2).sum()))
    n_hand = sum(len(p) for p in hands.values()) + len(nan_col) + len(support)
    assert k1[-n_hand:].all(), "a hand-built point was removed as stray"

    meds = np.array([m for _, _, m in info["columns"]])
    angs = np.concatenate([a for _, a, _ in info["columns"]])
    assert np.nanmin(np.abs(meds - 75)) > 1e-9 and np.nanmin(np.abs(angs - 75)) > 1e-9                  # (a)
    assert np.abs(info["heights"] - 0.1).min() > 1e-9                                                     # (b)
    heads, ends, ys = info["runs"]
    for a, b in zip(heads, ends):
        assert b - a <= 16 or len(np.unique(ys[a:b])) == b - a, (name, "equal y in a column of > 16 points")   # (c)
    kinds = set()
    for _, a, m in info["columns"]:
        c = int((a < 75).sum())
        if np.isnan(m):
            kinds.add("nan")
            continue
        kinds.add("removed" if m < 75 else "kept")
        kinds.add("odd" if len(a) % 2 else "even")
        if len(a) % 2 == 0 and c == len(a) // 2:
            kinds.add("half_below" if m < 75 else "half_above")
    assert kinds >= {"removed", "kept", "odd", "even", "half_below", "half_above", "nan"}, (name, kinds)   # (d)
    assert (counts == NB - 1).any() and (counts == NB).any(), (name, "no nb - 1 / nb neighbour counts")    # (d)

    out[f"{name}_points"], out[f"{name}_colors"] = pts, cols
    out[f"{name}_stray_keep"], out[f"{name}_shadow_keep"] = rk1, rk2
    out[f"{name}_cell"] = np.array(cell)
    out[f"{name}_stray_stats"], out[f"{name}_shadow_stats"] = s1, s2
    # what the reference prints: kept / total of the stray stage, points removed / total of the shadow stage
    out[f"{name}_printed"] = np.array([rk1.sum(), len(pts), (~rk2).sum(), len(p1)], dtype=np.int64)
    print(name, "points", len(pts), "stray kept", int(rk1.sum()), "cell", cell, "columns occupied/tested/removed",
          s2[2:5], "shadow points removed", int((~rk2).sum()), "kinds", sorted(kinds))


SCENES = {
    # name: (seed, grid step, half width, floor depth, wall height)
    "room": (1, 0.03, 1.5, 3.0, 1.5),
    "closet": (2, 0.026, 1.3, 2.2, 1.2),
}


def main():
    import clean_numpy as C

    ref = lift()
    out = {"scenes": np.array(list(SCENES)), "nb_points": np.array(NB), "radius": np.array(RADIUS)}
    for name, spec in SCENES.items():
        one_scene(ref, C, out, name, *spec)
    path = os.path.join(HERE, "golden_clean.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
