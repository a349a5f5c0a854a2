"""Point-cloud views (depth_pro.render, csrc/dp_render.hip) against the rule of DESIGN.md section 22 as tests/render_numpy.py
restates it: pictures and camera records byte for byte, counts exactly.

Clipping: a row beyond the far plane cannot exist.  The bounds are taken over the rows that are drawn, so every row has
w <= dist + (sqrt(3) / 2) extent < far = dist + 3 extent; what can be clipped is a row nearer than `near` or behind the eye,
which a small zoom produces, and that is what the clipping case checks."""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import render_numpy as RN  # noqa: E402

from depth_pro import _lib  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_render.npz")
PRESETS = ("front", "top", "side", "isometric")
ALL = PRESETS + ("plan",)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


# ------------------------------------------------------------------------------------------------ CPU

def test_restatement_reproduces_its_golden_file(golden):
    res = RN.render_views(golden["points"], golden["colors"], ALL, (64, 40), 7, min_height=0.5)
    assert np.array_equal(res["image"], golden["image"])
    assert np.array_equal(res["cameras"].view(np.uint64), golden["cameras"].view(np.uint64))
    keys = RN.GLOBAL_STATS + RN.VIEW_STATS
    for k, row in zip(keys, golden["stats"]):
        assert np.ravel(res["stats"][k]).tolist() == row[:np.size(res["stats"][k])].tolist(), k
    assert 0 < min(res["stats"]["covered_pixels"]) and max(res["stats"]["covered_pixels"]) < 64 * 40
    sheet = RN.render_views(golden["points"], None, RN.SHEET, (16, 9), 3, sheet=True)["image"]
    assert sheet.shape == (18, 32, 3) and np.array_equal(sheet, golden["sheet"])


def _matrix_camera(pts, view, W, H):
    """An independent statement of the same camera: a 4 x 4 look-at and a 4 x 4 perspective matrix, one matmul."""
    front, up, zoom = (np.asarray(view[0], float), np.asarray(view[1], float), float(view[2]))
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    centre, extent = 0.5 * (lo + hi), float((hi - lo).max())
    t = np.tan(np.pi / 6.0)
    f = front / np.linalg.norm(front)
    eye = centre + f * (zoom * extent / t)
    fwd = -f
    s = np.cross(fwd, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, fwd)
    look = np.eye(4)
    look[0, :3], look[1, :3], look[2, :3] = s, u, -fwd
    look[:3, 3] = -look[:3, :3] @ eye
    dist = zoom * extent / t
    near, far = max(0.01 * extent, dist - 3.0 * extent), dist + 3.0 * extent
    proj = np.zeros((4, 4))
    proj[0, 0], proj[1, 1] = 1.0 / (t * W / H), 1.0 / t
    proj[2, 2], proj[2, 3], proj[3, 2] = -(far + near) / (far - near), -2.0 * far * near / (far - near), -1.0
    clip = np.concatenate([pts, np.ones((len(pts), 1))], axis=1) @ (proj @ look).T
    ndc = clip[:, :3] / clip[:, 3:4]
    fx, fy = (ndc[:, 0] * 0.5 + 0.5) * W, (0.5 - ndc[:, 1] * 0.5) * H
    return fx, fy, np.abs(ndc[:, 2]) <= 1.0


@pytest.mark.parametrize("name", PRESETS)
def test_restatement_agrees_with_a_matrix_camera(golden, name):
    pts = golden["points"]
    for W, H in ((64, 40), (1280, 720)):
        ok, px, py = RN.centre_pixels(pts, name, W, H)
        fx, fy, inside = _matrix_camera(pts, RN.VIEW_PRESETS[name], W, H)
        near_edge = (np.abs(fx - np.rint(fx)) < 1e-9) | (np.abs(fy - np.rint(fy)) < 1e-9)
        assert near_edge.mean() == 0.0                          # the golden scene has no point that close to a boundary
        qx, qy = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
        assert np.array_equal(ok, inside & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)) and ok.mean() > 0.5
        assert np.array_equal(px[ok], qx[ok]) and np.array_equal(py[ok], qy[ok])


def test_orientation_facts():
    box = np.array([[-1.0, -0.5, 2.0], [1.5, 2.0, 6.0]])
    centre = box.mean(axis=0)
    for name in PRESETS:
        for W, H in ((1280, 720), (131, 67), (64, 40)):
            ok, px, py = RN.centre_pixels(np.vstack([box, centre]), name, W, H)
            assert ok[2] and (px[2], py[2]) == (W // 2, H // 2), (name, W, H)
    # front: +x is left, +y is up
    pts = np.vstack([box, centre, centre + [0.5, 0.0, 0.0], centre + [0.0, 0.5, 0.0]])
    ok, px, py = RN.centre_pixels(pts, "front", 640, 360)
    assert ok[2:].all() and px[3] < px[2] and py[3] == py[2] and py[4] < py[2] and px[4] == px[2]
    pts = np.vstack([box, centre + [0.0, -0.5, 0.0], centre + [0.0, 0.5, 0.0]])
    cols = np.array([[1, 1, 1], [2, 2, 2], [10, 20, 30], [40, 50, 60]], np.uint8)
    # plan: x is flipped, z increases upwards, the highest point wins
    res = RN.render_views(pts, cols, ("plan",), (64, 40), 1)
    (ok, px, py) = RN.centre_pixels(pts, "plan", 64, 40)
    assert px[0] > px[1] and py[0] > py[1] and tuple(res["image"][0, py[3], px[3]]) == (40, 50, 60)
    assert tuple(res["image"][0, 0, 0]) == RN.PLAN_BACKGROUND


def test_top_view_the_highest_point_hides_the_one_below_it():
    """`top` looks down on a cloud whose y points up: front = [0, 1, 0], so eye = centre + f * dist stands above it.  (The
    reference's table has [0, -1, 0], which with the same rule looks up from under the floor)"""
    box = np.array([[-1.0, -0.5, 2.0], [1.5, 2.0, 6.0]])
    centre = box.mean(axis=0)
    pts = np.vstack([box, centre + [0.0, -0.5, 0.0], centre + [0.0, 0.5, 0.0]])
    cols = np.array([[1, 1, 1], [2, 2, 2], [10, 20, 30], [40, 50, 60]], np.uint8)
    res = RN.render_views(pts, cols, ("top",), (64, 40), 7)
    assert res["cameras"][0][3] > box[1, 1] and tuple(res["cameras"][0][11:14]) == (0.0, -1.0, 0.0)      # the eye above, looking down
    assert (res["image"][0] != 255).any(axis=-1).sum() >= 49            # the two splats coincide: one of them is hidden
    assert tuple(res["image"][0, 20, 32]) == (40, 50, 60)
    assert (res["image"][0] == (40, 50, 60)).all(axis=-1).sum() == 49 and not (res["image"][0] == (10, 20, 30)).all(axis=-1).any()


def test_argument_errors_come_back_before_launch():
    """Every bad argument is DP_ERR_ARG from the host: a null stream and no device here, a launch would be a HIP error."""
    lib = _lib.load()
    ARG, P = 1000, 4096
    nan, inf = float("nan"), float("inf")
    f64, u8 = ctypes.c_double, ctypes.c_uint8
    front = [0.0, 0.0, -1.0, 0.0, 1.0, 0.0, 0.4]
    ws = lib.dp_render_workspace_size(64, 40, 7, 5)
    assert ws >= 256 + 5 * 8 * 46 * 70 and lib.dp_render_workspace_size(64, 40, 7, 1) < ws

    def points(pts=P, cols=P, cnt=P, n=100, views=front, nv=1, plan=0, mh=0.0, W=64, H=40, size=7, bg=(255,) * 6, t=RN.TAN_HALF_FOV,
               sheet=0, img=P, cams=P, stats=P, wsp=P, wb=ws):
        v = None if views is None else (f64 * len(views))(*views)
        b = None if bg is None else (u8 * 6)(*bg)
        return lib.dp_render_points(pts, cols, cnt, n, v, nv, plan, mh, W, H, size, b, t, sheet, img, cams, stats, wsp, wb, None)

    def cameras(pts=P, cnt=P, n=100, views=front, nv=1, plan=0, mh=0.0, W=64, H=40, t=RN.TAN_HALF_FOV, cams=P, stats=P, wsp=P, wb=256):
        v = None if views is None else (f64 * len(views))(*views)
        return lib.dp_render_cameras(pts, cnt, n, v, nv, plan, mh, W, H, t, cams, stats, wsp, wb, None)

    for name in ("pts", "views", "bg", "img", "cams", "stats", "wsp"):
        assert points(**{name: None}) == ARG, name
    for name in ("pts", "views", "cams", "stats", "wsp"):
        assert cameras(**{name: None}) == ARG, name
    for fn in (points, cameras):
        for dims in (dict(W=0), dict(H=0), dict(W=-3), dict(W=1 << 16, H=1 << 15), dict(W=46341, H=46341)):
            assert fn(**dims) == ARG, (fn.__name__, dims)
        assert fn(views=front * 5, nv=5) == ARG and fn(nv=0) == ARG and fn(nv=-1) == ARG and fn(n=-1) == ARG
        for k in range(7):
            for bad in (nan, inf, -inf):
                assert fn(views=front[:k] + [bad] + front[k + 1:]) == ARG, (k, bad)
        assert fn(views=[0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.4]) == ARG                      # a zero front
        assert fn(views=[0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.4]) == ARG                     # a zero up
        assert fn(views=front[:6] + [0.0]) == ARG                                        # a zero zoom
        assert fn(views=[0.0, 0.0, -1.0, 0.0, 0.0, 2.5, 0.4]) == ARG                     # up parallel to front
        assert fn(views=[1.0, -1.0, -1.0, -2.0, 2.0, 2.0, 0.35]) == ARG
        assert fn(views=front + [0.0] * 7, nv=2) == ARG                                  # the second view
        for bad in (nan, inf, -inf):
            assert fn(plan=2, mh=bad) == ARG and fn(t=bad) == ARG, bad
        assert fn(plan=3) == ARG and fn(t=0.0) == ARG
        assert fn(wsp=P + 4) == ARG and fn(wb=0) == ARG
    for size in (0, 2, 6, 16, 17, -1):
        assert points(size=size) == ARG and lib.dp_render_workspace_size(64, 40, size, 1) == 0, size
    assert points(wb=ws - 1, plan=1, views=front * 4, nv=4) == ARG
    assert points(wb=lib.dp_render_workspace_size(64, 40, 7, 1), W=128) == ARG              # the workspace of a smaller picture
    assert points(sheet=1) == ARG and points(sheet=1, views=front * 4, nv=4, plan=1) == ARG
    assert lib.dp_render_workspace_size(0, 40, 7, 1) == 0 and lib.dp_render_workspace_size(64, 40, 7, 6) == 0
    assert _lib.DP_ABI_VERSION == 20 and _lib.DP_RENDER_STATS == 4 + 4 * 5


def test_python_argument_checks_need_no_device():
    import torch

    from depth_pro import render as R

    assert R.VIEW_PRESETS == RN.VIEW_PRESETS and R.SHEET == RN.SHEET and R.TAN_HALF_FOV == RN.TAN_HALF_FOV
    assert R.GLOBAL_STATS == RN.GLOBAL_STATS and R.VIEW_STATS == RN.VIEW_STATS and R.PLAN_BACKGROUND == RN.PLAN_BACKGROUND
    with pytest.raises(_lib.DPError, match="dp_render.hip"):
        R.render_views(torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(ValueError):
        R._views(("front", "above"))
    with pytest.raises(ValueError):
        R._views(())


def test_stage_list_with_and_without_the_new_options(tmp_path):
    import generate_depth_maps as G

    o = dict(output_dir=str(tmp_path))
    names = [st.name for st in G.STAGES]
    st = G.STAGES[names.index("views")]
    assert names.index("clean") < names.index("views") and st.implies == "cloud" and st.suffixes == ("_view.png", "_view.json")
    # without the options the lists are those of today
    assert G.resolve_stages(**o) == {}
    assert list(G.resolve_stages(**o, pointcloud=True)) == ["cloud"]
    assert list(G.resolve_stages(**o, floor_polygons=True, floor_slices=5)) == ["cloud", "ground", "clean", "floor", "slices", "polygons"]
    assert list(G.resolve_stages(**o, simple_mesh=True, fit_shapes=True, anaglyph=True, parallax="zoom", depth_shadows=True)) == \
        ["shadows", "cloud", "ground", "clean", "cluster", "shapes", "mesh", "trimesh", "anaglyph", "parallax"]
    G.resolve_stages(**o, render_size="axb", render_point_size=4, render_min_height=float("nan"))       # off: not looked at
    got = G.resolve_stages(**o, render_view="multi")
    assert list(got) == ["cloud", "views"]
    assert got["views"] == {"view": "multi", "views": RN.SHEET, "sheet": True, "size": (1280, 720), "point_size": 7, "min_height": None}
    got = G.resolve_stages(**o, render_view="plan", render_size="320x200", render_point_size=3, render_min_height=1.3, clean_pointcloud=True)
    assert list(got) == ["cloud", "ground", "clean", "views"]
    assert got["views"] == {"view": "plan", "views": ("plan",), "sheet": False, "size": (320, 200), "point_size": 3, "min_height": 1.3}
    assert G.resolve_stages(**o, render_view="top", render_min_height=1.0)["views"]["min_height"] is None   # the plan's only
    for bad in (dict(render_view="below"), dict(render_view="top", render_size="0x10"), dict(render_view="top", render_size="12"),
                dict(render_view="top", render_point_size=4), dict(render_view="top", render_point_size=17),
                dict(render_view="plan", render_min_height=float("inf"))):
        with pytest.raises(ValueError):
            G.resolve_stages(**o, **bad)
    stages = {"views": {}}
    (tmp_path / "a_depth.png").write_bytes(b"")
    (tmp_path / "a_view.png").write_bytes(b"")
    assert G.plan_frames(["/in/a.png"], str(tmp_path), 1, 0, True, stages=stages) == [0]
    (tmp_path / "a_view.json").write_bytes(b"")
    assert G.plan_frames(["/in/a.png"], str(tmp_path), 1, 0, True, stages=stages) == []


# ------------------------------------------------------------------------------------------------ GPU

def _compare(cuda, pts, cols=None, views=ALL, size=(64, 40), point_size=7, count=None, min_height=None, sheet=False,
             background=(255, 255, 255)):
    import torch

    from depth_pro import render as R

    want = RN.render_views(pts, cols, views, size, point_size, background, count, sheet, min_height)
    p = torch.from_numpy(np.ascontiguousarray(pts, np.float64).reshape(-1, 3)).to(cuda)
    c = None if cols is None else torch.from_numpy(np.ascontiguousarray(cols)).to(cuda)
    res = R.render_views(p, c, views, size, point_size, background, count, sheet, min_height)
    cams, stats = R.cameras(p, views, size, count, min_height)
    got = R.render_summary(res)
    assert got["image"].shape == want["image"].shape and got["image"].dtype == np.uint8
    assert np.array_equal(got["cameras"].view(np.uint64), want["cameras"].view(np.uint64))
    assert np.array_equal(cams.cpu().numpy().view(np.uint64), want["cameras"].view(np.uint64))
    assert got["stats"] == want["stats"], (got["stats"], want["stats"])
    alone = R.stats_dict(stats.cpu().numpy(), 0)
    assert {k: alone[k] for k in RN.GLOBAL_STATS} == {k: want["stats"][k] for k in RN.GLOBAL_STATS}
    assert np.array_equal(got["image"], want["image"]), int((got["image"] != want["image"]).any(axis=-1).sum())
    return want


@pytest.fixture(scope="module")
def cloud():
    return RN.scene(5000, 11)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(1, 1), (16, 9), (64, 40), (131, 67)])
@pytest.mark.parametrize("point_size", [1, 7, 15])
def test_image_and_splat_sizes(cuda, cloud, size, point_size):
    want = _compare(cuda, *cloud, size=size, point_size=point_size, min_height=0.3)
    assert want["stats"]["live"] == 5000 and all(c > 0 for c in want["stats"]["covered_pixels"])


@pytest.mark.gpu
@pytest.mark.parametrize("count", [0, 1, 2, 63, 64, 65])
def test_point_counts(cuda, cloud, count):
    pts, cols = cloud
    want = _compare(cuda, pts[:count], cols[:count])
    assert want["stats"]["degenerate"] == int(count < 2) and want["stats"]["live"] == count
    if count < 2:
        assert (want["image"][:4] == 255).all() and want["stats"]["drawn"][:4] == [0] * 4


@pytest.mark.gpu
def test_count_smaller_than_n_with_junk_behind_it(cuda, cloud):
    pts, cols = cloud
    junk = np.vstack([pts[:700], np.full((40, 3), 1e300), np.full((40, 3), np.nan), -pts[:40] * 1e6])
    jc = np.vstack([cols[:700], np.full((120, 3), 9, np.uint8)])
    import torch
    want = _compare(cuda, junk, jc, count=700)
    assert np.array_equal(want["image"], RN.render_views(pts[:700], cols[:700], ALL, (64, 40), 7)["image"])
    _compare(cuda, junk, jc, count=torch.tensor(700, dtype=torch.int32, device=cuda))
    _compare(cuda, junk, jc, count=10 ** 6)                                 # clamped to N: the junk is drawn like any row


@pytest.mark.gpu
def test_duplicated_points_the_lower_row_wins(cuda, cloud):
    pts, cols = cloud
    rng = np.random.default_rng(5)
    p = np.vstack([pts[:500], pts[:500], pts[:500]])
    c = rng.integers(0, 256, (1500, 3), dtype=np.uint8)
    want = _compare(cuda, p, c, point_size=1)
    shown = {tuple(v) for v in want["image"][0][(want["image"][0] != 255).any(axis=-1)]}
    assert shown <= {tuple(v) for v in c[:500]}


@pytest.mark.gpu
def test_all_rows_in_one_pixel(cuda):
    rng = np.random.default_rng(6)
    p = np.vstack([[[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]], np.tile([[0.25, 0.125, 0.5]], (6000, 1))])
    c = rng.integers(0, 256, (6002, 3), dtype=np.uint8)
    want = _compare(cuda, p, c, point_size=1)
    assert want["stats"]["drawn"][0] >= 6000 and (want["image"][0] == c[2]).all(axis=-1).sum() == 1     # the lowest row's colour
    _compare(cuda, p, c, point_size=7)


@pytest.mark.gpu
@pytest.mark.parametrize("point_size", [1, 7, 15])
def test_splat_reach_past_every_edge(cuda, point_size):
    """Centres exactly (size - 1) / 2 pixels outside an edge still reach the picture, (size + 1) / 2 do not."""
    W, H, R = 64, 40, (point_size - 1) // 2
    view = ((0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 0.2)
    anchors = np.array([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])
    s = np.linspace(-0.99, 0.99, 6001)
    cand = np.vstack([np.stack([s, 0.013 * np.ones_like(s), np.zeros_like(s)], 1), np.stack([0.017 * np.ones_like(s), s, np.zeros_like(s)], 1)])
    ok, fx, fy = RN._project(*_cam_args(np.vstack([anchors, cand]), view, W, H), 33)[:3]     # centres up to 16 pixels outside
    fx, fy = np.where(ok, fx, -99), np.where(ok, fy, -99)
    keep = [0, 1]
    for target, axis, other, mid in ((-R, fx, fy, H // 2), (-R - 1, fx, fy, H // 2), (W - 1 + R, fx, fy, H // 2), (W + R, fx, fy, H // 2),
                                     (-R, fy, fx, W // 2), (-R - 1, fy, fx, W // 2), (H - 1 + R, fy, fx, W // 2), (H + R, fy, fx, W // 2)):
        hit = np.nonzero((axis == target) & (np.abs(other - mid) <= 2))[0]
        assert len(hit), target
        keep += hit[:3].tolist()
    pts = np.vstack([anchors, cand])[keep]
    cols = np.random.default_rng(8).integers(0, 255, (len(pts), 3), dtype=np.uint8)
    want = _compare(cuda, pts, cols, views=(view,), size=(W, H), point_size=point_size)
    assert want["stats"]["outside"][0] >= 12 and want["stats"]["drawn"][0] >= 12
    img = want["image"][0]
    edge = np.concatenate([img[0], img[-1], img[:, 0], img[:, -1]])
    assert (edge != 255).any(axis=-1).sum() >= 4                            # the reaching splats show on all four edges


def _cam_args(pts, view, W, H):
    p, fin = RN.live_rows(pts)
    return p, fin, RN.perspective_camera(p, fin, view, W, H), W, H


@pytest.mark.gpu
def test_rows_behind_the_eye_and_before_the_near_plane_are_clipped(cuda, cloud):
    pts, cols = cloud
    views = tuple((f, u, 0.05) for f, u, _ in (RN.VIEW_PRESETS[n] for n in PRESETS))
    want = _compare(cuda, pts, cols, views=views)
    assert all(c > 0 for c in want["stats"]["clipped"]) and all(d > 0 for d in want["stats"]["drawn"])
    cam = want["cameras"][0]
    w = (pts - cam[2:5]) @ cam[11:14]
    assert (w < 0).any() and ((w > 0) & (w < cam[14])).any() and not (w > cam[15]).any()


@pytest.mark.gpu
def test_non_finite_rows(cuda, cloud):
    pts, cols = cloud
    p = pts[:900].copy()
    p[10] = np.nan
    p[11, 1] = np.inf
    p[12, 2] = -np.inf
    p[13] = [np.inf, -np.inf, np.nan]
    want = _compare(cuda, p, cols[:900], min_height=0.2)
    assert want["stats"]["nonfinite"] == 4 and want["stats"]["error"] == 1 and want["stats"]["live"] == 900
    only = _compare(cuda, np.full((5, 3), np.nan), cols[:5])
    assert only["stats"]["degenerate"] == 1 and only["stats"]["nonfinite"] == 5


@pytest.mark.gpu
def test_no_colours_and_another_background(cuda, cloud):
    want = _compare(cuda, cloud[0], None, background=(10, 200, 30))
    assert {tuple(v) for v in want["image"][0].reshape(-1, 3)} == {(128, 128, 128), (10, 200, 30)}
    assert {tuple(v) for v in want["image"][4].reshape(-1, 3)} == {(128, 128, 128), RN.PLAN_BACKGROUND}


@pytest.mark.gpu
def test_four_views_in_one_call_equal_four_calls_and_the_sheet(cuda, cloud):
    import torch

    from depth_pro import render as R

    p, c = (torch.from_numpy(a).to(cuda) for a in cloud)
    size = (131, 67)
    multi = R.render_summary(R.render_views(p, c, RN.SHEET, size, 7))
    singles = [R.render_summary(R.render_views(p, c, (n,), size, 7)) for n in RN.SHEET]
    for k, one in enumerate(singles):
        assert np.array_equal(one["image"][0], multi["image"][k])
        assert np.array_equal(one["cameras"][0].view(np.uint64), multi["cameras"][k].view(np.uint64))
        assert all(one["stats"][s][0] == multi["stats"][s][k] for s in RN.VIEW_STATS)
    sheet = R.render_summary(R.render_views(p, c, RN.SHEET, size, 7, sheet=True))
    im = multi["image"]
    assert np.array_equal(sheet["image"], np.vstack([np.hstack([im[0], im[1]]), np.hstack([im[2], im[3]])]))
    assert sheet["stats"] == multi["stats"]
    _compare(cuda, *cloud, views=RN.SHEET, size=size, sheet=True)


@pytest.mark.gpu
def test_plan_view(cuda, cloud):
    pts, cols = cloud
    for size in ((64, 40), (131, 67), (1, 1)):
        for ps in (1, 7):
            a = _compare(cuda, pts, cols, views=("plan",), size=size, point_size=ps)
            b = _compare(cuda, pts, cols, views=("plan",), size=size, point_size=ps, min_height=1.0)
            assert a["stats"]["clipped"] == [0] and 0 < b["stats"]["clipped"][0] < 5000
    flat = pts.copy()
    flat[:, 0] = 0.75                                                       # a zero span in x counts as 1
    z = _compare(cuda, flat, cols, views=("plan",))
    assert (z["image"][0][:, :28] == 240).all() and z["cameras"][0][1] == 0.0
    below = _compare(cuda, pts, cols, views=("plan", "front"), min_height=100.0)
    assert (below["image"][1] == 240).all() and below["cameras"][1][1] == 1.0 and below["stats"]["drawn"][1] == 0   # a degenerate view counts nothing
    assert below["stats"]["degenerate"] == 0 and below["stats"]["covered_pixels"][0] > 0
    _compare(cuda, pts[:1], cols[:1], views=("plan",), point_size=3)        # one row: both spans are 0, the point is drawn


@pytest.mark.gpu
def test_contention_at_size(cuda):
    pts, cols = RN.scene(200000, 12)
    want = _compare(cuda, pts, cols, views=RN.SHEET, size=(1280, 720), point_size=7, sheet=True)
    assert want["image"].shape == (1440, 2560, 3) and min(want["stats"]["drawn"]) > 100000
