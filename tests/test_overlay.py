"""Shape overlays on the plan view (depth_pro.overlay, csrc/dp_overlay.hip) against the rule of DESIGN.md section 23 as
tests/overlay_numpy.py restates it.

The GPU is checked in two steps, so that the device's own sin and cos cannot blur the picture check: its records against
the restatement's (integers, colours and numbers equal, reals within 4 ulp, a box off by at most one pixel and only in a
record whose reals differ), then the picture byte for byte and the counts exactly against the restatement's `draw` over
the DEVICE's records.  Lists whose angles are all 0 (cos 1 and sin 0 exactly on both sides) are also checked through the
whole chain against the restatement's own records."""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import overlay_numpy as ON  # noqa: E402
import render_numpy as RN  # noqa: E402

from depth_pro import _lib  # noqa: E402


def _rects(rows):
    out = np.zeros((len(rows), 8))
    out[:, :5] = np.asarray(rows, np.float64).reshape(-1, 5)
    return out


def _table(circles, K=None, gaps=()):
    """A shapes table whose kind-2 rows hold `circles` (xc, yc, r); rows listed in `gaps` are kind-1 rows between them."""
    K = len(circles) + len(gaps) if K is None else K
    t = np.zeros((K, 16))
    it = iter(circles)
    for c in range(len(circles) + len(gaps)):
        if c in gaps:
            t[c, 0], t[c, 2:7] = 1.0, (0.0, 0.0, 1.0, 1.0, 10.0)
        else:
            t[c, 0], t[c, 8:11] = 2.0, next(it)
    return t


# ------------------------------------------------------------------------------------------------ CPU

def test_axis_aligned_rectangle_counts_and_corners():
    """a = 10, b = 5, t = 1 at the centre pixel (20, 15) of a 41 x 31 picture: the stroke is the 23 x 13 block without
    the 17 x 7 block inside it."""
    W, H = 41, 31
    cam = ON.plan_camera(0.0, 0.0, 1.0, W, H)
    img = np.full((H, W, 3), 200, np.uint8)
    res = ON.draw_shapes(img, cam, _rects([[0.0, 0.0, 20.0, 10.0, 0.0]]), stroke=2.0, alpha=255, label_scale=0)
    on = (res["image"] != 200).any(axis=-1)
    assert on.sum() == 23 * 13 - 17 * 7 == 180 and res["stats"]["pixels_painted"] == 180
    assert res["stats"] == {**{k: 0 for k in ON.STATS}, "rectangles": 1, "pixels_painted": 180}
    for i, j in ((9, 9), (31, 9), (9, 21), (31, 21)):
        assert tuple(res["image"][j, i]) == (0x42, 0x85, 0xF4), (i, j)
    for i, j in ((8, 9), (9, 8), (32, 21), (31, 22), (12, 12), (28, 18), (20, 15)):
        assert not on[j, i], (i, j)
    assert on[11, 11] and on[15, 11] and on[15, 9] and not on[15, 12]
    r = res["records"][0]
    assert r.tolist() == [1.0, 1.0, 20.0, 15.0, 10.0, 5.0, 1.0, 0.0, float(0x42 + 256 * 0x85 + 65536 * 0xF4), 1.0,
                          9.0, 9.0, 31.0, 21.0, 0.0, 0.0, -1.0, -1.0, 0.0, 0.0]
    # angle is counter-clockwise in (u, v), v up: the long side of a 30 degree rectangle rises to the right
    tilt = (ON.draw_shapes(img, cam, _rects([[0.0, 0.0, 30.0, 2.0, 30.0]]), stroke=2.0, alpha=255, label_scale=0)["image"] != 200).any(axis=-1)
    assert tilt[15 - 6, 20 + 10] and tilt[15 + 6, 20 - 10] and not tilt[15 + 6, 20 + 10] and not tilt[15 - 6, 20 - 10]


def test_circle_smaller_than_half_the_stroke_is_a_disc():
    W, H = 21, 21
    cam = ON.plan_camera(0.0, 0.0, 1.0, W, H)
    img = np.zeros((H, W, 3), np.uint8)
    res = ON.draw_shapes(img, cam, shapes=_table([(0.0, 0.0, 1.0)]), stroke=6.0, alpha=255, label_scale=0)
    on = (res["image"] != 0).any(axis=-1)
    yy, xx = np.mgrid[0:H, 0:W]
    assert on.sum() == 49 and np.array_equal(on, (xx - 10) ** 2 + (yy - 10) ** 2 <= 16)       # R + t = 4, R - t < 0
    assert tuple(res["image"][10, 10]) == (0x34, 0x98, 0xDB) and res["stats"]["circles"] == 1
    ring = (ON.draw_shapes(img, cam, shapes=_table([(0.0, 0.0, 5.0)]), stroke=2.0, alpha=255, label_scale=0)["image"] != 0).any(axis=-1)
    assert np.array_equal(ring, ((xx - 10) ** 2 + (yy - 10) ** 2 <= 36) & ((xx - 10) ** 2 + (yy - 10) ** 2 >= 16))
    point = ON.draw_shapes(img, cam, shapes=_table([(0.0, 0.0, 0.0)]), stroke=1.0, alpha=255, label_scale=0)      # r = 0
    assert (point["image"] != 0).any(axis=-1).sum() == 1 and point["image"][10, 10].any()


def test_blend_formula():
    p, c = np.arange(256), np.arange(256)[::-1]
    assert np.array_equal(ON.blend(p, c, 0), p) and np.array_equal(ON.blend(p, c, 255), c)
    assert ON.blend(240, 66, 230) == (230 * 66 + 25 * 240 + 127) // 255 == 21307 // 255 == 83
    assert ON.blend(240, 255, 179) == (179 * 255 + 76 * 240 + 127) // 255 == 251
    W, H = 9, 9
    res = ON.draw_shapes(np.full((H, W, 3), 240, np.uint8), ON.plan_camera(0.0, 0.0, 1.0, W, H), shapes=_table([(0.0, 0.0, 0.0)]),
                         stroke=1.0, label_scale=0)
    assert tuple(res["image"][4, 4]) == (ON.blend(240, 0x34, 230), ON.blend(240, 0x98, 230), ON.blend(240, 0xDB, 230))
    twice = ON.draw_shapes(np.full((H, W, 3), 240, np.uint8), ON.plan_camera(0.0, 0.0, 1.0, W, H),
                           shapes=_table([(0.0, 0.0, 0.0), (0.0, 0.0, 0.0)]), stroke=1.0, label_scale=0)
    assert twice["image"][4, 4, 0] == ON.blend(ON.blend(240, 0x34, 230), 0x2E, 230)          # every covering shape in turn


GLYPHS = {"1": ("..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."),
          "0": (".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."),
          "9": (".###.", "#...#", "#...#", ".####", "....#", "...#.", ".##..")}


def _block(text, L):
    rows = [".".join(GLYPHS[ch][r] for ch in text) for r in range(7)]
    cells = np.array([[ch == "#" for ch in row] for row in rows])
    return np.repeat(np.repeat(cells, L, axis=0), L, axis=1)


@pytest.mark.parametrize("number,L", [(10, 1), (10, 2), (9999, 1), (9999, 3)])
def test_digit_block_pixel_for_pixel(number, L):
    """The label of the `number`-th rectangle, alone on the picture: box, block and digits where the rule puts them."""
    W, H = 101, 41
    cam = ON.plan_camera(0.0, 0.0, 1.0, W, H)
    rects = _rects([[1e6, 0.0, 0.0, 0.0, 0.0]] * (number - 1) + [[0.0, 0.0, 0.0, 0.0, 0.0]])
    res = ON.draw_shapes(np.full((H, W, 3), 40, np.uint8), cam, rects, stroke=1.0, alpha=0, label_scale=L)      # alpha 0: no stroke shows
    want = _block(str(number), L)
    bh, bw = want.shape
    assert (bw, bh) == ((6 * len(str(number)) - 1) * L, 7 * L) and np.array_equal(want, ON.digit_block(number, L))
    x0, y0 = 50 - bw // 2, 20 - bh // 2
    colour = tuple(ON.palette()[(number - 1) % 8])
    white = ON.blend(40, 255, 179)
    expect = np.full((H, W, 3), 40, np.uint8)
    expect[y0 - L:y0 + bh + L, x0 - L:x0 + bw + L] = white
    expect[y0:y0 + bh, x0:x0 + bw][want] = colour
    assert np.array_equal(res["image"], expect)
    assert res["stats"]["pixels_painted"] == (bw + 2 * L) * (bh + 2 * L) and res["stats"]["offscreen"] == number - 1
    assert res["records"][-1][14:19].tolist() == [x0 - L, y0 - L, x0 + bw - 1 + L, y0 + bh - 1 + L, len(str(number))]


def test_restatement_counts_skips_and_degenerate_cameras():
    cam = ON.plan_camera(0.25, -0.5, 3.0, 67, 35)
    nan, inf = np.nan, np.inf
    rows = [[0, 0, 2, 1, 10], [nan, 0, 2, 1, 10], [0, inf, 2, 1, 10], [0, 0, -1, 1, 10], [0, 0, 1, -2, 10], [0, 0, 1, 1, nan],
            [0, 0, 1e308, 1, 0], [500, 0, 1, 1, 0]]
    t = _table([(0, 0, 2), (0, 0, -1), (nan, 0, 1), (0, 0, inf), (0, -400, 1)])
    recs, stats = ON.records(cam, _rects(rows), None, t, None, (67, 35))
    assert stats == {**{k: 0 for k in ON.STATS}, "rectangles": 1, "circles": 1, "skipped": 9, "offscreen": 2, "error": 1}
    assert recs[:, 9].tolist() == list(range(1, 14)) and recs[8:, 0].tolist() == [2.0] * 5
    assert (recs[[1, 2, 3, 4, 5, 6, 9, 10, 11], 1] == 8).all() and (recs[[7, 12], 1] == 0).all()
    for bad in (ON.plan_camera(0, 0, 1, 67, 35, degenerate=1.0), ON.plan_camera(nan, 0, 1, 67, 35), ON.plan_camera(0, 0, inf, 67, 35),
                np.zeros(24)):
        recs, stats = ON.records(bad, _rects(rows), None, t, None, (67, 35))
        assert len(recs) == 0 and stats == {**{k: 0 for k in ON.STATS}, "error": 2}
    assert ON.records(cam, _rects(rows), 3, t, 1, (67, 35))[0][:, 9].tolist() == [1, 2, 3, 4]           # counts cut both lists
    # finite R and t whose sum is not: the box has no finite side, the shape is skipped, not called off-screen
    recs, stats = ON.records(cam, _rects([[0, 0, 2, 1, 10]]), None, _table([(0, 0, 5.9e307)]), None, (67, 35), stroke=1e308)
    assert recs[:, 1].tolist() == [3.0, 8.0] and np.isfinite(5.9e307 * 3.0) and stats["skipped"] == 1 and stats["offscreen"] == 0
    assert len(ON.records(cam, _rects(rows), -2, t, 0, (67, 35))[0]) == 0


def test_palettes_and_constants_agree_with_the_package():
    from depth_pro import overlay as OV

    assert OV.RECT_PALETTE == ON.RECT_PALETTE and OV.CIRCLE_PALETTE == ON.CIRCLE_PALETTE and OV.STATS == ON.STATS
    assert OV._rgb(OV.RECT_PALETTE) + OV._rgb(OV.CIRCLE_PALETTE) == ON.palette().reshape(-1).tolist()
    assert _lib.DP_OVERLAY_RECORD_DOUBLES == ON.RECORD_DOUBLES == len(OV.RECORD_COLUMNS) and _lib.DP_ABI_VERSION == 20
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dp_mi355x.h")).read()
    font = header.split("#define DP_OVERLAY_FONT", 1)[1].split("int64_t dp_overlay_workspace_size", 1)[0]
    assert [int(v) for v in font.replace("{", " ").replace("}", " ").replace(",", " ").replace("\\", " ").split()] == \
        [v for g in ON.FONT for v in g]
    assert f"#define DP_OVERLAY_LABEL_ALPHA      {ON.LABEL_ALPHA}" in header


def _call(lib, img=4096, W=64, H=40, cam=4096, rects=4096, nr=4096, mr=10, shapes=4096, nc=4096, mc=10, pal=True, stroke=3.0,
          alpha=230, L=2, rec=4096, stats=4096, ws=4096, wb=None, stream=None):
    p = (ctypes.c_uint8 * 48)(*ON.palette().reshape(-1).tolist()) if pal else None
    wb = lib.dp_overlay_workspace_size(max(mr, 0), max(mc, 0)) if wb is None else wb
    return lib.dp_overlay_shapes(img, W, H, cam, rects, nr, mr, shapes, nc, mc, p, stroke, alpha, L, rec, stats, ws, wb, stream)


BAD_ARGUMENTS = [dict(img=None), dict(cam=None), dict(pal=False), dict(rec=None), dict(stats=None), dict(ws=None), dict(rects=None),
                 dict(shapes=None), dict(cam=4100), dict(rects=4100), dict(shapes=4100), dict(rec=4100), dict(stats=4100), dict(ws=4100),
                 dict(nr=4098), dict(nc=4097), dict(W=0), dict(H=0), dict(W=-5), dict(W=1 << 16, H=1 << 15), dict(W=46341, H=46341),
                 dict(stroke=0.0), dict(stroke=-1.0), dict(stroke=float("nan")), dict(stroke=float("inf")), dict(alpha=-1),
                 dict(alpha=256), dict(L=-1), dict(L=9), dict(mr=-1), dict(mc=-1), dict(mr=(1 << 31) - 1, mc=1), dict(wb=0),
                 dict(mr=5000, mc=5000, wb=256 + 256)]


def test_argument_errors_come_back_before_launch():
    """Every bad argument is DP_ERR_ARG from the host: a null stream and no device here, a launch would be a HIP error."""
    lib = _lib.load()
    for bad in BAD_ARGUMENTS:
        assert _call(lib, **bad) == 1000, bad
    assert lib.dp_overlay_workspace_size(-1, 0) == 0 and lib.dp_overlay_workspace_size(0, -1) == 0
    assert lib.dp_overlay_workspace_size(0, 0) == 256 and lib.dp_overlay_workspace_size(1 << 30, 1 << 30) == 0
    assert lib.dp_overlay_workspace_size(10, 5000) >= 256 + 5000 + 4 * 3 and lib.dp_overlay_workspace_size(10 ** 6, 0) == 256
    assert _call(lib, wb=lib.dp_overlay_workspace_size(10, 10) - 1) == 1000


def test_python_argument_checks_need_no_device():
    import torch

    from depth_pro import overlay as OV

    with pytest.raises(_lib.DPError, match="dp_overlay.hip"):
        OV.draw_shapes(torch.zeros(4, 4, 3, dtype=torch.uint8), torch.zeros(24, dtype=torch.float64))
    assert OV.stats_dict(np.arange(8.0)) == dict(zip(ON.STATS, range(8)))


def test_stage_list_with_and_without_the_new_option(tmp_path):
    import generate_depth_maps as G

    o = dict(output_dir=str(tmp_path))
    names = [st.name for st in G.STAGES]
    st = G.STAGES[names.index("planshapes")]
    assert names.index("planshapes") == names.index("shapes") + 1 and st.implies == "shapes" and st.suffixes == ("_plan.png", "_plan.json")
    assert G.resolve_stages(**o) == {} and list(G.resolve_stages(**o, fit_shapes=True)) == ["cloud", "ground", "clean", "cluster", "shapes"]
    G.resolve_stages(**o, plan_size="axb", plan_point_size=4, plan_stroke=-1.0, plan_label_scale=99)       # off: not looked at
    got = G.resolve_stages(**o, plan_shapes=True)
    assert list(got) == ["cloud", "ground", "clean", "cluster", "shapes", "planshapes"] and "l_split" not in got["shapes"]
    assert got["planshapes"] == {"size": (1280, 720), "point_size": 7, "stroke": 3.0, "label_scale": 2, "min_height": 1.3, "split": False}
    got = G.resolve_stages(**o, plan_shapes=True, split_l_shapes=True, cluster_height=float("nan"), plan_size="320x200", plan_point_size=3,
                           plan_stroke=1.5, plan_label_scale=0)
    assert got["shapes"]["l_split"] is True
    assert got["planshapes"] == {"size": (320, 200), "point_size": 3, "stroke": 1.5, "label_scale": 0, "min_height": None, "split": True}
    for bad in (dict(plan_size="0x10"), dict(plan_size="12"), dict(plan_point_size=4), dict(plan_point_size=17), dict(plan_stroke=0.0),
                dict(plan_stroke=float("nan")), dict(plan_label_scale=-1), dict(plan_label_scale=9)):
        with pytest.raises(ValueError):
            G.resolve_stages(**o, plan_shapes=True, **bad)
    stages = {"planshapes": {}}
    (tmp_path / "a_depth.png").write_bytes(b"")
    (tmp_path / "a_plan.png").write_bytes(b"")
    assert G.plan_frames(["/in/a.png"], str(tmp_path), 1, 0, True, stages=stages) == [0]
    (tmp_path / "a_plan.json").write_bytes(b"")
    assert G.plan_frames(["/in/a.png"], str(tmp_path), 1, 0, True, stages=stages) == []


def test_command_line_knows_the_new_options(monkeypatch, capsys):
    import generate_depth_maps as G

    monkeypatch.setattr(sys, "argv", ["generate_depth_maps.py", "--plan_shapes", "--plan_size", "0x0"])
    with pytest.raises(SystemExit):
        G.main()
    assert "--plan_size: W and H must be >= 1" in capsys.readouterr().err               # parsed, resolved, refused by its own check


# ------------------------------------------------------------------------------------------------ GPU

def _ulps(got, want):
    with np.errstate(all="ignore"):
        d = np.abs(got - want) / np.spacing(np.maximum(np.abs(got), np.abs(want)))
    return np.where(got == want, 0.0, d)


def _check(cuda, image, cam, rects=None, n_rects=None, shapes=None, n_clusters=None, stroke=3.0, alpha=230, label_scale=2, exact=None):
    """The two-step check; returns (the device's summary, the restatement's own result)."""
    import torch

    from depth_pro import overlay as OV

    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)   # noqa: E731
    H, W = image.shape[:2]
    want = ON.draw_shapes(image, cam, rects, n_rects, shapes, n_clusters, stroke, alpha, label_scale)
    src = dev(image)
    res = OV.draw_shapes(src, dev(np.asarray(cam, np.float64)), dev(rects), n_rects, dev(shapes), n_clusters, stroke, alpha, label_scale)
    got = OV.overlay_summary(res)
    assert np.array_equal(src.cpu().numpy(), image)                                      # drawn on a copy
    g, w = got["records"], want["records"]
    assert g.shape == w.shape, (g.shape, w.shape)
    ints = list(ON.INT_FIELDS)
    assert np.array_equal(g[:, ints], w[:, ints]), np.argwhere(g[:, ints] != w[:, ints])[:5]
    reals, boxes = list(ON.REAL_FIELDS), list(ON.BOX_FIELDS)
    ulps = _ulps(g[:, reals], w[:, reals])
    assert ulps.max(initial=0.0) <= 4.0, ulps.max()
    same = (g[:, reals] == w[:, reals]).all(axis=1)
    assert np.array_equal(g[same][:, boxes], w[same][:, boxes])
    assert np.abs(g[:, boxes] - w[:, boxes]).max(initial=0.0) <= 1.0
    pic, painted = ON.draw(image, g, stroke, alpha, label_scale)
    assert np.array_equal(got["image"], pic), int((got["image"] != pic).any(axis=-1).sum())
    assert got["stats"] == ON.stats_of(g, painted, degenerate=not ON.camera_ok(cam)), got["stats"]
    if exact is None:
        exact = rects is None or not np.nan_to_num(np.asarray(rects)[:, 4]).any()
    if exact:                                                                            # angles all 0: the whole chain
        assert np.array_equal(g.view(np.uint64), w.view(np.uint64))
        assert np.array_equal(got["image"], want["image"]) and got["stats"] == want["stats"]
    # in place, the same bytes
    again = OV.draw_shapes(src, dev(np.asarray(cam, np.float64)), dev(rects), n_rects, dev(shapes), n_clusters, stroke, alpha, label_scale,
                           inplace=True)
    assert again["image"].data_ptr() == src.data_ptr() and np.array_equal(src.cpu().numpy(), got["image"])
    return got, want


def _noise(W, H, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def _mixed(W, H, seed=5, n=12):
    """A camera and n rectangles (every kind of angle) with n // 2 circles spread over a W x H picture and past its edges."""
    rng = np.random.default_rng(seed)
    scale = 7.5
    cam = ON.plan_camera(0.3, -0.2, scale, W, H)
    cu = 0.3 + (rng.random(n) - 0.5) * 1.2 * W / scale
    cv = -0.2 + (rng.random(n) - 0.5) * 1.2 * H / scale
    ang = np.concatenate([[0.0, 30.0, 45.0, 90.0, 180.0, -30.0, 359.0], rng.random(n) * 90.0])[:n]
    rects = _rects(np.stack([cu, cv, rng.random(n) * 0.5 * W / scale, rng.random(n) * 0.8 * H / scale, ang], axis=1))
    m = n // 2
    circles = np.stack([0.3 + (rng.random(m) - 0.5) * W / scale, -0.2 + (rng.random(m) - 0.5) * H / scale, rng.random(m) * 0.4 * H / scale], axis=1)
    return cam, rects, _table([tuple(c) for c in circles], gaps=(1, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(67, 35), (1, 1), (64, 16), (131, 67)])
def test_picture_sizes_circles_over_rectangles_over_noise(cuda, size):
    W, H = size
    cam, rects, table = _mixed(W, H)
    got, want = _check(cuda, _noise(W, H), cam, rects, None, table, None)
    assert want["stats"]["rectangles"] + want["stats"]["circles"] > 5 and want["stats"]["pixels_painted"] > 0
    for stroke, alpha, L in ((1.0, 255, 1), (6.5, 128, 3), (3.0, 0, 8)):
        _check(cuda, _noise(W, H), cam, rects, None, table, None, stroke=stroke, alpha=alpha, label_scale=L)
    rects0 = rects.copy()
    rects0[:, 4] = 0.0
    _check(cuda, _noise(W, H), cam, rects0, None, table, None, exact=True)


@pytest.mark.gpu
def test_three_hundred_overlapping_rectangles_keep_list_order_across_chunks(cuda):
    W, H = 67, 35
    rng = np.random.default_rng(9)
    cam = ON.plan_camera(0.0, 0.0, 1.0, W, H)
    n = 300
    rows = np.stack([rng.integers(-6, 7, n), rng.integers(-4, 5, n), rng.integers(10, 60, n), rng.integers(6, 30, n), np.zeros(n)], axis=1)
    got, want = _check(cuda, _noise(W, H), cam, _rects(rows), None, None, None, label_scale=0, exact=True)
    assert want["stats"]["rectangles"] == n
    # the order matters: the same list backwards is another picture, and the device follows
    back, _ = _check(cuda, _noise(W, H), cam, _rects(rows[::-1]), None, None, None, label_scale=0, exact=True)
    assert (back["image"] != got["image"]).any()
    turned = rows.astype(np.float64)
    turned[:, 4] = rng.random(n) * 360.0 - 180.0
    _check(cuda, _noise(W, H), cam, _rects(turned), None, None, None, label_scale=1)


@pytest.mark.gpu
def test_labels_of_one_to_four_digits_on_rectangles_and_circles(cuda):
    W, H = 131, 67
    rng = np.random.default_rng(10)
    cam = ON.plan_camera(0.0, 0.0, 1.0, W, H)
    n = 1005
    rows = np.stack([rng.integers(-70, 71, n), rng.integers(-36, 37, n), rng.random(n) * 2, rng.random(n) * 2, np.zeros(n)], axis=1)
    table = _table([(float(x), float(y), 1.0) for x, y in zip(rng.integers(-60, 61, 12), rng.integers(-30, 31, 12))], gaps=(0, 5, 6))
    got, want = _check(cuda, _noise(W, H), cam, _rects(rows), None, table, None, exact=True)
    assert got["records"][:, 9].tolist() == list(range(1, n + 13)) and sorted(set(got["records"][:, 18])) == [1.0, 2.0, 3.0, 4.0]
    assert got["records"][n:, 0].tolist() == [2.0] * 12 and got["records"][n:, 18].tolist() == [4.0] * 12
    assert got["records"][n:, 8].tolist() == [float(int(c[0]) + 256 * int(c[1]) + 65536 * int(c[2])) for c in ON.palette()[8 + np.arange(12) % 8]]
    _check(cuda, _noise(W, H), cam, _rects(rows[:9]), None, table, None, label_scale=1, exact=True)    # circles 10 .. 21 after 9 rectangles


@pytest.mark.gpu
def test_numbers_above_9999_have_no_label_and_are_counted(cuda):
    W, H = 67, 35
    cam = ON.plan_camera(0.0, 0.0, 1.0, W, H)
    n = 10001
    rows = np.zeros((n, 5))
    rows[:, 0] = 1e4                                               # off-screen but for the last five
    rows[-5:, 0], rows[-5:, 1], rows[-5:, 2:4] = [-20, -10, 0, 10, 20], 3.0, 6.0
    got, want = _check(cuda, np.full((H, W, 3), 90, np.uint8), cam, _rects(rows), None, _table([(0.0, -8.0, 3.0)]), None, exact=True)
    assert want["stats"] == {**want["stats"], "rectangles": 5, "circles": 1, "offscreen": n - 5, "labels_dropped": 3, "skipped": 0}
    assert got["records"][-4:, 1].tolist() == [3.0, 5.0, 5.0, 5.0] and got["records"][-1, 9] == n + 1


@pytest.mark.gpu
def test_shapes_outside_the_picture_and_labels_alone_inside(cuda):
    W, H = 67, 35
    cam = ON.plan_camera(0.0, 0.0, 1.0, W, H)
    flat = np.full((H, W, 3), 0x5A, np.uint8)
    outside = _rects([[-100, 0, 4, 4, 0], [0, 100, 4, 4, 20], [70, 0, 40, 3, 0], [0, -40, 3, 30, 0]])
    got, want = _check(cuda, flat, cam, outside, None, _table([(200.0, 0.0, 5.0), (0.0, 0.0, 80.0)]), None, label_scale=0, exact=False)
    assert want["stats"] == {**{k: 0 for k in ON.STATS}, "offscreen": 5, "circles": 1} and (got["image"] == 0x5A).all()   # the big circle's box meets it
    # the centre 5 pixels left of the picture: the stroke's box misses it, the label's reaches pixel column 1
    got, want = _check(cuda, flat, cam, _rects([[-38, 0, 1, 1, 0], [0, 22.0, 1, 1, 0]]), None, _table([(38.0, 5.0, 0.5)]), None)
    assert got["records"][:, 1].tolist() == [2.0, 2.0, 2.0] and want["stats"]["pixels_painted"] > 0 and want["stats"]["offscreen"] == 0
    assert (got["image"][:, 2:-3][4:-4] == 0x5A).all() and (got["image"][:, :2] != 0x5A).any() and (got["image"][:, -2:] != 0x5A).any()


@pytest.mark.gpu
def test_zero_sizes_nan_and_negative_rows(cuda):
    W, H = 67, 35
    cam = ON.plan_camera(0.25, -0.5, 3.0, W, H)
    nan, inf = np.nan, np.inf
    rows = [[0, 0, 0, 0, 0], [2, 1, 0, 0, 33], [nan, 0, 2, 1, 10], [0, inf, 2, 1, 10], [0, 0, -1, 1, 10], [0, 0, 1, -2, 10], [0, 0, 1, 1, nan],
            [0, 0, 1e308, 1, 0], [3, -2, 2, 1, 10], [0, 0, 4, 0, 45], [0, 0, -0.0, 3, 0]]
    table = _table([(0, 0, 0), (0, 0, -1), (nan, 0, 1), (0, 0, inf), (1, 2, 3), (0, 0, -inf), (-3, 1, 1e-300)], gaps=(2,))
    table[2, 8:11] = nan                                           # a rectangle row of the table: its circle columns are not read
    got, want = _check(cuda, _noise(W, H), cam, _rects(rows), None, table, None, exact=False)
    assert want["stats"]["skipped"] == 10 and want["stats"]["error"] == 1 and want["stats"]["rectangles"] == 5 and want["stats"]["circles"] == 3
    one = _check(cuda, np.full((H, W, 3), 7, np.uint8), cam, _rects([[0.25, -0.5, 0, 0, 0]]), None, None, None, stroke=1.0, label_scale=0)[0]
    assert (one["image"] != 7).any(axis=-1).sum() == 1 and one["image"][17, 33].tolist() != [7, 7, 7]       # w = h = 0: the centre pixel
    dot = _check(cuda, np.full((H, W, 3), 7, np.uint8), cam, None, None, _table([(0.25, -0.5, 0.0)]), None, stroke=1.0, label_scale=0)[0]
    wide = _check(cuda, _noise(W, H), cam, _rects([[0, 0, 2, 1, 10]]), None, _table([(0, 0, 5.9e307)]), None, stroke=1e308)[0]
    assert wide["records"][:, 1].tolist() == [3.0, 8.0] and wide["stats"]["skipped"] == 1 and wide["stats"]["pixels_painted"] == W * H
    assert (dot["image"] != 7).any(axis=-1).sum() == 1                                                      # r = 0 the same


@pytest.mark.gpu
def test_counts_above_the_capacity_zero_and_null_lists(cuda):
    import torch

    W, H = 67, 35
    cam, rects, table = _mixed(W, H)
    rects[:, 4] = 0.0
    flat = np.full((H, W, 3), 0xA5, np.uint8)
    full = _check(cuda, flat, cam, rects, None, table, None)[0]
    over = _check(cuda, flat, cam, rects, 10 ** 6, table, 2 ** 31 - 1)[0]                               # clamped to the capacity
    assert np.array_equal(over["image"], full["image"]) and over["stats"] == full["stats"]
    part = _check(cuda, flat, cam, rects, torch.tensor(5, dtype=torch.int32, device=cuda), table, torch.tensor([3], dtype=torch.int32, device=cuda))[0]
    assert len(part["records"]) == 5 + 2 and part["records"][5:, 9].tolist() == [6, 7]                   # table rows 0..2 hold two circles
    for nr, nc in ((0, 0), (-4, -1)):
        none = _check(cuda, flat, cam, rects, nr, table, nc)[0]
        assert (none["image"] == 0xA5).all() and none["stats"] == {k: 0 for k in ON.STATS} and len(none["records"]) == 0
    null = _check(cuda, flat, cam)[0]
    assert (null["image"] == 0xA5).all() and null["stats"] == {k: 0 for k in ON.STATS}
    only = _check(cuda, flat, cam, None, None, table, None)[0]
    assert only["stats"]["rectangles"] == 0 and only["stats"]["circles"] > 0 and only["records"][0, 9] == 1
    _check(cuda, flat, cam, rects, None, np.zeros((0, 16)), None)
    no_labels = _check(cuda, flat, cam, rects, None, table, None, label_scale=0)[0]
    assert (no_labels["records"][:, 14:19] == [0, 0, -1, -1, 0]).all() and (no_labels["image"] != full["image"]).any()


@pytest.mark.gpu
def test_degenerate_camera_draws_nothing(cuda):
    W, H = 67, 35
    _, rects, table = _mixed(W, H)
    flat = np.full((H, W, 3), 0x33, np.uint8)
    for cam in (ON.plan_camera(0.0, 0.0, 1.0, W, H, degenerate=1.0), ON.plan_camera(np.nan, 0.0, 1.0, W, H), np.zeros(24)):
        got = _check(cuda, flat, cam, rects, None, table, None, exact=True)[0]
        assert (got["image"] == 0x33).all() and got["stats"] == {**{k: 0 for k in ON.STATS}, "error": 2} and len(got["records"]) == 0


@pytest.mark.gpu
def test_refused_arguments_leave_the_picture_untouched(cuda):
    import torch

    lib = _lib.load()
    W, H = 64, 40
    cam, rects, table = _mixed(W, H, n=10)
    image = torch.from_numpy(_noise(W, H)).to(cuda)
    before = image.cpu().numpy().copy()
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(cuda) for k, v in dict(cam=cam, rects=rects, shapes=table).items()}
    n = torch.tensor([10, 7], dtype=torch.int32, device=cuda)
    rec = torch.zeros(20, 20, dtype=torch.float64, device=cuda)
    stats = torch.full((8,), -1.0, dtype=torch.float64, device=cuda)
    ws = torch.zeros(int(lib.dp_overlay_workspace_size(10, 7)) + 8, dtype=torch.uint8, device=cuda)
    good = dict(img=image.data_ptr(), cam=t["cam"].data_ptr(), rects=t["rects"].data_ptr(), nr=n.data_ptr(), mr=10, shapes=t["shapes"].data_ptr(),
                nc=n.data_ptr() + 4, mc=7, rec=rec.data_ptr(), stats=stats.data_ptr(), ws=ws.data_ptr(), wb=ws.numel() - 8,
                stream=torch.cuda.current_stream(cuda).cuda_stream)
    pointers = ("img", "cam", "rects", "shapes", "rec", "stats", "ws", "nr", "nc")
    for bad in BAD_ARGUMENTS:
        kw = dict(good, W=W, H=H)
        for k, v in bad.items():                        # a pointer of the list: null, or this many bytes off its alignment
            kw[k] = good[k] + (v - 4096) if k in pointers and v is not None else v
        assert _call(lib, **kw) == 1000, bad
    torch.cuda.synchronize()
    assert np.array_equal(image.cpu().numpy(), before) and (stats.cpu().numpy() == -1.0).all() and not rec.cpu().numpy().any()
    assert _call(lib, W=W, H=H, **good) == 0                                                            # and the same call, unspoilt, draws
    torch.cuda.synchronize()
    assert (image.cpu().numpy() != before).any() and stats.cpu().numpy()[:2].sum() > 0


@pytest.fixture(scope="module")
def clustered_cloud():
    """About 2000 rows at y = 1.5: two boxes and a ring, 3 m apart, and a floor under them."""
    rng = np.random.default_rng(21)
    box1 = np.stack([rng.random(600) * 1.6 - 3.0, np.full(600, 1.5), rng.random(600) * 0.8 + 2.0], axis=1)
    box2 = np.stack([rng.random(600) * 0.7 + 1.0, np.full(600, 1.6), rng.random(600) * 2.0 + 3.0], axis=1)
    th = rng.random(500) * 2 * np.pi
    ring = np.stack([0.5 * np.cos(th) - 0.5, np.full(500, 1.7), 0.5 * np.sin(th) + 6.0], axis=1)
    floor = np.stack([rng.random(300) * 8 - 4, np.zeros(300), rng.random(300) * 6 + 1], axis=1)
    pts = np.vstack([box1, box2, ring, floor])
    return np.ascontiguousarray(pts[rng.permutation(len(pts))]), rng.integers(0, 256, (len(pts), 3), dtype=np.uint8)


@pytest.mark.gpu
def test_plan_with_shapes_is_render_views_then_draw_shapes(cuda, clustered_cloud):
    import torch

    from depth_pro import overlay as OV
    from depth_pro import pointcloud as PC
    from depth_pro import render as R

    pts, cols = (torch.from_numpy(a).to(cuda) for a in clustered_cloud)
    count = torch.tensor(len(pts), dtype=torch.int32, device=cuda)
    labels, ncl, _, _, order, offsets = PC.cluster_pointcloud(pts, count, max_clusters=64)
    table = PC.fit_shapes(pts, order, offsets, ncl, count, 64)[0]
    rects, n_rects = PC.rectangle_list(table, ncl, 64)
    size = (160, 96)
    whole = OV.overlay_summary(OV.plan_with_shapes(pts, cols, count, rects, n_rects, table, ncl, size=size, point_size=3, min_height=1.3))
    plan = R.render_views(pts, cols, views="plan", size=size, point_size=3, count=count, min_height=1.3)
    parts = OV.overlay_summary(OV.draw_shapes(plan["image"][0], plan["cameras"][0], rects, n_rects, table, ncl))
    assert int(ncl) == 3 and whole["stats"] == parts["stats"] and whole["stats"]["rectangles"] + whole["stats"]["circles"] == 3
    assert whole["stats"]["circles"] == 1 and whole["stats"]["offscreen"] == 0 and whole["stats"]["error"] == 0
    assert np.array_equal(whole["image"], parts["image"]) and np.array_equal(whole["records"].view(np.uint64), parts["records"].view(np.uint64))
    assert np.array_equal(whole["camera"].view(np.uint64), plan["cameras"][0].cpu().numpy().view(np.uint64))
    # and both are the restatement's: the plan of tests/render_numpy.py with the device's records drawn on it
    base = RN.render_views(clustered_cloud[0], clustered_cloud[1], ("plan",), size, 3, min_height=1.3)
    assert np.array_equal(plan["image"][0].cpu().numpy(), base["image"][0])
    pic, painted = ON.draw(base["image"][0], whole["records"])
    assert np.array_equal(whole["image"], pic) and whole["stats"]["pixels_painted"] == painted > 0
    assert whole["plan_stats"]["clipped"] == [300] and (whole["image"] != base["image"][0]).any()
