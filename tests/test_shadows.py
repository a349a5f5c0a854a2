"""Depth shadows (csrc/dp_shadows.hip, depth_pro/shadows.py): find_depth_shadows and the ground fill of the reference's
OLD_SCRIPTS/mesh_from_depth.py.

CPU part: the restatement's pure-NumPy Sobel and size filter against scipy; every argument error before launch; the
stage lists.  GPU part: byte for byte against the restatement on scipy (tests/shadows_numpy.py), every count exactly --
no tolerance, every device operation is IEEE-defined and the labelling is exact."""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import shadows_numpy as SN  # noqa: E402

SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 200), (67, 131), (130, 257))      # the last two cross 64 x 64 tiles
WIDE = (130, 257, 0)            # SN.wide_field(*WIDE): the two summation orders differ on it, on both axes


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _random_depth(h, w, seed):
    return np.random.default_rng(seed).uniform(0.5, 50.0, (h, w)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ CPU

def test_numpy_sobel_is_scipys_and_the_other_order_is_not():
    from scipy import ndimage

    fields = [_random_depth(h, w, 10 + k) for k, (h, w) in enumerate(SHAPES)] + [SN.wide_field(*WIDE)]
    for f in fields:
        for axis in (0, 1):
            want = ndimage.sobel(f, axis)
            assert want.dtype == np.float32
            assert np.array_equal(_bits(SN.sobel_numpy(f, axis)), _bits(want)), (f.shape, axis)
    wide = fields[-1]
    assert np.log2(np.abs(wide).max() / np.abs(wide).min()) > 75                    # the field does span the binades
    for axis in (0, 1):                                                             # and it is what tells the orders apart
        assert not np.array_equal(_bits(SN.sobel_left_to_right(wide, axis)), _bits(ndimage.sobel(wide, axis))), axis
    narrow = _random_depth(130, 257, 3)                                             # within 2^-10 ... 2^16 both agree
    for axis in (0, 1):
        assert np.array_equal(_bits(SN.sobel_left_to_right(narrow, axis)), _bits(ndimage.sobel(narrow, axis)))
    g = SN.gradient_magnitude(wide, SN.sobel_numpy)
    assert np.array_equal(_bits(g), _bits(SN.gradient_magnitude(wide)))


def test_numpy_size_filter_is_label_plus_bincount():
    rng = np.random.default_rng(1)
    masks = [rng.random((40, 57)) < p for p in (0.3, 0.6, 0.9)] + [SN.spiral(33, 41), SN.comb(20, 31), SN.blobs(67, 131, 2),
                                                                     np.ones((5, 6), bool), np.zeros((5, 6), bool)]
    for m in masks:
        labels, sizes = SN.region_sizes(m)
        for k in (0, 1, 2, 7, 100):
            want = ~np.isin(labels, np.where(sizes[1:] >= k)[0] + 1)                # the reference's last three lines
            assert np.array_equal(SN.small_region_mask(m, k)[0], want)
            assert np.array_equal(SN.small_region_mask_numpy(m, k), want), (np.shape(m), k)
    two = np.zeros((6, 6), bool)
    two[0:3, 0:3] = two[3:6, 3:6] = True                                            # corner contact: two components
    assert SN.small_region_mask(two, 10)[1]["components"] == 2 and SN.small_region_mask_numpy(two, 10).all()


def test_argument_errors_are_reported_before_launch():
    """Null stream, no device: a launch would return a HIP error instead of DP_ERR_ARG."""
    from depth_pro import _lib

    lib = _lib.load()
    ARG, P = 1000, 4096
    H, W = 8, 9
    ws = int(lib.dp_shadows_workspace_size(H, W))
    assert ws >= 13 * H * W and lib.dp_shadows_workspace_size(0, 4) == 0 and lib.dp_shadows_workspace_size(1 << 16, 1 << 15) == 0
    assert lib.dp_shadows_workspace_size(46340, 46340) > 13 * 46340 * 46340          # < 2^31 pixels: sized in 64 bits
    nan, inf = float("nan"), float("inf")

    def grad(depth=P, h=H, w=W, g=P, gmax=P, stats=P, wsp=P, wb=ws):
        return lib.dp_depth_gradient(depth, h, w, g, gmax, stats, wsp, wb, None)

    def edges(depth=P, h=H, w=W, thr=0.2, out=P, stats=P, wsp=P, wb=ws):
        return lib.dp_depth_edges(depth, h, w, thr, out, stats, wsp, wb, None)

    def regions(free=P, h=H, w=W, k=100, out=P, stats=P, wsp=P, wb=ws):
        return lib.dp_region_filter(free, h, w, k, out, stats, wsp, wb, None)

    def chain(depth=P, h=H, w=W, thr=0.2, k=100, out=P, dropped=None, stats=P, wsp=P, wb=ws):
        return lib.dp_depth_shadows(depth, h, w, thr, k, out, dropped, stats, wsp, wb, None)

    plane = (ctypes.c_double * 4)(0.0, -0.6, 0.8, 1.5)

    def fill(depth=P, shadow=P, h=H, w=W, pl=plane, rows=0.7, out=P, filled=P):
        return lib.dp_fill_ground_shadows(depth, shadow, h, w, pl, rows, out, filled, None)

    for fn, pointers in ((grad, ("depth", "g", "gmax", "stats", "wsp")), (edges, ("depth", "out", "stats", "wsp")),
                         (regions, ("free", "out", "stats", "wsp")), (chain, ("depth", "out", "stats", "wsp")),
                         (fill, ("depth", "shadow", "pl", "out", "filled"))):
        for name in pointers:
            assert fn(**{name: None}) == ARG, (fn.__name__, name)
        for dims in (dict(h=0), dict(w=0), dict(h=-1), dict(w=-5), dict(h=1 << 16, w=1 << 15), dict(h=46341, w=46341)):
            assert fn(**dims) == ARG, (fn.__name__, dims)
    for fn in (grad, edges, regions, chain):
        assert fn(wb=ws - 1) == ARG and fn(wb=0) == ARG and fn(wsp=P + 4) == ARG, fn.__name__
        assert fn(h=8 * H) == ARG, fn.__name__                                       # the workspace of a smaller frame
    for bad in (nan, inf, -inf):
        assert edges(thr=bad) == ARG and chain(thr=bad) == ARG, bad
    assert regions(k=-1) == ARG and chain(k=-1) == ARG
    # the fill: the unbuilt x-aligned branch, a plane or a fraction that is not finite, a misaligned count
    assert fill(pl=(ctypes.c_double * 4)(1.0, 0.0, 0.0, 1.0)) == ARG
    assert fill(pl=(ctypes.c_double * 4)(0.0, nan, 1.0, 1.0)) == ARG and fill(pl=(ctypes.c_double * 4)(0.0, -1.0, 0.0, inf)) == ARG
    assert fill(rows=nan) == ARG and fill(filled=P + 4) == ARG
    assert _lib.DP_SHADOW_STATS == len(SN.STATS) and _lib.DP_ABI_VERSION == 20


def test_stage_position_parameters_and_the_lists_of_today(tmp_path):
    import generate_depth_maps as G

    from depth_pro import shadows as SH

    assert SH.STATS == SN.STATS
    o = dict(output_dir=str(tmp_path))
    names = [st.name for st in G.STAGES]
    assert names[0] == "shadows" and names[1] == "cloud" and names[-3:] == ["anaglyph", "parallax", "polygons"]
    st = G.STAGES[0]
    assert st.implies is None and st.suffixes == ("_shadows.png", "_shadows.json")
    default = {"threshold_factor": 0.2, "min_region_size": 100, "drop": False}
    assert G.resolve_stages(**o, depth_shadows=True) == {"shadows": default}
    assert G.resolve_stages(**o, depth_shadows=True, shadow_threshold=0.35, shadow_min_region=7) == \
        {"shadows": {"threshold_factor": 0.35, "min_region_size": 7, "drop": False}}
    got = G.resolve_stages(**o, pointcloud=True, drop_depth_shadows=True)                 # implies --depth_shadows
    assert list(got) == ["shadows", "cloud"] and got["shadows"] == {**default, "drop": True}
    got = G.resolve_stages(**o, clean_pointcloud=True, drop_depth_shadows=True, anaglyph=True, floor_polygons=True)
    assert list(got) == ["shadows", "cloud", "ground", "clean", "floor", "anaglyph", "polygons"]
    for bad in (dict(drop_depth_shadows=True), dict(drop_depth_shadows=True, depth_shadows=True, anaglyph=True),
                dict(depth_shadows=True, shadow_threshold=float("nan")), dict(depth_shadows=True, shadow_threshold=float("inf")),
                dict(depth_shadows=True, shadow_min_region=-1)):
        with pytest.raises(ValueError):
            G.resolve_stages(**o, **bad)
    with pytest.raises(ValueError, match="requires --pointcloud"):
        G.resolve_stages(**o, drop_depth_shadows=True)
    G.resolve_stages(**o, shadow_threshold=float("nan"), shadow_min_region=-1)            # off: not looked at
    # with the options absent, the lists are those of today
    assert G.resolve_stages(**o) == {}
    assert list(G.resolve_stages(**o, pointcloud=True)) == ["cloud"]
    assert list(G.resolve_stages(**o, floor_polygons=True, floor_slices=5)) == ["cloud", "ground", "clean", "floor", "slices", "polygons"]
    assert list(G.resolve_stages(**o, simple_mesh=True, fit_shapes=True, anaglyph=True, parallax="zoom")) == \
        ["cloud", "ground", "clean", "cluster", "shapes", "mesh", "trimesh", "anaglyph", "parallax"]
    # --resume needs both files
    stages = {"shadows": default}
    (tmp_path / "a_depth.png").write_bytes(b"")
    assert G.plan_frames(["/in/a.png"], str(tmp_path), 1, 0, True, stages=stages) == [0]
    (tmp_path / "a_shadows.png").write_bytes(b"")
    assert G.plan_frames(["/in/a.png"], str(tmp_path), 1, 0, True, stages=stages) == [0]
    (tmp_path / "a_shadows.json").write_bytes(b"")
    assert G.plan_frames(["/in/a.png"], str(tmp_path), 1, 0, True, stages=stages) == []
    # the 8-bit grey PNG the stage writes
    from PIL import Image
    mask = (np.arange(35).reshape(5, 7) % 3 == 0).astype(np.uint8) * np.uint8(255)
    G._write_png(str(tmp_path / "m.png"), mask)
    im = Image.open(tmp_path / "m.png")
    assert im.mode == "L" and np.array_equal(np.asarray(im), mask)


# ------------------------------------------------------------------------------------------------ GPU

def _dev(cuda, a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _stats(t):
    from depth_pro import shadows as SH

    return SH.stats_dict(t.cpu().numpy())


def _check_gradient_and_edges(cuda, depth, thr=0.2):
    from depth_pro import shadows as SH

    d = _dev(cuda, depth)
    g, gmax, st = SH.gradient_magnitude(d)
    want = SN.gradient_magnitude(depth)
    assert g.dtype.is_floating_point and tuple(g.shape) == depth.shape
    diff = int((_bits(g.cpu().numpy()) != _bits(want)).sum())
    assert diff == 0, f"{diff} gradient pixels differ"
    assert _bits(gmax.cpu().numpy().reshape(1))[0] == _bits(want.max().reshape(1))[0]
    edge, st = SH.edge_mask(d, thr)
    e_want, gmax_want, nonfinite = SN.edge_mask(depth, thr)
    assert np.array_equal(edge.cpu().numpy().astype(bool), e_want)
    s = _stats(st)
    assert s["edge"] == int(e_want.sum()) and s["nonfinite"] == nonfinite == 0 and s["error"] == 0
    assert np.float32(s["gmax"]) == gmax_want
    return e_want


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_gradient_and_edges_random_depth(cuda, shape):
    edges = _check_gradient_and_edges(cuda, _random_depth(*shape, seed=20 + shape[1]))
    if shape == (130, 257):
        assert 0 < edges.sum() < edges.size                           # the threshold does cut


@pytest.mark.gpu
def test_gpu_gradient_wide_range_field_in_scipys_order(cuda):
    wide = SN.wide_field(*WIDE)
    _check_gradient_and_edges(cuda, wide, 1e-30)


@pytest.mark.gpu
def test_gpu_constant_step_and_nan_frames(cuda):
    from depth_pro import shadows as SH

    const = np.full((67, 131), 3.25, np.float32)
    assert not _check_gradient_and_edges(cuda, const).any()           # gmax == 0: no normalisation, no edge
    g, gmax, st = SH.gradient_magnitude(_dev(cuda, const))
    assert float(gmax) == 0.0 and _stats(st)["gmax"] == 0.0
    assert _check_gradient_and_edges(cuda, const, -1.0).all()         # 0 > -1: every pixel an edge, as in NumPy
    step = np.full((67, 131), 2.0, np.float32)
    step[:, 70:] = 9.0
    edges = _check_gradient_and_edges(cuda, step)
    assert edges[:, 69:71].all() and edges.sum() == 2 * 67            # the two columns at the step, nothing else
    holed = _random_depth(67, 131, 5)
    holed[30, 64] = np.nan
    res = SH.find_depth_shadows(_dev(cuda, holed), 0.2, 100, drop=True)
    out = SH.shadows_summary(res)
    assert not out["mask"].any()                                      # every pixel free, no edges: one kept component
    s = out["stats"]
    assert s["nonfinite"] == 1 and s["error"] == 1 and s["edge"] == 0 and s["shadow"] == 0
    assert s["components"] == 1 and s["kept"] == 1 and s["largest"] == 67 * 131
    assert np.array_equal(_bits(out["depth"]), _bits(holed))
    want_mask, want = SN.find_depth_shadows(holed, 0.2, 100)
    assert not want_mask.any() and {k: v for k, v in s.items() if k != "gmax"} == {k: v for k, v in want.items() if k != "gmax"}
    edge, st = SH.edge_mask(_dev(cuda, np.array([[1.0, np.inf], [2.0, 3.0]], np.float32)))
    assert not edge.cpu().numpy().any() and _stats(st)["nonfinite"] == 1
    tiny = SH.shadows_summary(SH.find_depth_shadows(_dev(cuda, holed[:3, :4].copy()), 0.2, 100))
    assert tiny["mask"].all() and tiny["stats"]["kept"] == 0          # 12 pixels < 100 (no NaN in that corner)


def _check_regions(cuda, free, k):
    from depth_pro import shadows as SH

    mask, st = SH.small_region_mask(_dev(cuda, np.asarray(free, np.uint8)), k)
    want, counts = SN.small_region_mask(free, k)
    got = mask.cpu().numpy()
    assert got.dtype == np.uint8 and got.max(initial=0) <= 1
    assert np.array_equal(got.astype(bool), want), f"{int((got.astype(bool) != want).sum())} mask pixels differ (k = {k})"
    s = _stats(st)
    assert {name: s[name] for name in counts} == counts, k
    assert s["gmax"] == 0.0 and s["nonfinite"] == 0 and s["error"] == 0 and s["shadow_nonpositive"] == 0
    return counts


def _hand_made(h, w):
    """The hand-made masks of one frame size: {name: (free, the sizes to run it with)}."""
    rng = np.random.default_rng(h * 1000 + w)
    corner = np.zeros((h, w), np.uint8)
    corner[2:34, 3:35] = 1
    corner[34:66, 35:67] = 1                                          # touches the first at one corner (and crosses tiles)
    exact = np.zeros((h, w), np.uint8)
    exact[1, 1:26] = 1                                                # 25 pixels
    exact[5:9, 60:66] = 1                                             # 24 pixels, across a tile border
    exact[62:66, 10:16] = 1                                           # 24 pixels, across the other border
    exact[40:45, 40:45] = 1                                           # 25 pixels
    checker = ((np.add.outer(np.arange(h), np.arange(w)) & 1) == 0).astype(np.uint8)
    return {"corner": (corner, (1024, 1025, 2048)), "exact": (exact, (24, 25, 26)), "zero_one": (exact | checker, (0, 1, 2)),
            "spiral": (SN.spiral(h, w), (100, h * w)), "comb": (SN.comb(h, w), (100, h * w)),
            "all_free": (np.ones((h, w), np.uint8), (100, h * w, h * w + 1)), "none_free": (np.zeros((h, w), np.uint8), (0, 100)),
            "checkerboard": (checker, (1, 2)), "random_0.6": ((rng.random((h, w)) < 0.6).astype(np.uint8), (1, 5, 30, 100))}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ((96, 96), (67, 131)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_small_region_mask_hand_made(cuda, shape):
    masks = _hand_made(*shape)
    for name, (free, sizes) in masks.items():
        for k in sizes:
            counts = _check_regions(cuda, free, k)
        if name == "corner":
            assert counts["components"] == 2 and counts["largest"] == 1024           # an 8-connected labeller finds one
        if name in ("spiral", "comb"):
            assert counts["components"] == 1 and counts["largest"] == int(free.sum())
        if name == "checkerboard":
            assert counts["largest"] == 1 and counts["components"] == int(free.sum())
    exact = masks["exact"][0]
    want25 = SN.small_region_mask(exact, 25)[0]
    assert not want25[1, 1:26].any() and want25[5:9, 60:66].all()                     # exactly k stays, k - 1 goes


@pytest.mark.gpu
def test_gpu_small_region_mask_full_frame_blobs(cuda):
    free = SN.blobs(1536, 1536, 5)
    counts = _check_regions(cuda, free, 100)
    assert counts["largest"] > free.size // 3 and counts["components"] > 10000         # one giant component, many slivers


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ((67, 131), (1536, 1536)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_gpu_find_depth_shadows_scene(cuda, shape):
    from depth_pro import shadows as SH

    depth = SN.scene(*shape, seed=7, noise=0.02 if shape[0] > 100 else 0.0)
    depth[0, 0] = 0.0                                                 # a depth <= 0 (shadow or not: counted when shadow)
    thr, k = (0.2, 100) if shape[0] < 100 else (0.05, 100)
    want, want_stats = SN.find_depth_shadows(depth, thr, k)
    assert 0 < want.sum() < want.size
    d = _dev(cuda, depth)
    plain = SH.shadows_summary(SH.find_depth_shadows(d, thr, k))
    dropped = SH.shadows_summary(SH.find_depth_shadows(d, thr, k, drop=True))
    for out in (plain, dropped):
        assert np.array_equal(out["mask"].astype(bool), want)
        assert {n: v for n, v in out["stats"].items() if n != "gmax"} == {n: v for n, v in want_stats.items() if n != "gmax"}
        assert np.float32(out["stats"]["gmax"]) == np.float32(want_stats["gmax"])
    assert "depth" not in plain
    assert np.array_equal(np.isnan(dropped["depth"]), want)                           # the NaN set is the mask
    assert np.array_equal(_bits(dropped["depth"])[~want], _bits(depth)[~want])        # the rest bit-identical
    assert np.array_equal(_bits(d.cpu().numpy()), _bits(depth))                       # the input is not touched


@pytest.mark.gpu
def test_gpu_fill_ground_shadows(cuda):
    from depth_pro import shadows as SH

    h, w = 66, 131                                                    # cy = 33: the row yi == cy is a ground row
    rng = np.random.default_rng(9)
    depth = _random_depth(h, w, 31)
    shadow = (rng.random((h, w)) < 0.4).astype(np.uint8)
    shadow[33, :] = 1
    d, s = _dev(cuda, depth), _dev(cuda, shadow)
    n = np.array([0.05, -0.8, 0.6])
    planes = [({"normal": n / np.linalg.norm(n), "d": 1.45}, 0.4),    # tilted, |n2| large
              ({"normal": [0.0, -1.0, 0.0], "d": 1.5}, 0.4),          # exactly horizontal, the rows from 26: yi == cy among them
              ({"normal": [0.0, -1.0, 0.0], "d": -1.5}, 0.7),         # negative depths below the horizon: clamped to 0.1
              ({"normal": [0.0, 0.6, -0.8], "d": 2.0}, 0.0),          # every row
              ({"normal": [1e-7, -1.0, 1e-7], "d": 1.5}, 1.0)]        # no row
    for plane, rows in planes:
        out, filled = SH.fill_ground_shadows(d, s, plane, rows)
        want = SN.fill_ground_shadows(depth, shadow, plane["normal"], plane["d"], rows)
        got = out.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), (plane, int((_bits(got) != _bits(want)).sum()))
        touched = (shadow != 0) & (np.arange(h)[:, None] >= int(rows * h))
        assert int(filled) == int(touched.sum())
        assert np.array_equal(_bits(got)[~touched], _bits(depth)[~touched])            # outside: bit-identical
        if touched.any():
            assert got[touched].min() >= np.float32(0.1)
    at_horizon = SH.fill_ground_shadows(d, s, planes[1][0], 0.4)[0][33, 5].cpu().numpy()
    assert at_horizon == np.float32(1.5 * 131 / 1e-6)                 # yi == cy: the denominator is 1e-6
    for normal in ([1.0, 0.0, 0.0], [0.5, -0.8, 1e-7]):
        with pytest.raises(ValueError, match="not built"):
            SH.fill_ground_shadows(d, s, {"normal": normal, "d": 1.0})
    with pytest.raises(ValueError):
        SH.fill_ground_shadows(d, s[:, :-1], planes[0][0])
    assert SH.fill_ground_shadows(d, s.bool(), planes[0][0], 0.4)[0].equal(SH.fill_ground_shadows(d, s, planes[0][0], 0.4)[0])
