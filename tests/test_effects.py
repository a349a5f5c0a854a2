"""Depth-warped views (csrc/dp_effects.hip, depth_pro/effects.py): the parallax frames and the red-cyan anaglyph of the
reference's OLD_SCRIPTS/depth_video_effect.py.

CPU part: the restatement (tests/effects_numpy.py) against its golden file, against scipy's linear interpolation and
against its own literal (transposed, as the reference calls cv2.remap) form; the host phase schedule; every argument
error before launch; the stage lists.  GPU part: byte for byte against the restatement, `bad` exactly -- no tolerance,
every device operation is IEEE-defined."""

import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import effects_numpy as FX  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_effects.npz")
MOTIONS = ("circle", "zoom", "swing")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


# ------------------------------------------------------------------------------------------------ CPU

def test_restatement_reproduces_its_golden_file_and_scipy(golden):
    import make_golden_effects as MG

    image, depth, views = golden["image"], golden["depth"], [tuple(v) for v in golden["views"]]
    assert image.shape == (MG.H, MG.W, 3) and views == [tuple(map(float, v)) for v in MG.views()]
    out, bad = FX.warp_views(image, depth, views)
    assert np.array_equal(out, golden["out"]) and not bad.any()
    ana, ana_bad = FX.anaglyph(image, depth, MG.SEPARATION)
    assert np.array_equal(ana, golden["anaglyph"]) and ana_bad == 0
    H, W = depth.shape
    for v in views:
        mx, my = FX.maps(depth, v)
        mx, my = np.clip(mx, 0, W - 1).astype(np.float32), np.clip(my, 0, H - 1).astype(np.float32)
        assert MG.sampler_vs_scipy(image, mx, my) <= 1.0


def test_literal_transposed_form_is_the_transpose_of_ours(golden):
    image, depth = golden["image"], golden["depth"]
    for v, ours in zip(golden["views"], golden["out"]):
        literal = FX.warp_view(image, depth, tuple(v), literal=True)[0]
        assert literal.shape == (depth.shape[1], depth.shape[0], 3)
        assert np.array_equal(literal.transpose(1, 0, 2), ours)
    assert np.array_equal(golden["literal_first"].transpose(1, 0, 2), golden["out"][1])
    assert np.array_equal(golden["anaglyph_literal"].transpose(1, 0, 2), golden["anaglyph"])
    assert not np.array_equal(golden["out"][1], golden["image"])          # the view does move pixels


def test_view_params_phase_schedule():
    from depth_pro import _lib, effects as E

    W, H, a, period = 64, 48, 0.05, 100
    for motion in MOTIONS:
        for frame in (0, period // 4, period):
            got = E.view_params(motion, a, W, H, frame, period)
            assert tuple(got) == tuple(float(c) for c in FX.view_params(motion, a, W, H, frame, period)), (motion, frame)
    c0, cq, c1 = (E.view_params("circle", a, W, H, f, period) for f in (0, period // 4, period))
    assert c0 == (_lib.DP_WARP_SHIFT, a * W, 0.0)                                            # cos 0 = 1, sin 0 = 0
    assert cq.kind == _lib.DP_WARP_SHIFT and abs(cq.a) < 1e-14 and cq.b == a * H * np.sin(2 * np.pi * 25 / 100)
    assert abs(cq.b - a * H) < 1e-14 and abs(c1.a - c0.a) < 1e-14 and abs(c1.b) < 1e-14      # a quarter turn; a full one
    s0, sq = E.view_params("swing", a, W, H, 0, period), E.view_params("swing", a, W, H, period // 4, period)
    assert s0 == (_lib.DP_WARP_SHIFT, 0.0, 0.0) and abs(sq.a - a * W) < 1e-14 and sq.b == 0.0
    z0, zq = E.view_params("zoom", a, W, H, 0, period), E.view_params("zoom", a, W, H, period // 4, period)
    assert z0 == (_lib.DP_WARP_ZOOM, 0.0, 0.0) and zq.kind == _lib.DP_WARP_ZOOM and zq.a == 1 - (1.0 + a * np.sin(2 * np.pi * 25 / 100))
    with pytest.raises(ValueError, match="Unknown motion type"):
        E.view_params("spiral", a, W, H, 0, period)
    left, right = E.anaglyph_views(0.05, W)
    assert left == (_lib.DP_WARP_SHIFT_F32, 0.05 * W, 0.0) and right == (_lib.DP_WARP_SHIFT_F32, -0.05 * W, 0.0)


def test_argument_errors_are_reported_before_launch():
    """Null stream, no device: a launch would return a HIP error instead of DP_ERR_*."""
    from depth_pro import _lib

    lib = _lib.load()
    ARG, SHAPE = 1000, 1001
    P = 4096
    ws = int(lib.dp_effects_workspace_size())
    assert 0 < ws <= 4096
    one = (ctypes.c_double * 3)(_lib.DP_WARP_SHIFT, 1.0, 0.0)

    def warp(image=P, depth=P, H=8, W=8, views=one, n=1, out=P, bad=P, w=P, wb=ws):
        return lib.dp_warp_views(image, depth, H, W, views, n, out, bad, w, wb, None)

    def ana(image=P, depth=P, H=8, W=8, out=P, bad=P, w=P, wb=ws):
        return lib.dp_anaglyph(image, depth, H, W, 0.4, out, bad, w, wb, None)

    for kw in (dict(image=None), dict(depth=None), dict(out=None), dict(bad=None), dict(w=None)):
        assert warp(**kw) == ARG and ana(**kw) == ARG, kw
    assert warp(views=None) == ARG
    for kw in (dict(H=0), dict(W=0), dict(H=-3), dict(H=16385), dict(W=16385)):
        assert warp(**kw) == SHAPE and ana(**kw) == SHAPE, kw
    many = (ctypes.c_double * (3 * 33))(*([float(_lib.DP_WARP_ZOOM), 0.0, 0.0] * 33))
    assert warp(n=0) == SHAPE and warp(n=-1) == SHAPE and warp(views=many, n=33) == SHAPE
    for kind in (3.0, -1.0, 0.5, float("nan")):
        assert warp(views=(ctypes.c_double * 3)(kind, 1.0, 0.0)) == ARG, kind
    two = (ctypes.c_double * 6)(float(_lib.DP_WARP_ZOOM), 0.1, 0.0, 7.0, 0.0, 0.0)
    assert warp(views=two, n=2) == ARG                                   # the second view's kind
    assert warp(wb=ws - 1) == ARG and ana(wb=ws - 1) == ARG and warp(wb=0) == ARG
    assert _lib.DP_WARP_MAX_VIEWS == 32 and _lib.DP_ABI_VERSION == 20


def test_stage_lists_with_and_without_the_new_options(tmp_path):
    import generate_depth_maps as G

    o = dict(output_dir=str(tmp_path))
    assert [st.name for st in G.STAGES][-3:] == ["anaglyph", "parallax", "polygons"]
    assert G.resolve_stages(**o) == {}
    assert list(G.resolve_stages(**o, floor_polygons=True, floor_slices=5)) == ["cloud", "ground", "clean", "floor", "slices", "polygons"]
    assert list(G.resolve_stages(**o, pointcloud=True)) == ["cloud"]
    assert G.resolve_stages(**o, anaglyph=True) == {"anaglyph": {"separation": 0.05}}
    assert G.resolve_stages(**o, parallax="swing", parallax_period=30) == {"parallax": {"motion": "swing", "amplitude": 0.05, "period": 30}}
    both = G.resolve_stages(**o, anaglyph=True, anaglyph_separation=0.02, parallax="circle", floor_polygons=True)
    assert list(both) == ["cloud", "ground", "clean", "floor", "anaglyph", "parallax", "polygons"]
    assert both["anaglyph"] == {"separation": 0.02} and both["parallax"] == {"motion": "circle", "amplitude": 0.05, "period": 150}
    for st in G.STAGES:
        if st.name in ("anaglyph", "parallax"):
            assert st.implies is None and st.suffixes == (f"_{st.name}.png",)
    for bad in (dict(anaglyph=True, anaglyph_separation=-0.1), dict(anaglyph=True, anaglyph_separation=float("nan")),
                dict(parallax="spiral"), dict(parallax="zoom", parallax_amplitude=float("inf")),
                dict(parallax="zoom", parallax_amplitude=-1.0), dict(parallax="zoom", parallax_period=0)):
        with pytest.raises(ValueError):
            G.resolve_stages(**o, **bad)
    G.resolve_stages(**o, anaglyph_separation=-1.0, parallax_period=0)          # off: not looked at
    todo = G.plan_frames(["/in/a.png"], str(tmp_path), 1, 0, True, stages={"anaglyph": {}})
    (tmp_path / "a_depth.png").write_bytes(b"")
    assert todo == [0] and G.plan_frames(["/in/a.png"], str(tmp_path), 1, 0, True, stages={"anaglyph": {}}) == [0]
    (tmp_path / "a_anaglyph.png").write_bytes(b"")
    assert G.plan_frames(["/in/a.png"], str(tmp_path), 1, 0, True, stages={"anaglyph": {}}) == []
    assert G.plan_frames(["/in/a.png"], str(tmp_path), 1, 0, True, stages={"anaglyph": {}, "parallax": {}}) == [0]


# ------------------------------------------------------------------------------------------------ GPU

def _gpu_views(cuda, image, depth, views):
    import torch

    from depth_pro import effects as E

    out, bad = E.warp_views(torch.from_numpy(image).to(cuda), torch.from_numpy(depth).to(cuda), views)
    return out.cpu().numpy(), bad.cpu().numpy()


def _gpu_anaglyph(cuda, image, depth, separation):
    import torch

    from depth_pro import effects as E

    out, bad = E.anaglyph(torch.from_numpy(image).to(cuda), torch.from_numpy(depth).to(cuda), separation)
    return out.cpu().numpy(), int(bad)


def _same(got, want):
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), \
        f"{int((got[0] != want[0]).sum())} bytes differ"
    assert np.array_equal(np.asarray(got[1]), np.asarray(want[1])), (got[1], want[1])


@pytest.mark.gpu
def test_gpu_odd_size_three_motions_five_phases_and_anaglyph(cuda, golden):
    """37 x 53: W % 4 != 0, 3 W % 4 != 0, H W odd (bytewise views and tail next to the dword stores); the golden views."""
    image, depth, views = golden["image"], golden["depth"], [tuple(v) for v in golden["views"]]
    got = _gpu_views(cuda, image, depth, views)
    _same(got, (golden["out"], np.zeros(len(views), np.int64)))
    for k in (1, 2, 3, 5):                                   # every alignment of a view's first byte
        _same(_gpu_views(cuda, image, depth, views[:k]), (golden["out"][:k], np.zeros(k, np.int64)))
    _same(_gpu_anaglyph(cuda, image, depth, 0.05), (golden["anaglyph"], 0))
    image2, depth2 = FX.scene(38, 54, 3)                     # H W % 4 == 0 with W % 4 != 0: groups that straddle rows
    views2 = [FX.view_params(m, 0.07, 54, 38, f, 40) for m in MOTIONS for f in (3, 17, 31)]
    _same(_gpu_views(cuda, image2, depth2, views2), FX.warp_views(image2, depth2, views2))
    _same(_gpu_anaglyph(cuda, image2, depth2, 0.03), FX.anaglyph(image2, depth2, 0.03))


@pytest.mark.gpu
def test_gpu_round_half_even_coordinates(cuda):
    """16 x 64, separation 1/64 (dx = 1), depths m / 64 with 0 and 1 present: x 32 lands on an exact half for odd m."""
    rng = np.random.default_rng(5)
    H, W = 16, 64
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    depth = (rng.integers(0, 65, (H, W)) / 64.0).astype(np.float32)
    depth[0, 0], depth[0, 1] = 0.0, 1.0
    mx = FX.maps(depth, (FX.SHIFT_F32, 1.0, 0.0))[0]
    halves = np.abs((np.clip(mx, 0, W - 1).astype(np.float32) * 32) % 1 - 0.5) == 0
    assert halves.mean() > 0.3                                # the inputs do what the case is for
    _same(_gpu_anaglyph(cuda, image, depth, 1 / 64), FX.anaglyph(image, depth, 1 / 64))
    views = [(FX.SHIFT_F32, 1.0, 0.0), (FX.SHIFT_F32, -1.0, 0.0), (FX.SHIFT, 1.0, 0.25), (FX.SHIFT, -0.5, -1.0)]
    _same(_gpu_views(cuda, image, depth, views), FX.warp_views(image, depth, views))


@pytest.mark.gpu
def test_gpu_33_views_split_at_32(cuda):
    image, depth = FX.scene(128, 200, 7)
    views = [FX.view_params(MOTIONS[f % 3], 0.04, 200, 128, f, 33) for f in range(33)]
    got = _gpu_views(cuda, image, depth, views)
    assert got[0].shape == (33, 128, 200, 3)
    _same(got, FX.warp_views(image, depth, views))


@pytest.mark.gpu
def test_gpu_nan_and_inf_pixels_are_black_and_counted(cuda):
    rng = np.random.default_rng(11)
    image = rng.integers(1, 256, (2, 3, 3), dtype=np.uint8)
    depth = np.array([[1.0, np.nan, 2.0], [np.inf, 3.0, 5.0]], np.float32)
    views = [FX.view_params("circle", 0.3, 3, 2, f, 8) for f in range(8)] + [FX.view_params("swing", 0.3, 3, 2, 2, 8),
                                                                              FX.view_params("zoom", 0.3, 3, 2, 2, 8)]
    want = FX.warp_views(image, depth, views)
    assert list(want[1]) == [2] * 9 + [0]
    clean = np.where(np.isfinite(depth), depth, np.float32(3.0))        # same finite min and max
    assert np.array_equal(np.delete(want[0].reshape(10, 6, 3), [1, 3], 1), np.delete(FX.warp_views(image, clean, views)[0].reshape(10, 6, 3), [1, 3], 1))
    got = _gpu_views(cuda, image, depth, views)
    _same(got, want)
    assert not got[0][:9, 0, 1].any() and not got[0][:9, 1, 0].any() and got[0][9].all()
    for d in (depth, np.array([[1.0, -np.inf, 2.0], [np.nan, 3.0, 5.0]], np.float32)):
        ana = _gpu_anaglyph(cuda, image, d, 0.2)
        _same(ana, FX.anaglyph(image, d, 0.2))
        assert ana[1] == 2 and not ana[0][0, 1].any() and not ana[0][1, 0].any()


@pytest.mark.gpu
def test_gpu_single_pixel_and_constant_depth(cuda):
    """max == min gives 0 / 0: every pixel of a shift view is bad, none of a zoom view."""
    rng = np.random.default_rng(13)
    for H, W in ((1, 1), (5, 7)):
        image = rng.integers(1, 256, (H, W, 3), dtype=np.uint8)
        for depth in (np.full((H, W), 2.5, np.float32), np.full((H, W), np.nan, np.float32)):
            views = [FX.view_params(m, 0.1, W, H, 1, 8) for m in MOTIONS] + [(FX.SHIFT_F32, 0.4, 0.0)]
            got = _gpu_views(cuda, image, depth, views)
            _same(got, FX.warp_views(image, depth, views))
            assert list(got[1]) == [H * W, 0, H * W, H * W] and not got[0][[0, 2, 3]].any() and got[0][1].all()
            ana = _gpu_anaglyph(cuda, image, depth, 0.05)
            _same(ana, FX.anaglyph(image, depth, 0.05))
            assert ana[1] == H * W and not ana[0].any()
        zoom = [FX.view_params("zoom", 0.2, W, H, f, 8) for f in (0, 2, 6)]          # zoom alone: the depth is not read
        _same(_gpu_views(cuda, image, np.full((H, W), np.nan, np.float32), zoom), FX.warp_views(image, depth, zoom))


@pytest.mark.gpu
def test_gpu_clipping_at_all_four_borders(cuda):
    image, depth = FX.scene(37, 53, 17)
    H, W = depth.shape
    views = [FX.view_params("circle", 0.6, W, H, f, 8) for f in (0, 1, 2, 3, 4, 5, 6, 7)] + \
            [FX.view_params("zoom", 0.9, W, H, 6, 8), FX.view_params("zoom", 0.9, W, H, 2, 8)]
    mx, my = zip(*(FX.maps(depth, v) for v in views[:8]))
    assert np.max(mx) > W - 1 and np.min(mx) < 0 and np.max(my) > H - 1 and np.min(my) < 0
    zx, zy = FX.maps(depth, views[8])
    assert zx.min() < 0 and zx.max() > W - 1 and zy.min() < 0 and zy.max() > H - 1
    _same(_gpu_views(cuda, image, depth, views), FX.warp_views(image, depth, views))
    _same(_gpu_anaglyph(cuda, image, depth, 0.7), FX.anaglyph(image, depth, 0.7))


@pytest.mark.gpu
def test_gpu_parallax_views_api_and_host_image(cuda, golden):
    """parallax_views picks frames of the cycle; a host image is uploaded; results stay on the device."""
    import torch

    from depth_pro import effects as E

    image, depth = golden["image"], golden["depth"]
    d = torch.from_numpy(depth).to(cuda)
    out, bad = E.parallax_views(image, d, "swing", 0.05, 150, frames=[19, 113])
    assert out.is_cuda and bad.is_cuda and bad.dtype == torch.int64 and tuple(out.shape) == (2, 37, 53, 3)
    assert np.array_equal(out.cpu().numpy(), golden["out"][[11, 14]]) and not bad.any()
    assert tuple(E.parallax_views(image, d, "zoom", 0.05, total_frames=3)[0].shape) == (3, 37, 53, 3)
    with pytest.raises(ValueError):
        E.warp_views(image, d, [])
    with pytest.raises(ValueError):
        E.warp_views(image[:, :-1], d, [(0, 1.0, 0.0)])
