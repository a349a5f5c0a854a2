"""Occupancy floor plan (ABI 20, csrc/dp_floorplan.hip): raster, morphology, regions, picture.

The expected values come from tests/floorplan_numpy.py, a numpy restatement of the header's rules, which the non-GPU
tests pin to scipy.ndimage through tests/golden/golden_floorplan.npz (made by tests/golden/make_golden_floorplan.py).
Grids, labels, integer columns, boxes and pixels are compared exactly; centroids within 2 ulp (sums exact, one
division); a region's mean height within cells * 2^-52 * max |height| of the restatement's fp64 sum divided by the
same count (a sum of m fp64 terms in any order is within (m - 1) * 2^-53 * sum |v| of the exact one; two such sums
differ by at most twice that, and sum |v| <= m * max |v| -- after the division by m: cells * 2^-52 * max |v|, the
rounding of the division itself included for m >= 2; a single cell's mean is exact).
"""

import ctypes
import json
import os
import sys

import numpy as np
import pytest

import floorplan_numpy as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RES, PAD, THR = 0.1, 0.2, 1.3
PLAN = dict(height_threshold=THR, resolution=RES, padding=PAD, close_size=3, close_iters=1, open_size=3, min_area=0.3,
            max_height=2.5)
MORPH_CALLS = [(cs, it, 3) for cs in (1, 3, 7, 15) for it in (1, 2)] + [(7, 1, 1), (7, 1, 7), (1, 0, 15), (15, 0, 1)]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_floorplan.npz"))


@pytest.fixture(scope="module")
def cloud(gold):
    return gold["cloud_points"], gold["cloud_colors"], int(gold["cloud_count"])


@pytest.fixture(scope="module")
def restated(cloud):
    """The restatement on the raster cloud, computed once and never changed."""
    pts, cols, count = cloud
    return {"grid": F.occupancy_grid(pts, cols, count, THR, RES, PAD), "plan": F.floor_plan(pts, cols, count, **PLAN)}


def _bits(gold, key, shape):
    return np.unpackbits(gold[key])[:shape[0] * shape[1]].reshape(shape)


def _region_inputs(grid):
    """A density and a height for a given binary grid: deterministic, some set cells empty, some heights negative."""
    h, w = grid.shape
    z, x = np.indices((h, w))
    density = ((x * 7 + z * 3) % 5).astype(np.uint32) * (grid != 0)
    height = (((x * 13 + z * 29) % 97) / 16.0 - 1.0).astype(np.float32) * (density > 0)
    return density, height


# ---- no GPU ---------------------------------------------------------------------------------------------

def test_restatement_morphology_is_pinned_to_scipy(gold):
    for name in gold["morph_names"]:
        a = gold[f"morph_{name}"]
        for k in (3, 7, 15):
            want = {op: _bits(gold, f"morph_{name}_{op}{k}", a.shape) for op in ("dilate", "erode", "close", "open")}
            assert np.array_equal(F.dilate(a, k), want["dilate"]) and np.array_equal(F.erode(a, k), want["erode"]), (name, k)
            assert np.array_equal(F.morphology(a, k, 1, 1), want["close"]), (name, k)
            assert np.array_equal(F.morphology(a, 1, 0, k), want["open"]), (name, k)
        assert np.array_equal(F.morphology(a, 1, 3, 1), a) and np.array_equal(F.morphology(a, 15, 0, 1), a)


def test_restatement_regions_are_pinned_to_scipy(gold):
    for name in gold["region_names"]:
        a = gold[f"region_{name}"]
        density, height = _region_inputs(a)
        labels, n, table, stats, _ = F.regions(a, density, height, (0.0, 0.0), RES, max_regions=4096)
        assert np.array_equal(labels, gold[f"region_{name}_labels"]) and n == labels.max(), name
        assert np.array_equal(table[:, 0], gold[f"region_{name}_sum"]), name
        assert np.array_equal(table[:, 2:6], gold[f"region_{name}_box"]), name
        com = gold[f"region_{name}_com"]
        if n:
            assert np.abs(table[:, 6] - com[:, 1]).max() <= 1e-12 * 130 and np.abs(table[:, 7] - com[:, 0]).max() <= 1e-12 * 130
        assert list(stats[:4]) == [a.sum(), n, n, 0]
    assert gold["region_checkerboard_labels"].max() == 1 and gold["region_many_labels"].max() == 2178


def test_restatement_rules_on_small_cases():
    g = np.zeros((3, 5), np.uint8)
    g[1, 2] = 1
    assert F.dilate(g, 7).all() and F.morphology(g, 7, 1, 1).all()        # the erosion's outside reads 1: the grid stays full
    assert F.erode(np.ones((3, 5), np.uint8), 7).all() and F.erode(np.ones((1, 1), np.uint8), 15).all()
    assert not F.erode(g, 3).any() and F.dilate(g, 3).sum() == 9
    two = np.zeros((4, 4), np.uint8)
    two[1, 1] = two[2, 2] = 1
    assert F.label(two)[1] == 1
    two[2, 2], two[1, 3] = 0, 1
    assert F.label(two)[1] == 2 and F.label(two)[0][1, 3] == 2
    # padding 0: the row on the maximum falls into cell W and is dropped
    pts = np.array([[0.0, 2.0, 0.0], [0.55, 2.0, 0.25], [1.0, 2.0, 0.5], [0.2, 1.0, 0.2], [np.nan, 2.0, 0.0]])
    r = F.occupancy_grid(pts, None, None, THR, 0.5, 0.0)
    assert r["dims"] == (1, 2) and list(r["stats"]) == [3, 1, 1, 1, 2, 1, 2, 0] and r["density"].tolist() == [[1, 1]]
    r = F.occupancy_grid(pts, None, None, THR, 0.5, 0.25)
    assert r["dims"] == (2, 3) and r["stats"][3] == 0 and r["origin"] == (-0.25, -0.25)
    assert F.occupancy_grid(pts, None, None, float("nan"), 0.5, 0.25)["stats"][0] == 4
    # equal heights in float32: the smaller row owns the cell
    pts = np.array([[0.1, 1.5, 0.1], [0.12, 2.0 + 1e-9, 0.1], [0.11, 2.0, 0.12], [0.9, 1.4, 0.9]])
    cols = np.array([[1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 4, 4]], np.uint8)
    r = F.occupancy_grid(pts, cols, None, THR, 0.5, 0.0)
    assert r["owner"][0, 0] == 1 and r["color"][0, 0].tolist() == [2, 2, 2] and r["height"][0, 0] == np.float32(2.0)
    assert r["density"][0, 0] == 3
    assert F.occupancy_grid(pts, None, None, 5.0, 0.5, 0.0)["stats"][7] == 1
    assert F.occupancy_grid(pts, None, None, THR, 0.5, 0.3, max_cells=8)["stats"][7] == 2
    # picture: a 5 x 5 region has a 3 x 3 interior; a too small region is blank
    lab = np.zeros((9, 12), np.int32)
    lab[1:6, 1:6], lab[7, 9] = 1, 2
    table = np.zeros((2, 13))
    table[:, 1], table[:, 12] = [0.25, 0.01], [1.25, 1.0]
    img = F.image(lab, table, RES, 0.025, 2.5)
    assert (img[2:5, 2:5] == [127, 255, 127]).all() and (img[1, 1:6] == 0).all() and (img[7, 9] == 255).all()
    assert (img == 0).all(axis=2).sum() == 16 and (F.image(lab, table, RES, 0.025, 2.5, False)[3, 3] == 180).all()


def test_workspace_size_and_argument_errors_need_no_device():
    from depth_pro import _lib

    lib = _lib.load()
    size = lib.dp_floorplan_workspace_size
    sizes = [size(n, 0) for n in (0, 1, 2048, 2049, 100003, 1 << 22)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert size(-5, -1) == sizes[0] and size(1 << 22, 0) >= 13 * (1 << 22)
    by_regions = [size(1000, k) for k in (0, 1, 100, 4096)]
    assert by_regions == sorted(by_regions) and len(set(by_regions)) == 4 and by_regions[3] >= by_regions[0] + 96 * 4096
    P, big, ARG, SHAPE = 4096, 1 << 40, 1000, 1001
    f64 = ctypes.c_double

    def grid(points=P, colors=None, n=8, thr=1.3, res=0.1, pad=0.2, mc=64, density=P, height=P, color=None, occ=P, dims=P,
             origin=P, stats=P, ws=P, wsb=big):
        return lib.dp_occupancy_grid(points, colors, None, n, f64(thr), f64(res), f64(pad), mc, density, height, color, occ,
                                     dims, origin, stats, ws, wsb, None)

    def morph(g=P, dims=P, mc=64, cs=7, it=2, os_=3, out=P, ws=P, wsb=big):
        return lib.dp_grid_morphology(g, dims, mc, cs, it, os_, out, ws, wsb, None)

    def regions(g=P, density=P, height=P, dims=P, origin=P, mc=64, res=0.1, mr=16, labels=P, n=P, table=P, stats=P, ws=P, wsb=big):
        return lib.dp_grid_regions(g, density, height, dims, origin, mc, f64(res), mr, labels, n, table, stats, ws, wsb, None)

    def image(labels=P, dims=P, mc=64, table=P, n=P, mr=16, res=0.1, area=0.025, maxh=2.5, img=P):
        return lib.dp_floorplan_image(labels, dims, mc, table, n, mr, f64(res), f64(area), f64(maxh), 1, img, None)

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert grid(res=bad) == SHAPE and regions(res=bad) == SHAPE and image(res=bad) == SHAPE and image(maxh=bad) == SHAPE, bad
    for bad in (-0.1, float("nan"), float("inf")):
        assert grid(pad=bad) == SHAPE and image(area=bad) == SHAPE, bad
    assert grid(thr=float("inf")) == SHAPE and grid(thr=float("-inf")) == SHAPE
    assert grid(n=-1) == SHAPE and grid(mc=-1) == SHAPE and morph(mc=-1) == SHAPE and regions(mc=-1) == SHAPE and image(mc=-1) == SHAPE
    assert regions(mr=-1) == SHAPE and image(mr=-1) == SHAPE
    for k in (0, 2, 4, 16, 17, -3):
        assert morph(cs=k) == SHAPE and morph(os_=k) == SHAPE, k
    assert morph(it=-1) == SHAPE
    short = size(64, 0) - 1
    for kw in ({"points": None}, {"density": None}, {"height": None}, {"occ": None}, {"dims": None}, {"origin": None},
               {"stats": None}, {"colors": P}, {"ws": None}, {"ws": P + 4}, {"wsb": 16}, {"wsb": short}):
        assert grid(**kw) == ARG, kw
    for kw in ({"g": None}, {"dims": None}, {"out": None}, {"ws": None}, {"ws": P + 4}, {"wsb": short}):
        assert morph(**kw) == ARG, kw
    for kw in ({"g": None}, {"density": None}, {"height": None}, {"dims": None}, {"origin": None}, {"labels": None}, {"n": None},
               {"table": None}, {"stats": None}, {"ws": None}, {"ws": P + 4}, {"wsb": size(64, 16) - 1}):
        assert regions(**kw) == ARG, kw
    for kw in ({"labels": None}, {"dims": None}, {"table": None}, {"n": None}, {"img": None}):
        assert image(**kw) == ARG, kw


def test_python_layer_refuses_bad_arguments_and_host_tensors(tmp_path, monkeypatch):
    import torch

    import generate_depth_maps as G
    from depth_pro import _lib
    from depth_pro import pointcloud as PC

    assert len(PC.GRID_STATS) == len(PC.REGION_STATS) == 8 and len(PC.REGION_COLUMNS) == _lib.DP_FLOOR_COLUMNS == F.COLUMNS
    assert _lib.DP_ABI_VERSION == 20 and (PC.FLOOR_MAX_DIM, PC.FLOOR_MAX_KERNEL) == (F.MAX_DIM, F.MAX_KERNEL)
    pts = torch.zeros(4, 3, dtype=torch.float64)
    g, dims = torch.zeros(12, dtype=torch.uint8), torch.tensor([3, 4], dtype=torch.int32)
    for call in (lambda: PC.occupancy_grid(pts), lambda: PC.floor_plan(pts), lambda: PC.grid_morphology(g, dims)):
        with pytest.raises(_lib.DPError):
            call()
    for call in (lambda: PC.occupancy_grid(pts, resolution=0.0), lambda: PC.occupancy_grid(pts, padding=-1.0),
                 lambda: PC.floor_plan(pts, close_size=4), lambda: PC.floor_plan(pts, open_size=17),
                 lambda: PC.floor_plan(pts, min_area=float("nan")), lambda: PC.floor_plan(pts, max_height=0.0),
                 lambda: PC.grid_morphology(g, dims, close_iters=-1), lambda: PC.occupancy_grid(pts, height_threshold=float("inf"))):
        with pytest.raises(ValueError):
            call()
    for extra in (["--floor_resolution", "0"], ["--floor_resolution", "nan"], ["--floor_min_area", "-1"], ["--floor_height", "inf"]):
        monkeypatch.setattr(G, "_model", lambda *a, **k: pytest.fail("the model was loaded"))
        monkeypatch.setattr(sys, "argv", ["generate_depth_maps.py", "--input_dir", str(tmp_path), "--floor_plan"] + extra)
        with pytest.raises(SystemExit) as e:
            G.main()
        assert e.value.code == 2, extra
    with pytest.raises(ValueError):
        G.batch_generate_depth_maps(str(tmp_path), str(tmp_path / "o"), floor_plan=True, floor_resolution=0.0)
    frames = [str(tmp_path / f"f{k}.png") for k in range(2)]
    assert G.floorplan_name(frames[0]) == "f0_floorplan.png" and G.floorplan_json_name(frames[0]) == "f0_floorplan.json"
    for k in (0, 1):
        for s in ("depth.png", "clean.ply"):
            (tmp_path / f"f{k}_{s}").write_bytes(b"")
    (tmp_path / "f0_floorplan.png").write_bytes(b"")
    (tmp_path / "f0_floorplan.json").write_bytes(b"")
    (tmp_path / "f1_floorplan.png").write_bytes(b"")             # the json is missing: not done
    assert G.plan_frames(frames, str(tmp_path), 1, 0, True, cleaned=True) == []
    assert G.plan_frames(frames, str(tmp_path), 1, 0, True, cleaned=True, floor=True) == [1]


# ---- GPU ------------------------------------------------------------------------------------------------

def _dev(a, cuda):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _grid_host(out):
    """A device `occupancy_grid` result as the restatement's dict (one read-back)."""
    h, w = (int(v) for v in out["dims"].cpu().numpy())
    cut = lambda t, *tail: t.cpu().numpy()[:h * w].reshape(h, w, *tail)      # noqa: E731
    return {"density": cut(out["density"]).view(np.uint32), "height": cut(out["height"]), "occupied": cut(out["occupied"]),
            "color": None if out["color"] is None else cut(out["color"], 3), "dims": (h, w),
            "origin": tuple(out["origin"].cpu().numpy()), "stats": out["stats"].cpu().numpy()}


def _same_grid(got, want):
    assert got["dims"] == want["dims"] and got["origin"] == tuple(want["origin"]), (got["dims"], got["origin"], want["origin"])
    assert np.array_equal(got["stats"], want["stats"]), (got["stats"], want["stats"])
    for k in ("density", "height", "occupied"):
        assert np.array_equal(got[k], want[k]), k
    if want["color"] is not None:
        occ = want["density"] > 0
        assert np.array_equal(got["color"][occ], want["color"][occ])


@pytest.mark.gpu
def test_raster(cloud, restated, cuda):
    """Fails on the parent commit: dp_occupancy_grid does not exist there."""
    from depth_pro import pointcloud as PC

    pts, cols, count = cloud
    want = restated["grid"]
    H, W = want["dims"]
    st = want["stats"]
    print(f"grid {H} x {W}; stats {st}; largest density {want['density'].max()}")
    assert W % 64 and st[1] == 12 and st[2] > 300 and st[3] == 0 and want["density"].max() > 3 and len(pts) > count
    # cells that hold equal float32 heights: the owner rule decides their colour
    live = pts[:count]
    part = live[np.isfinite(live).all(axis=1) & (live[:, 1] >= THR)]
    cell = ((part[:, 2] - want["origin"][1]) / RES).astype(int) * W + ((part[:, 0] - want["origin"][0]) / RES).astype(int)
    top = part[:, 1].astype(np.float32) == want["height"].reshape(-1)[cell]
    ties = np.count_nonzero(np.bincount(cell[top]) > 1)
    print(f"cells whose largest float32 height is shared: {ties}")
    assert ties > 20
    out = PC.occupancy_grid(_dev(pts, cuda), _dev(cols, cuda), count, THR, RES, PAD, max_cells=H * W + 77)
    _same_grid(_grid_host(out), want)
    # without colours, and with the count on the device
    import torch
    out = PC.occupancy_grid(_dev(pts, cuda), None, torch.tensor([count], dtype=torch.int32, device=cuda), THR, RES, PAD, max_cells=H * W)
    assert out["color"] is None
    _same_grid(_grid_host(out), dict(want, color=None))
    # padding 0 with an extent that is a whole number of cells (8 m x 6.25 m at 0.125 m, all binary fractions): the rows
    # on the maxima fall into column W / row H, are dropped and counted
    edge = pts.copy()
    edge[:4] = [[-4.0, 2.0, -1.0], [4.0, 2.0, 5.25], [4.0, 2.0, 0.3], [0.1, 2.0, 5.25]]
    want0 = F.occupancy_grid(edge, cols, count, THR, 0.125, 0.0)
    assert want0["dims"] == (50, 64) and want0["stats"][3] == 3
    _same_grid(_grid_host(PC.occupancy_grid(_dev(edge, cuda), _dev(cols, cuda), count, THR, 0.125, 0.0, max_cells=1 << 14)), want0)
    # NaN threshold: every finite row
    wall = F.occupancy_grid(pts, cols, count, float("nan"), RES, PAD)
    _same_grid(_grid_host(PC.occupancy_grid(_dev(pts, cuda), _dev(cols, cuda), count, None, RES, PAD, max_cells=1 << 14)), wall)
    assert wall["stats"][2] == 0 and wall["stats"][0] == count - 12


@pytest.mark.gpu
def test_raster_errors_leave_the_outputs_alone(cloud, restated, cuda):
    import torch

    from depth_pro import _lib

    pts, cols, count = cloud
    H, W = restated["grid"]["dims"]
    lib = _lib.load()
    p, c = _dev(pts, cuda), _dev(cols, cuda)

    def call(thr, mc, n_dev):
        cap = H * W
        bufs = {"density": torch.full((cap,), 7, dtype=torch.int32, device=cuda), "height": torch.full((cap,), 7.0, dtype=torch.float32, device=cuda),
                "color": torch.full((cap, 3), 7, dtype=torch.uint8, device=cuda), "occupied": torch.full((cap,), 7, dtype=torch.uint8, device=cuda)}
        dims = torch.full((2,), 9, dtype=torch.int32, device=cuda)
        origin, stats = torch.zeros(2, dtype=torch.float64, device=cuda), torch.zeros(8, dtype=torch.float64, device=cuda)
        ws = torch.empty(int(lib.dp_floorplan_workspace_size(mc, 0)), dtype=torch.uint8, device=cuda)
        rc = lib.dp_occupancy_grid(p.data_ptr(), c.data_ptr(), n_dev.data_ptr(), len(pts), thr, RES, PAD, mc, bufs["density"].data_ptr(),
                                   bufs["height"].data_ptr(), bufs["color"].data_ptr(), bufs["occupied"].data_ptr(), dims.data_ptr(),
                                   origin.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert all((t == 7).all().item() for t in bufs.values())
        return dims.cpu().tolist(), stats.cpu().numpy()

    n_dev = torch.tensor([count], dtype=torch.int32, device=cuda)
    dims, st = call(THR, H * W - 1, n_dev)                      # one cell short: error 2
    assert dims == [0, 0] and st[7] == 2 and st[0] == restated["grid"]["stats"][0] and st[4] == 0
    dims, st = call(50.0, H * W, n_dev)                         # nothing that high: error 1
    assert dims == [0, 0] and list(st) == [0, 12, count - 12, 0, 0, 0, 0, 1]
    dims, st = call(THR, H * W, torch.zeros(1, dtype=torch.int32, device=cuda))      # a live count of 0
    assert dims == [0, 0] and list(st) == [0, 0, 0, 0, 0, 0, 0, 1]


@pytest.fixture(scope="module")
def morph_cases(gold):
    """name -> (grid, {(close_size, close_iters, open_size): restated result}), computed once."""
    out = {}
    for name in gold["morph_names"]:
        a = gold[f"morph_{name}"]
        out[str(name)] = (a, {k: F.morphology(a, *k) for k in MORPH_CALLS})
    return out


@pytest.mark.gpu
def test_morphology(morph_cases, cuda):
    from depth_pro import pointcloud as PC

    shapes = set()
    for name, (a, wants) in morph_cases.items():
        h, w = a.shape
        shapes.add((h, w))
        assert a[0].any() and a[-1].any() and a[:, 0].any() and a[:, -1].any(), name       # content on all four borders
        dims = PC.grid_dims(a.shape, cuda)
        g = _dev(np.concatenate([a.reshape(-1), np.full(5, 1, np.uint8)]), cuda)          # capacity above H * W
        for key, want in wants.items():
            got = PC.grid_morphology(g, dims, *key).cpu().numpy()[:h * w].reshape(h, w)
            assert np.array_equal(got, want), (name, key, int((got != want).sum()))
        inplace = g.clone()
        assert PC.grid_morphology(inplace, dims, 7, 2, 3, out=inplace) is inplace
        assert np.array_equal(inplace.cpu().numpy()[:h * w].reshape(h, w), wants[(7, 2, 3)]) and (inplace[h * w:] == 1).all().item()
    assert shapes >= {(1, 1), (3, 5), (37, 63), (37, 64), (37, 65), (70, 130), (129, 200)}
    lone = np.zeros((3, 5), np.uint8)
    lone[1, 2] = 2                                                                         # non-zero is set; the result is 0 / 1
    got = PC.grid_morphology(_dev(lone.reshape(-1), cuda), PC.grid_dims((3, 5), cuda), 7, 1, 1).cpu().numpy()
    assert (got == 1).all()
    # dims that say "no grid": nothing is written
    keep = _dev(np.full(15, 9, np.uint8), cuda)
    for bad in ((0, 5), (4, 5), (-1, 5), (1, 9000)):
        assert (PC.grid_morphology(keep, PC.grid_dims(bad, cuda), out=keep.clone()) == 9).all().item(), bad


def _regions(grid, cuda, max_regions=4096, capacity_extra=3):
    from depth_pro import pointcloud as PC

    h, w = grid.shape
    density, height = _region_inputs(grid)
    pad = lambda a, fill: np.concatenate([a.reshape(-1), np.full(capacity_extra, fill, a.dtype)])      # noqa: E731
    origin = np.array([-1.25, 0.5])
    labels, n, table, stats = PC.grid_regions(_dev(pad(grid, 1), cuda), PC.grid_dims(grid.shape, cuda),
                                              _dev(pad(density.view(np.int32), 3), cuda), _dev(pad(height, 3.0), cuda),
                                              _dev(origin, cuda), RES, max_regions)
    want = F.regions(grid, density, height, origin, RES, max_regions)
    return labels.cpu().numpy()[:h * w].reshape(h, w), int(n.item()), table.cpu().numpy(), stats.cpu().numpy(), want


def _same_regions(got, name):
    labels, n, table, stats, (wl, wn, wt, ws, bound) = got
    rows = len(wt)
    print(f"{name}: regions {n} (want {wn}), stats {stats}")
    assert n == wn and np.array_equal(labels, wl) and np.array_equal(stats, ws)
    t = table[:rows]
    for c in (0, 1, 2, 3, 4, 5, 10, 11):
        assert np.array_equal(t[:, c], wt[:, c]), (name, c)
    for c in (6, 7, 8, 9):
        assert (np.abs(t[:, c] - wt[:, c]) <= 2 * np.spacing(np.abs(wt[:, c]))).all(), (name, c)
    err = np.abs(t[:, 12] - wt[:, 12])
    if rows:
        print(f"  largest mean-height error {err.max():.3e}, bound there {bound[err.argmax()]:.3e}")
    assert (err <= bound).all(), name
    assert (table[rows:] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["spiral", "combs", "diagonals", "checkerboard", "empty", "full", "blobs"])
def test_regions(name, gold, cuda):
    grid = gold[f"region_{name}"]
    got = _regions(grid, cuda)
    _same_regions(got, name)
    assert np.array_equal(got[0], gold[f"region_{name}_labels"])
    expect = {"spiral": 1, "combs": 2, "checkerboard": 1, "empty": 0, "full": 1}
    if name in expect:
        assert got[1] == expect[name]


@pytest.mark.gpu
def test_regions_overflow(gold, cuda):
    grid = gold["region_many"]
    got = _regions(grid, cuda, max_regions=100)
    _same_regions(got, "many")
    labels, n, table, stats, _ = got
    assert n == 2178 and list(stats[:4]) == [2178, 2178, 100, 1] and labels.max() == 2178
    assert (table[:100, 0] == 1).all() and list(table[99, 2:6]) == [2 * (99 % 66), 2 * (99 // 66)] * 2
    got = _regions(grid, cuda, max_regions=0)
    assert got[1] == 2178 and got[3][2] == 0 and got[3][3] == 1 and np.array_equal(got[0], gold["region_many_labels"])


@pytest.mark.gpu
def test_floor_plan_picture(cloud, restated, cuda):
    from depth_pro import pointcloud as PC

    pts, cols, count = cloud
    want = restated["plan"]
    H, W = want["grid"]["dims"]
    areas = want["table"][:, 1]
    img = want["image"]
    black, white = (img == 0).all(axis=2), (img == 255).all(axis=2)
    print(f"regions {want['n_regions']}, areas {np.sort(areas)}; black {black.sum()}, filled {(~black & ~white).sum()}")
    assert (areas >= PLAN["min_area"]).sum() >= 3 and (areas < PLAN["min_area"]).sum() >= 1
    dropped = np.isin(want["labels"], 1 + np.flatnonzero(areas < PLAN["min_area"]))
    bar = np.zeros((H, W), bool)
    bar[H - 50:H - 30, W - 60:W - 50] = True
    assert dropped.any() and white[dropped & ~bar].all() and black[bar].all() and (~black & ~white).sum() > 100
    plan = PC.floor_plan(_dev(pts, cuda), _dev(cols, cuda), count, max_cells=1 << 13, max_regions=64, **PLAN)
    _same_grid(_grid_host(plan), want["grid"])
    s = PC.floor_plan_summary(plan)
    cleaned = plan["cleaned"].cpu().numpy()[:H * W].reshape(H, W)
    labels = plan["labels"].cpu().numpy()[:H * W].reshape(H, W)
    assert np.array_equal(cleaned, want["cleaned"]) and np.array_equal(labels, want["labels"])
    assert s["image"].shape == (H, W, 3) and np.array_equal(s["image"], img), int((s["image"] != img).any(axis=2).sum())
    assert (s["height"], s["width"]) == (H, W) and s["origin"] == list(want["grid"]["origin"]) and s["stats"]["error"] == 0
    assert [r["label"] for r in s["regions"]] == [int(k) + 1 for k in np.flatnonzero(areas >= PLAN["min_area"])]
    assert [r["cells"] for r in s["regions"]] == [int(c) for c in want["table"][areas >= PLAN["min_area"], 0]]
    json.dumps({k: v for k, v in s.items() if k != "image"})
    # grey fill
    grey = PC.floorplan_image(plan["labels"], plan["dims"], plan["table"], plan["n_regions"], RES, PLAN["min_area"], 2.5, False)
    assert np.array_equal(grey.cpu().numpy()[:H * W].reshape(H, W, 3), F.image(want["labels"], want["table"], RES, PLAN["min_area"], 2.5, False))
    # the reference's own values run through as well (closing 7 x 7 twice)
    ref = F.floor_plan(pts, cols, count)
    got = PC.floor_plan_summary(PC.floor_plan(_dev(pts, cuda), _dev(cols, cuda), count, max_cells=1 << 13))
    assert np.array_equal(got["image"], ref["image"]) and got["region_stats"]["regions"] == ref["n_regions"]


@pytest.mark.gpu
def test_generate_depth_maps_floor_plan(tmp_path, cuda):
    """--floor_plan on the example frame: both files, the PNG decodes to the device image, the JSON round-trips the table."""
    import torch
    from PIL import Image

    import generate_depth_maps as G
    from depth_pro import pointcloud as PC

    gg = np.load(os.path.join(GOLDEN, "golden_ground.npz"))
    src, out = tmp_path / "frames", tmp_path / "out"
    src.mkdir()
    Image.open(os.path.join(GOLDEN, "data", "example.jpg")).convert("RGB").resize((128, 96)).save(src / "output_0000.png")

    class Model:
        def infer(self, x, f_px=None):
            return {"depth": _dev(gg["flat_depth"], cuda).clone(), "focallength_px": torch.tensor(float(gg["flat_f"]), device=cuda)}

    kw = dict(pattern="output_*.png", model=(Model(), lambda im: torch.as_tensor(np.asarray(im))), stray_radius=0.25,
              stray_neighbors=12, floor_plan=True, floor_resolution=0.05, floor_height=float("nan"), floor_min_area=0.01)
    assert G.batch_generate_depth_maps(str(src), str(out), **kw) == 1
    assert sorted(os.listdir(out)) == ["ground.json", "output_0000_clean.ply", "output_0000_depth.png", "output_0000_floorplan.json",
                                       "output_0000_floorplan.png"]
    # the device picture and table of the written cloud, made here by the public call
    cp, cc = PC.read_ply(str(out / "output_0000_clean.ply"))
    s = PC.floor_plan_summary(PC.floor_plan(_dev(cp, cuda), _dev(cc, cuda), None, height_threshold=None, resolution=0.05,
                                            min_area=0.01))
    png = np.asarray(Image.open(out / "output_0000_floorplan.png"))
    js = json.load(open(out / "output_0000_floorplan.json"))
    assert png.shape == (js["height"], js["width"], 3) and np.array_equal(png, s["image"]) and js["height"] * js["width"] > 0
    back = json.loads(json.dumps({k: v for k, v in s.items() if k != "image"}))
    means = [(r.pop("mean_height"), w.pop("mean_height")) for r, w in zip(js["regions"], back["regions"])]
    assert js == back and all(abs(a - b) <= 1e-12 * max(1.0, abs(b)) for a, b in means)      # the mean's sum has no fixed order
    assert js["resolution"] == 0.05 and js["parameters"]["height_threshold"] is None and js["parameters"]["min_area"] == 0.01
    assert js["stats"]["error"] == 0 and js["stats"]["participants"] > 100 and len(js["regions"]) >= 1
    assert all(r["area"] >= 0.01 and r["cells"] == round(r["area"] / 0.05 ** 2) for r in js["regions"])
    # the written cloud rasterises to the same grid in the restatement
    want = F.occupancy_grid(cp, cc, None, float("nan"), 0.05, 0.2)
    assert (js["height"], js["width"]) == want["dims"] and js["origin"] == list(want["origin"])
    assert js["stats"]["occupied_cells"] == want["stats"][4]
    assert G.plan_frames([str(src / "output_0000.png")], str(out), 1, 0, True, cleaned=True, floor=True) == []
