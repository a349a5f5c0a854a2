"""Floor-plan polygons (additive to ABI 20, csrc/dp_outline.hip): outlines, simplification, the polygons file.

The expected values come from tests/outline_numpy.py, a sequential restatement of rules O1-O5 and S1-S7 of the header.
The non-GPU tests pin it: hand cases whose OpenCV result is documented behaviour, the set of emitted cells against
scipy.ndimage (region & dilation of the outside of the filled region), the hull against scipy.spatial.ConvexHull, and
tests/golden/golden_outline.npz (made by tests/golden/make_golden_outline.py) against drift.  On the device vertices,
counts, the shoelace sum and the perimeter are compared exactly (the perimeter's fp64 sum of float32 lengths is exact
at these sizes, so its order cannot show); unsnapped polygons exactly (integers); a snapped rectangle's corners within
REL * hypot(width, height) of the restatement's, tests/test_shapes.py's margin rule for rectangle geometry (measured on
the fixtures: 0, every corner bit-identical); the mean height within MEAN_REL of numpy's fp64 mean.
"""

import ctypes
import json
import os
import sys

import numpy as np
import pytest
from scipy import ndimage
from scipy.spatial import ConvexHull

import outline_numpy as ON
import shapes_numpy as SN

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RES = 0.1
ORIGIN = (-1.2342, 0.4318)
REL = 1e-12                 # tests/test_shapes.py's relative margin for rectangle geometry
MEAN_REL = 1.4e-15          # one decade over the worst relative error seen on the device (1.36e-16): DESIGN.md section 18
CROSS = ndimage.generate_binary_structure(2, 1)
ONES3 = np.ones((3, 3), bool)
FIXTURES = ["shapes", "plus", "dots", "blob", "h1", "w1", "empty", "full"]
FLOOR_REGIONS = ["spiral", "combs", "diagonals", "checkerboard", "blobs", "empty", "full"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_outline.npz"))


@pytest.fixture(scope="module")
def floor_gold():
    return np.load(os.path.join(GOLDEN, "golden_floorplan.npz"))


@pytest.fixture(scope="module")
def restated(gold, floor_gold):
    """The restatement on every grid the device tests use, computed once and never changed."""
    out = {}
    for name in FIXTURES:
        out[name] = (gold[f"{name}_labels"], ON.region_outlines(gold[f"{name}_labels"]))
    for name in FLOOR_REGIONS:
        lab = floor_gold[f"region_{name}_labels"]
        out["floor_" + name] = (lab, ON.region_outlines(lab))
    return out


def _border_cells(region):
    """region & dilation of the outside of the filled region, 4-neighbour cross, the grid padded by one outside cell."""
    p = np.pad(region, 1)
    outside = ~ndimage.binary_fill_holes(p, structure=CROSS)
    return (p & ndimage.binary_dilation(outside, structure=CROSS))[1:-1, 1:-1]


def _check_trace(lab, label):
    emitted, verts = ON.trace(lab, label)
    got = np.zeros(lab.shape, bool)
    for x, z in emitted:
        got[z, x] = True
    assert np.array_equal(got, _border_cells(lab == label)), label
    n = len(emitted)
    assert all(max(abs(emitted[i][0] - emitted[(i + 1) % n][0]), abs(emitted[i][1] - emitted[(i + 1) % n][1])) == 1
               for i in range(n)) or n == 1
    first = int(np.flatnonzero(lab.reshape(-1) == label)[0])
    assert verts[0] == (first % lab.shape[1], first // lab.shape[1]) and set(verts) <= set(emitted)


# ---- no GPU ---------------------------------------------------------------------------------------------

def test_restatement_hand_cases_with_documented_opencv_results():
    lab = np.zeros((8, 10), np.int32)
    lab[2:6, 3:9] = 1
    assert ON.trace(lab, 1)[1] == [(3, 2), (3, 5), (8, 5), (8, 2)]          # top-left, bottom-left, bottom-right, top-right
    o = ON.region_outlines(lab)
    assert o["columns"][0].tolist() == [4, 16, -30, 2 * 10 + 3] and o["measures"][0].tolist() == [15.0, 16.0]
    lab[:] = 0
    lab[4, 7] = 1
    assert ON.trace(lab, 1) == ([(7, 4)], [(7, 4)])
    lab[4, 2:8] = 1
    assert ON.trace(lab, 1)[1] == [(2, 4), (7, 4)] and len(ON.trace(lab, 1)[0]) == 10
    assert ON.region_outlines(lab)["measures"][0].tolist() == [0.0, 10.0]
    assert ON.trace(lab.T.copy(), 1)[1] == [(4, 2), (4, 7)]
    # a hole is never entered; a diagonal neighbour belongs to the region
    lab[:] = 0
    lab[1:7, 1:7] = 1
    lab[3:5, 3:5] = 0
    assert ON.trace(lab, 1)[1] == [(1, 1), (1, 6), (6, 6), (6, 1)]
    lab[7, 7] = 1
    assert (7, 7) in ON.trace(lab, 1)[1]


def test_restatement_border_cells_are_pinned_to_scipy(gold, floor_gold):
    for name in FIXTURES:
        lab = gold[f"{name}_labels"]
        for l in range(1, int(lab.max()) + 1):
            _check_trace(lab, l)
    for name in FLOOR_REGIONS:
        lab = floor_gold[f"region_{name}_labels"]
        for l in range(1, min(int(lab.max()), 40) + 1):
            _check_trace(lab, l)
    g = np.random.default_rng(5)
    regions = 0
    for _ in range(12):
        lab = ndimage.label(g.random((24, 31)) < g.uniform(0.3, 0.6), structure=ONES3)[0].astype(np.int32)
        for l in range(1, int(lab.max()) + 1):
            _check_trace(lab, l)
        regions += int(lab.max())
    assert regions > 200


def test_restatement_reproduces_the_golden_file(gold, restated):
    assert list(gold["names"]) == FIXTURES and float(gold["resolution"]) == RES
    for name in FIXTURES:
        lab, o = restated[name]
        assert np.array_equal(ndimage.label(gold[f"{name}_grid"], structure=ONES3)[0], lab)
        for k in ("offsets", "vertices", "columns", "stats"):
            assert np.array_equal(o[k], gold[f"{name}_{k}"]), (name, k)
        assert np.array_equal(o["measures"], gold[f"{name}_measures"]), name
        for i, ma in enumerate(gold["min_areas"]):
            p = ON.simplify_outlines(o, RES, float(ma))
            for k in ("offsets", "polygons", "stats"):
                assert np.array_equal(p[k], gold[f"{name}_poly{i}_{k}"]), (name, i, k)
            assert np.abs(p["vertices"] - gold[f"{name}_poly{i}_vertices"]).max(initial=0.0) <= 1e-12, (name, i)
    pol = gold["shapes_poly1_polygons"]
    # one ring each of 3, 4, 6 and 7 vertices (S4 / S6 boundaries), every drop reason but overflow
    ring = {int(n): (int(v), int(f)) for n, v, f, r in zip(pol[:, 7], pol[:, 1], pol[:, 2], pol[:, 6]) if r == 0}
    assert ring[3] == (3, 0) and ring[4] == (4, 1) and ring[6] == (4, 1) and ring[7] == (7, 0) and ring[24] == (24, 0)
    assert set(pol[:, 6].astype(int)) == {0, 2, 3} and 1 in set(gold["shapes_poly0_polygons"][:, 6].astype(int))
    assert gold["dots_stats"][0] == 77 and (gold["blob_columns"][:, 1] % 64 != 0).any()


def test_restatement_hull_validity_and_douglas_peucker(restated):
    g = np.random.default_rng(9)
    for _ in range(50):
        p = g.integers(0, 12, (int(g.integers(4, 7)), 2)).astype(np.float64)
        if len(np.unique(p, axis=0)) < 3 or abs(SN.hull_area(p[SN.hull(p)])) == 0:
            continue
        assert set(SN.hull(p).tolist()) == set(ConvexHull(p).vertices.tolist()) or len(np.unique(p, axis=0)) < len(p)
    assert not ON.ring_valid([(0, 0), (4, 4), (4, 0), (0, 4)])                           # a bow-tie
    assert not ON.ring_valid([(0, 0), (4, 0), (4, 4), (2, 0), (0, 4)])                   # touches itself at a vertex
    assert not ON.ring_valid([(0, 0), (4, 0), (8, 0), (4, 0), (4, 4)])                   # a repeated vertex
    assert not ON.ring_valid([(0, 0), (6, 0), (3, 0), (3, 4)])                           # a spike
    assert not ON.ring_valid([(0, 0), (2, 0), (5, 0)])                                   # no area
    assert ON.ring_valid([(0, 0), (0, 4), (4, 4), (4, 2), (2, 2), (2, 0)])               # an L
    assert ON.ring_valid([(0, 0), (2, 0), (4, 0), (4, 4)])                               # a redundant vertex is valid
    # S3's guarantee in fp64: never more vertices, and every outline vertex within epsilon of the simplified ring, taken
    # as the rule takes it -- the distance to the LINE through the chord of the vertex's chain (|cross| / |chord|), for
    # a chord with distinct ends.  The distance to the chord as a segment is not bounded by the rule (OpenCV's is the
    # same): floor_blobs region 271 at epsilon 1.5 has a vertex 2.0 from the nearest segment of its ring.
    for name in ("blob", "floor_blobs", "floor_spiral", "shapes"):
        lab, o = restated[name]
        for r in range(len(o["columns"])):
            v = o["vertices"][o["offsets"][r]:o["offsets"][r + 1]].astype(np.float64)
            n = len(v)
            for eps in (0.005 * o["measures"][r, 1], 1.5):
                idx = ON.douglas_peucker(v, eps)
                assert len(idx) <= n and len(set(idx)) == len(idx)
                if len(idx) < 2:
                    continue
                for k, a in enumerate(idx):
                    b = idx[(k + 1) % len(idx)]
                    chord = v[b] - v[a]
                    if not chord.any():
                        continue
                    for j in range(1, (b - a) % n):
                        p = v[(a + j) % n] - v[a]
                        d = abs(p[1] * chord[0] - p[0] * chord[1]) / np.hypot(*chord)
                        assert d <= eps * (1 + 1e-12), (name, r, eps, d)


def test_workspace_size_and_argument_errors_need_no_device():
    from depth_pro import _lib

    lib = _lib.load()
    size = lib.dp_outline_workspace_size
    assert size(0, 0, 0) > 0 and size(-1, -1, -1) == size(0, 0, 0) and size(1 << 22, 0, 0) == size(0, 0, 0)
    assert size(0, 4096, 1 << 20) >= 20 * (1 << 20) + 80 * 4096 and size(0, 16, 100) < size(0, 17, 100) < size(0, 17, 1000)
    P, big, ARG, SHAPE = 4096, 1 << 40, 1000, 1001
    f64 = ctypes.c_double

    def outl(labels=P, dims=P, mc=64, n=P, mr=16, mv=64, off=P, verts=P, cols=P, meas=P, stats=P, ws=P, wsb=big):
        return lib.dp_region_outlines(labels, dims, mc, n, mr, mv, off, verts, cols, meas, stats, ws, wsb, None)

    def simp(off=P, verts=P, cols=P, meas=P, n=P, mr=16, mv=64, res=0.1, area=0.025, mp=64, poff=P, pv=P, pol=P, stats=P, ws=P,
             wsb=big):
        return lib.dp_simplify_outlines(off, verts, cols, meas, n, mr, mv, f64(res), f64(area), mp, poff, pv, pol, stats, ws, wsb,
                                        None)

    def mean(points=P, n=8, thr=1.3, out=P):
        return lib.dp_floor_mean_height(points, None, n, f64(thr), out, None)

    for kw in ({"mc": -1}, {"mr": -1}, {"mv": -1}):
        assert outl(**kw) == SHAPE, kw
    for kw in ({"labels": None}, {"dims": None}, {"n": None}, {"off": None}, {"verts": None}, {"cols": None}, {"meas": None},
               {"stats": None}, {"ws": None}, {"ws": P + 4}, {"wsb": size(64, 16, 64) - 1}):
        assert outl(**kw) == ARG, kw
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert simp(res=bad) == SHAPE, bad
    for bad in (-0.1, float("nan"), float("inf")):
        assert simp(area=bad) == SHAPE, bad
    for kw in ({"mr": -1}, {"mv": -1}, {"mp": -1}):
        assert simp(**kw) == SHAPE, kw
    for kw in ({"off": None}, {"verts": None}, {"cols": None}, {"meas": None}, {"n": None}, {"poff": None}, {"pv": None},
               {"pol": None}, {"stats": None}, {"ws": None}, {"ws": P + 4}, {"wsb": size(0, 16, 64) - 1}):
        assert simp(**kw) == ARG, kw
    assert mean(points=None) == ARG and mean(out=None) == ARG and mean(n=-1) == SHAPE and mean(thr=float("inf")) == SHAPE


def test_python_layer_refuses_bad_arguments_and_host_tensors(tmp_path):
    import torch

    import generate_depth_maps as G
    from depth_pro import _lib
    from depth_pro import pointcloud as PC

    assert len(PC.OUTLINE_COLUMNS) == _lib.DP_OUTLINE_INT_COLUMNS == ON.INT_COLUMNS and _lib.DP_ABI_VERSION == 20
    assert len(PC.OUTLINE_MEASURES) == _lib.DP_OUTLINE_REAL_COLUMNS and len(PC.POLYGON_COLUMNS) == _lib.DP_POLYGON_COLUMNS
    assert len(PC.OUTLINE_STATS) == len(PC.POLYGON_STATS) == 8 and len(PC.DROP_REASONS) == 5
    plan = {"labels": torch.zeros(12, dtype=torch.int32), "dims": torch.tensor([3, 4], dtype=torch.int32),
            "n_regions": torch.zeros(1, dtype=torch.int32), "table": torch.zeros(4, 13, dtype=torch.float64),
            "parameters": {"resolution": 0.1, "min_area": 0.025, "height_threshold": 1.3}}
    for call in (lambda: PC.region_outlines(plan), lambda: PC.floor_polygons(plan),
                 lambda: PC.floor_mean_height(torch.zeros(4, 3, dtype=torch.float64))):
        with pytest.raises(_lib.DPError):
            call()
    for call in (lambda: PC.region_outlines(plan, max_vertices=-1), lambda: PC.region_outlines({"labels": plan["labels"]}),
                 lambda: PC.simplify_outlines(plan), lambda: PC.floor_polygons(plan, max_polygon_vertices=1 << 31),
                 lambda: PC.floor_mean_height(torch.zeros(4, 3, dtype=torch.float64), height_threshold=float("inf")),
                 lambda: PC.floor_polygons_summary(plan)):
        with pytest.raises(ValueError):
            call()
    assert [s.name for s in G.STAGES][-1] == "polygons" and G.STAGES[-1].implies == "floor"
    assert list(G.resolve_stages(floor_polygons=True)) == ["cloud", "ground", "clean", "floor", "polygons"]
    assert "polygons" not in G.resolve_stages(floor_plan=True)
    frames = [str(tmp_path / f"f{k}.png") for k in range(2)]
    for k in (0, 1):
        for s in ("depth.png", "clean.ply", "floorplan.png", "floorplan.json", "floorplan.txt"):
            (tmp_path / f"f{k}_{s}").write_bytes(b"")
    (tmp_path / "f0_floorplan_polygons.json").write_bytes(b"")
    assert G.plan_frames(frames, str(tmp_path), 1, 0, True, stages=("clean", "floor")) == []
    assert G.plan_frames(frames, str(tmp_path), 1, 0, True, stages=("clean", "floor", "polygons")) == [1]
    # the text file: the reference's header and line format, descending label
    s = {"height": 1.23456, "polygons": [{"label": 1, "vertices_reference": [[0.0, 1.0], [2.0, 1.0005], [2.0, 3.0]]},
                                         {"label": 3, "vertices_reference": [[-1.0, 0.25], [0.5, 0.5], [0.0, 7.0], [1.0, 1.0]]}]}
    text = open(PC.export_floorplan_text(str(tmp_path / "p.txt"), s)).read()
    assert text == ("# Floor Plan Data\n# Units: meters\n\n# Shapes by height\n# Format: height, num_points, x1, z1, x2, z2, ...\n"
                    "1.235, 4, -1.000, 0.250, 0.500, 0.500, 0.000, 7.000, 1.000, 1.000\n"
                    "1.235, 3, 0.000, 1.000, 2.000, 1.000, 2.000, 3.000\n")
    xy = np.array([[2.0, 3.0], [2.0, 9.0], [12.0, 9.0]])
    assert np.allclose(PC.reference_world(xy, ORIGIN, RES), ON.world_reference(xy, ORIGIN, RES), rtol=0, atol=0)


# ---- GPU ------------------------------------------------------------------------------------------------

def _dev(a, cuda):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _plan(lab, cuda, max_regions=512, n_regions=None, min_area=0.025):
    """A floor_plan result as far as the polygon stages read it, from a label grid made on the host."""
    import torch

    from depth_pro import pointcloud as PC

    n = int(lab.max()) if n_regions is None and lab.size else int(n_regions or 0)
    return {"labels": _dev(lab.astype(np.int32).reshape(-1), cuda), "dims": PC.grid_dims(lab.shape, cuda),
            "n_regions": torch.tensor([n], dtype=torch.int32, device=cuda),
            "table": torch.zeros(max_regions, 13, dtype=torch.float64, device=cuda), "origin": _dev(np.array(ORIGIN), cuda),
            "parameters": {"resolution": RES, "min_area": min_area, "height_threshold": 1.3}}


def _outline_host(plan):
    st = plan["outline_stats"].cpu().numpy()
    rows = int(st[1])
    off = plan["outline_offsets"].cpu().numpy()[:rows + 1]
    return {"offsets": off, "vertices": plan["outline_vertices"].cpu().numpy()[:off[rows]],
            "columns": plan["outline_columns"].cpu().numpy()[:rows], "measures": plan["outline_measures"].cpu().numpy()[:rows],
            "stats": st}


def _same_outlines(got, want):
    assert np.array_equal(got["stats"], want["stats"]), (got["stats"], want["stats"])
    for k in ("offsets", "columns", "vertices"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["measures"], want["measures"])            # area exact; perimeter to the last bit


def _same_polygons(plan, want, record=None):
    """Polygon rows, offsets and vertices against the restatement's: exact but for a snapped rectangle's corners and area."""
    st = plan["polygon_stats"].cpu().numpy()
    rows = int(st[0])
    pol = plan["polygons"].cpu().numpy()[:rows]
    off = plan["polygon_offsets"].cpu().numpy()[:rows + 1]
    verts = plan["polygon_vertices"].cpu().numpy()[:off[rows]]
    assert np.array_equal(st, want["stats"]), (st, want["stats"])
    assert np.array_equal(off, want["offsets"]) and np.array_equal(pol[:, [0, 1, 2, 6, 7]], want["polygons"][:, [0, 1, 2, 6, 7]])
    assert np.array_equal(pol[:, 5], want["polygons"][:, 5])                                  # epsilon: one fp64 product
    worst = 0.0
    for r in range(rows):
        g, w = verts[off[r]:off[r + 1]], want["vertices"][off[r]:off[r + 1]]
        if pol[r, 2] == 0:
            assert np.array_equal(g, w) and np.array_equal(pol[r, 3:5], want["polygons"][r, 3:5]), r
        elif len(g):
            diag = float(np.hypot(*(w.max(axis=0) - w.min(axis=0))))
            d = float(np.linalg.norm(g - w, axis=1).max()) / diag
            worst = max(worst, d)
            assert d <= REL, (r, d)
            assert abs(pol[r, 3] - want["polygons"][r, 3]) <= REL * want["polygons"][r, 3], r
    print(f"snapped corners: worst distance / diagonal = {worst:.3e}")
    if record is not None:
        record("snapped_corner_rel", worst)
    return pol, off, verts


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES + ["floor_" + n for n in FLOOR_REGIONS])
def test_outlines_and_polygons_on_fixture(name, restated, cuda, record):
    from depth_pro import pointcloud as PC

    lab, want = restated[name]
    plan = PC.region_outlines(_plan(lab, cuda), max_vertices=1 << 14)
    _same_outlines(_outline_host(plan), want)
    for ma in (0.025, 0.0):
        plan["parameters"]["min_area"] = ma
        _same_polygons(PC.simplify_outlines(plan, max_polygon_vertices=1 << 13), ON.simplify_outlines(want, RES, ma), record)


@pytest.mark.gpu
def test_many_regions_table_rows_and_region_overflow(floor_gold, cuda):
    """2178 single cells with 100 table rows: rows past max_regions are skipped and flagged."""
    from depth_pro import pointcloud as PC

    lab = floor_gold["region_many_labels"]
    plan = PC.floor_polygons(_plan(lab, cuda, max_regions=100, min_area=0.0), max_vertices=256, max_polygon_vertices=16)
    want = ON.region_outlines(lab, max_regions=100, max_vertices=256)
    _same_outlines(_outline_host(plan), want)
    assert want["stats"].tolist() == [2178, 100, 100, 100, 0, 1, 66, 131]
    _same_polygons(plan, ON.simplify_outlines(want, RES, 0.0, 16))


@pytest.mark.gpu
def test_overflow_leaves_other_regions_intact_and_nothing_past_capacity(restated, cuda):
    import torch

    from depth_pro import _lib

    lib = _lib.load()
    lab, full = restated["shapes"]
    rows, H, W = len(full["columns"]), *lab.shape
    GUARD = 0x5A5A5A5A
    stream = torch.cuda.current_stream(cuda).cuda_stream
    labels, dims = _dev(lab.reshape(-1), cuda), _dev(np.array([H, W], np.int32), cuda)
    nreg = _dev(np.array([rows], np.int32), cuda)
    for mr, mv, mp in ((rows, 40, 1 << 10), (5, 1 << 10, 9), (rows, 0, 0), (rows, 1 << 10, 1 << 10)):
        want = ON.region_outlines(lab, max_regions=mr, max_vertices=mv)
        wpol = ON.simplify_outlines(want, RES, 0.0, mp)
        off = torch.full((mr + 1 + 8,), GUARD, dtype=torch.int32, device=cuda)
        verts = torch.full((mv + 8, 2), GUARD, dtype=torch.int32, device=cuda)
        cols = torch.full((mr + 2, 4), GUARD, dtype=torch.int64, device=cuda)
        meas = torch.full((mr + 2, 2), -7.0, dtype=torch.float64, device=cuda)
        poff = torch.full((mr + 1 + 8,), GUARD, dtype=torch.int32, device=cuda)
        pverts = torch.full((mp + 8, 2), -7.0, dtype=torch.float64, device=cuda)
        pol = torch.full((mr + 2, 8), -7.0, dtype=torch.float64, device=cuda)
        st, pst = torch.zeros(8, dtype=torch.float64, device=cuda), torch.zeros(8, dtype=torch.float64, device=cuda)
        ws = torch.empty(int(lib.dp_outline_workspace_size(H * W, mr, mv)), dtype=torch.uint8, device=cuda)
        assert lib.dp_region_outlines(labels.data_ptr(), dims.data_ptr(), H * W, nreg.data_ptr(), mr, mv, off.data_ptr(),
                                      verts.data_ptr(), cols.data_ptr(), meas.data_ptr(), st.data_ptr(), ws.data_ptr(), ws.numel(),
                                      stream) == 0
        assert lib.dp_simplify_outlines(off.data_ptr(), verts.data_ptr(), cols.data_ptr(), meas.data_ptr(), nreg.data_ptr(), mr, mv,
                                        RES, 0.0, mp, poff.data_ptr(), pverts.data_ptr(), pol.data_ptr(), pst.data_ptr(),
                                        ws.data_ptr(), ws.numel(), stream) == 0
        k = min(rows, mr)
        written, pwritten = int(want["offsets"][k]), int(wpol["offsets"][k])
        assert np.array_equal(st.cpu().numpy(), want["stats"]) and np.array_equal(pst.cpu().numpy(), wpol["stats"]), (mr, mv, mp)
        assert want["stats"][4] == (mv < full["stats"][2]) and want["stats"][5] == (mr < rows)
        assert np.array_equal(off.cpu().numpy()[:k + 1], want["offsets"]) and (off.cpu().numpy()[k + 1:] == GUARD).all()
        assert np.array_equal(verts.cpu().numpy()[:written], want["vertices"]) and (verts.cpu().numpy()[written:] == GUARD).all()
        assert np.array_equal(cols.cpu().numpy()[:k], want["columns"]) and (cols.cpu().numpy()[k:] == GUARD).all()
        assert np.array_equal(meas.cpu().numpy()[:k], want["measures"]) and (meas.cpu().numpy()[k:] == -7.0).all()
        assert np.array_equal(poff.cpu().numpy()[:k + 1], wpol["offsets"]) and (poff.cpu().numpy()[k + 1:] == GUARD).all()
        assert (pverts.cpu().numpy()[pwritten:] == -7.0).all() and (pol.cpu().numpy()[k:] == -7.0).all()
        assert np.array_equal(pol.cpu().numpy()[:k, [0, 1, 2, 6, 7]], wpol["polygons"][:, [0, 1, 2, 6, 7]])
        if mp == 9:
            assert 4 in wpol["polygons"][:, 6] and wpol["stats"][4] >= 1           # a polygon that does not fit
        if mv == 40:
            assert (wpol["polygons"][:, 6] == 4).sum() >= 5 and (wpol["polygons"][:, 6] == 0).sum() >= 4


def _summary(lab, cuda, pts=None, **kw):
    from depth_pro import pointcloud as PC

    plan = PC.floor_polygons(_plan(lab, cuda, **kw), None if pts is None else _dev(pts, cuda))
    return PC.floor_polygons_summary(plan)


def _boundary_distance(values):
    """Distance of each value from the nearest .3f rounding boundary (k + 0.5) * 1e-3."""
    q = np.asarray(values, np.float64) * 1e3
    return np.abs(q - np.floor(q) - 0.5) * 1e-3


@pytest.mark.gpu
def test_polygons_file_against_the_restatement(restated, gold, tmp_path, cuda):
    from depth_pro import pointcloud as PC

    lab, want = restated["shapes"]
    wpol = ON.simplify_outlines(want, RES, 0.025)
    kept = np.flatnonzero(wpol["polygons"][:, 6] == 0)
    unsnapped = [r for r in kept if wpol["polygons"][r, 2] == 0]
    assert len(unsnapped) >= 4 and len(kept) > len(unsnapped)
    pts = np.array([[0.0, 1.5, 0.0], [1.0, 2.25, 1.0], [0.5, 0.2, 0.5], [np.nan, 2.0, 0.0]])
    height = ON.mean_height(pts, None, 1.3)[0]
    assert height == 1.875
    # (a) no snapped polygon: the file's bytes
    sub = np.zeros_like(lab)
    for i, r in enumerate(unsnapped):
        sub[lab == r + 1] = i + 1
    wo = ON.region_outlines(sub)
    wp = ON.simplify_outlines(wo, RES, 0.025)
    assert (wp["polygons"][:, 2] == 0).all() and (wp["polygons"][:, 6] == 0).all()
    polys = [wp["vertices"][wp["offsets"][r]:wp["offsets"][r + 1]] for r in range(len(unsnapped))]
    text = ON.floorplan_text(polys, height, ORIGIN, RES)
    world = np.concatenate([ON.world_reference(p, ORIGIN, RES) for p in polys])
    assert _boundary_distance(world).min() >= 1e-4 and _boundary_distance([height]).min() >= 1e-4
    s = _summary(sub, cuda, pts)
    assert s["height"] == height and s["participants"] == 2 and [p["label"] for p in s["polygons"]] == list(range(1, len(polys) + 1))
    path = PC.export_floorplan_text(str(tmp_path / "a_floorplan.txt"), s)
    assert open(path, "rb").read() == text.encode()
    json.dumps(s)
    for p, w in zip(s["polygons"], polys):
        assert np.array_equal(p["vertices_grid"], w) and not p["snapped"]
        assert np.array_equal(p["vertices"], np.asarray(ORIGIN) + w * RES)
    # (b) with snapped ones: the parsed numbers at the .3f grain
    polys = [wpol["vertices"][wpol["offsets"][r]:wpol["offsets"][r + 1]] for r in kept]
    world = np.concatenate([ON.world_reference(p, ORIGIN, RES) for p in polys])
    assert _boundary_distance(world).min() >= 1e-4
    s = _summary(lab, cuda, pts)
    assert [p["label"] for p in s["polygons"]] == [int(r) + 1 for r in kept]
    assert sorted(d["label"] for d in s["dropped"]) == [int(r) + 1 for r in np.flatnonzero(wpol["polygons"][:, 6] != 0)]
    assert {d["reason"] for d in s["dropped"]} == {"too_small", "invalid"}
    path = PC.export_floorplan_text(str(tmp_path / "b_floorplan.txt"), s)
    got, exp = open(path).read().splitlines(), ON.floorplan_text(polys, height, ORIGIN, RES).splitlines()
    assert got[:5] == exp[:5] and len(got) == len(exp) == 5 + len(kept)
    for a, b in zip(got[5:], exp[5:]):
        fa, fb = [float(v) for v in a.split(", ")], [float(v) for v in b.split(", ")]
        assert len(fa) == len(fb) and np.abs(np.array(fa) - np.array(fb)).max() < 1e-9, (a, b)


@pytest.mark.gpu
def test_mean_height_against_numpy(floor_gold, cuda, record):
    from depth_pro import pointcloud as PC

    pts, count = floor_gold["cloud_points"], int(floor_gold["cloud_count"])
    worst = 0.0
    for thr, cnt in ((1.3, count), (float("nan"), count), (2.0, None), (1.3, 3000), (50.0, count)):
        got = PC.floor_mean_height(_dev(pts, cuda), cnt, thr).cpu().numpy()
        mean, n = ON.mean_height(pts, cnt, thr)
        rel = abs(got[0] - mean) / abs(mean)
        print(f"threshold {thr} count {cnt}: participants {n}, relative error {rel:.3e}")
        worst = max(worst, rel)
        assert got[1] == n and rel <= MEAN_REL, (thr, cnt, rel)
    assert ON.mean_height(pts, count, 50.0) == (50.0, 0)
    record("mean_height_rel", worst)


@pytest.mark.gpu
def test_generate_depth_maps_floor_polygons(tmp_path, cuda):
    """--floor_polygons on the ground fixture cloud: both new files exist and parse, the floor plan's own two files are
    byte-identical to a run without the flag, --resume skips the finished frame."""
    import torch
    from PIL import Image

    import generate_depth_maps as G
    from depth_pro import pointcloud as PC

    gg = np.load(os.path.join(GOLDEN, "golden_ground.npz"))
    src = tmp_path / "frames"
    src.mkdir()
    Image.open(os.path.join(GOLDEN, "data", "example.jpg")).convert("RGB").resize((128, 96)).save(src / "output_0000.png")
    calls = []

    class Model:
        def infer(self, x, f_px=None):
            calls.append(1)
            return {"depth": _dev(gg["flat_depth"], cuda).clone(), "focallength_px": torch.tensor(float(gg["flat_f"]), device=cuda)}

    kw = dict(pattern="output_*.png", model=(Model(), lambda im: torch.as_tensor(np.asarray(im))), stray_radius=0.25,
              stray_neighbors=12, floor_resolution=0.05, floor_height=float("nan"), floor_min_area=0.01)
    assert G.batch_generate_depth_maps(str(src), str(tmp_path / "plain"), floor_plan=True, **kw) == 1
    out = tmp_path / "out"
    assert G.batch_generate_depth_maps(str(src), str(out), floor_polygons=True, **kw) == 1
    assert sorted(os.listdir(out)) == ["ground.json", "output_0000_clean.ply", "output_0000_depth.png", "output_0000_floorplan.json",
                                       "output_0000_floorplan.png", "output_0000_floorplan.txt",
                                       "output_0000_floorplan_polygons.json"]
    for name in ("output_0000_floorplan.png", "output_0000_floorplan.json"):
        assert (out / name).read_bytes() == (tmp_path / "plain" / name).read_bytes(), name
    js = json.load(open(out / "output_0000_floorplan_polygons.json"))
    plain = json.load(open(out / "output_0000_floorplan.json"))
    assert js["origin"] == plain["origin"] and js["resolution"] == 0.05 and js["outline_stats"]["regions"] == plain["region_stats"]["regions"]
    assert js["polygon_stats"]["polygons"] == len(js["polygons"]) >= 1 and js["participants"] == plain["stats"]["participants"]
    cp, _ = PC.read_ply(str(out / "output_0000_clean.ply"))
    assert abs(js["height"] - cp[:, 1].mean()) <= 1e-12 * abs(cp[:, 1].mean())
    lines = open(out / "output_0000_floorplan.txt").read().splitlines()
    assert lines[:5] == ["# Floor Plan Data", "# Units: meters", "", "# Shapes by height",
                         "# Format: height, num_points, x1, z1, x2, z2, ..."] and len(lines) == 5 + len(js["polygons"])
    for line, p in zip(lines[5:], js["polygons"][::-1]):
        f = [float(v) for v in line.split(", ")]
        assert f[0] == round(js["height"], 3) and f[1] == len(p["vertices_grid"]) == (len(f) - 2) // 2 >= 3
        assert np.abs(np.array(f[2:]).reshape(-1, 2) - np.array(p["vertices_reference"])).max() <= 0.5e-3 + 1e-12
    done = len(calls)
    assert G.batch_generate_depth_maps(str(src), str(out), floor_polygons=True, resume=True, **kw) == 0 and len(calls) == done
