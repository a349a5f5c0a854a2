"""Height-sliced floor plan (additive to ABI 20, csrc/dp_slices.hip and dp_simplify_outlines_with of csrc/dp_outline.hip).

Expected values come from tests/slices_numpy.py, a sequential restatement of rules R1-R4, C1-C2, M1-M2 and the two
simplification parameters that composes tests/floorplan_numpy.py and tests/outline_numpy.py.  The non-GPU tests pin it:
the slice masks against numpy's literal `(y >= lo) & (y < hi)`, the integer closing-size rule against the reference's
float formula, the component count against scipy.ndimage.label, and tests/golden/golden_slices.npz (made by
tests/golden/make_golden_slices.py) against drift.  On the device every comparison is exact except a snapped rectangle's
corners, which keep tests/test_outline.py's rule (REL = 1e-12 of the diagonal).  Every output buffer of the raw calls has
guard words behind it, and a slice's cells past H * W are guard words too.
"""

import json
import os

import numpy as np
import pytest
from scipy import ndimage

import floorplan_numpy as FN
import outline_numpy as ON
import slices_numpy as SL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ONES3 = np.ones((3, 3), bool)
REL = 1e-12                     # tests/test_outline.py's margin for a snapped rectangle's corners
HMIN, HMAX = 0.1, 2.5
TRIPLES = [(0.1, 2.5, 5), (0.1, 2.5, 7), (0.0, 1.0, 3)]
OUTLINE_FIXTURES = ["shapes", "plus", "dots", "blob", "h1", "w1", "empty", "full"]
GUARD32, GUARD8, GUARDF = 0x5A5A5A5A, 0x5A, -7.0


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_slices.npz"))


@pytest.fixture(scope="module")
def room(gold):
    """The end-to-end room and what the restatement makes of it, computed once and never changed."""
    pts = gold["room_points"]
    plan = SL.sliced_floor_plan(pts)
    return pts, plan, SL.summary(plan)


def boundary_ys(b):
    """lo_s, hi_s and their nextafter neighbours for every slice."""
    ys = []
    for lo, hi, _ in b:
        for v in (lo, hi):
            ys += [v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)]
    return np.array(ys)


def raster_cloud(S, seed=3):
    """About 5 000 live rows for S slices of [0.1, 2.5): rows below and above every slice, NaN and Inf rows, every slice
    bound and its neighbours, equal (x, z) in different slices, 64 consecutive rows in one cell, and for S >= 4 a slice
    of exactly 9 rows (status 1), one of exactly 10 (kept) and one whose extent exceeds the capacity (status 2).
    Returns (points [n_max][3], live count, {role: slice})."""
    g = np.random.default_rng(seed + S)
    b = SL.bounds(HMIN, HMAX, S)
    roles = {"nine": 1, "ten": 2, "big": 3} if S >= 4 else {}
    bulk = [s for s in range(S) if s not in roles.values()]

    def rows(y, x=None, z=None):
        y = np.atleast_1d(np.asarray(y, np.float64))
        return np.column_stack([g.uniform(0.0, 3.0, len(y)) if x is None else np.full(len(y), x), y,
                                g.uniform(0.0, 2.0, len(y)) if z is None else np.full(len(y), z)])

    parts = [rows(boundary_ys(b)), rows(g.uniform(-0.2, HMIN - 1e-9, 100)), rows(g.uniform(HMAX, 2.8, 100)),
             np.array([[np.nan, 1.0, 1.0], [1.0, np.nan, 1.0], [1.0, 1.0, np.inf], [-np.inf, 0.5, 0.5], [0.3, np.inf, 0.2],
                       [np.nan, np.nan, np.nan]])]
    run = rows(np.full(64, b[bulk[0], 2]), 1.01, 0.52) + g.uniform(0, 1e-3, (64, 3)) * [1, 0, 1]         # one cell, 64 rows
    for s in bulk:                                           # equal x and z in different slices: the join key
        parts.append(rows([b[s, 2]] * 2, 2.2, 1.3))
    per = max(8, 4400 // len(bulk))
    for s in bulk:
        parts.append(rows(g.uniform(b[s, 0] + 1e-6, b[s, 1] - 1e-6, per)))
    pts = np.concatenate(parts)
    have = [int(m.sum()) for m in SL.masks(pts, b)]
    for role, want in (("nine", 9), ("ten", 10), ("big", 14)):
        if role in roles:
            s = roles[role]
            assert have[s] <= want, (role, have[s])
            extra = rows(np.full(want - have[s], b[s, 2]))
            if role == "big":
                extra[:2, 0] = (-60.0, 60.0)
            pts = np.concatenate([pts, extra])
    pts = pts[g.permutation(len(pts))]
    pts = np.concatenate([pts[:1000], run, pts[1000:]])      # the 64 rows stay consecutive, and straddle two waves
    n = len(pts)
    tail = rows(g.uniform(HMIN, HMAX, 37))                   # past n_dev: in range, never read
    return np.concatenate([pts, tail]), n, roles


# ---- no GPU ---------------------------------------------------------------------------------------------

def test_slice_masks_are_numpys_literal_comparisons():
    """R2: the restatement's masks equal (y >= lo) & (y < hi) as the reference writes its loop, on a cloud that holds
    every bound and its neighbours; one of the triples has a slice with hi_s != lo_{s+1}."""
    differing = {}
    for hmin, hmax, S in TRIPLES:
        b = SL.bounds(hmin, hmax, S)
        slice_height = (hmax - hmin) / S
        y = np.concatenate([boundary_ys(b), np.linspace(hmin - 0.2, hmax + 0.2, 41), [np.nan, np.inf, -np.inf]])
        pts = np.column_stack([np.zeros_like(y), y, np.ones_like(y)])
        got = SL.masks(pts, b)
        taken = np.zeros(len(y), int)
        for i in range(S):
            slice_start = hmin + i * slice_height
            slice_end = slice_start + slice_height
            assert (b[i, 0], b[i, 1], b[i, 2]) == (slice_start, slice_end, (slice_start + slice_end) / 2)
            with np.errstate(invalid="ignore"):
                want = (pts[:, 1] >= slice_start) & (pts[:, 1] < slice_end) & np.isfinite(pts[:, 1])
            assert np.array_equal(got[i], want), (hmin, hmax, S, i)
            taken += want
        differing[(hmin, hmax, S)] = [s for s in range(S - 1) if b[s, 1] != b[s + 1, 0]]
        if differing[(hmin, hmax, S)]:
            assert (taken[np.isfinite(y) & (y >= b[0, 0]) & (y < b[-1, 1])] != 1).any()     # a row in two slices or in none
    assert differing[(0.1, 2.5, 7)], differing


def test_integer_closing_rule_is_the_reference_float_formula():
    """C2 against max(3, min(11, int(np.sqrt(cells / comps) / 5))) made odd: at every threshold 25 m^2 comps and beside
    it for comps 1..1000, and on random pairs up to 2^26 cells."""
    for comps in range(1, 1001):
        for m in range(3, 12):
            for cells in (25 * m * m * comps - 1, 25 * m * m * comps, 25 * m * m * comps + 1):
                assert SL.closing_size(cells, comps) == SL.closing_size_float(cells, comps), (cells, comps)
    assert SL.closing_size(0, 0) == SL.closing_size_float(0, 0) == 3
    assert [SL.closing_size(c, 1) for c in (399, 400, 899, 900, 1599, 1600, 2499, 2500, 10 ** 7)] == [3, 5, 5, 7, 7, 9, 9, 11, 11]
    g = np.random.default_rng(17)
    cells = g.integers(1, 1 << 26, 20000, endpoint=True)
    comps = np.minimum(cells, g.integers(1, 1 << 16, 20000))
    for c, k in zip(cells.tolist(), comps.tolist()):
        assert SL.closing_size(c, k) == SL.closing_size_float(c, k), (c, k)


def closing_grids():
    """Stacked raw grids of at most 70 x 130 whose (cells, comps) sit on both sides of every threshold of C2, an empty
    grid, and the one-cell-wide spiral of golden_floorplan.npz.  [(grid, cells, comps, size)]."""
    def block(*counts):
        grid = np.zeros((70, 130), np.uint8)
        for k, n in enumerate(counts):                      # each component: the first n cells of a 60-column band
            band = grid[:, 65 * k:65 * k + 60]
            flat = np.zeros(band.size, np.uint8)
            flat[:n] = 1
            band[:] = flat.reshape(band.shape)
        return grid

    fg = np.load(os.path.join(GOLDEN, "golden_floorplan.npz"))
    spiral = (fg["region_spiral_labels"] != 0).astype(np.uint8)
    cases = [(block(399), 3), (block(400), 5), (block(899, 900), 5), (block(899, 901), 7), (block(1599), 7), (block(1600), 9),
             (block(2499), 9), (block(2500), 11), (block(), 3), (np.zeros((0, 0), np.uint8), 3), (spiral, None),
             (block(400)[:7, :60].copy(), None)]
    out = []
    for grid, size in cases:
        cells, comps = SL.components(grid)
        k = SL.closing_size(cells, comps)
        assert size is None or k == size
        out.append((grid, cells, comps, k))
    assert out[10][0].shape == (65, 130) and out[10][2] == 1
    return out


def test_component_count_is_scipys(gold):
    """C1 against scipy.ndimage.label with a 3 x 3 structure of ones."""
    grids = [g for g, _, _, _ in closing_grids()] + [gold[f"slice{s}_cleaned"] for s in range(5)]
    r = np.random.default_rng(5)
    grids += [(r.random((24, 31)) < r.uniform(0.2, 0.7)).astype(np.uint8) for _ in range(20)]
    for grid in grids:
        want = ndimage.label(grid, structure=ONES3)[1] if grid.size else 0
        assert SL.components(grid) == (int(np.count_nonzero(grid)), want)
    assert {SL.closing_size(*SL.components(g)[:2]) for g in grids} >= {3, 5, 7, 9, 11}


def test_text_file_from_a_hand_written_summary(tmp_path):
    from depth_pro import pointcloud as PC

    tri, quad = [[0.0, 1.0], [2.0, 1.0005], [2.0, 3.0]], [[-1.0, 0.25], [0.5, 0.5], [0.0, 7.0], [1.0, 1.0]]
    summary = {"slices": [
        {"index": 1, "height": 0.82, "status": "ok", "polygons": [{"label": 2, "vertices_reference": quad}]},
        {"index": 0, "height": 0.34, "status": "ok", "polygons": [{"label": 1, "vertices_reference": tri},
                                                                   {"label": 4, "vertices_reference": quad}]},
        {"index": 2, "height": 1.3, "status": "too_few_points", "polygons": []},
        {"index": 3, "height": 1.78049, "status": "ok", "polygons": [{"label": 1, "vertices_reference": tri}]}]}
    path = PC.export_sliced_floorplan_text(str(tmp_path / "s.txt"), summary)
    assert open(path).read() == (
        "# Floor Plan Data\n# Units: meters\n\n# Shapes by height\n# Format: height, num_points, x1, z1, x2, z2, ...\n"
        "0.340, 4, -1.000, 0.250, 0.500, 0.500, 0.000, 7.000, 1.000, 1.000\n"
        "0.340, 3, 0.000, 1.000, 2.000, 1.000, 2.000, 3.000\n"
        "0.820, 4, -1.000, 0.250, 0.500, 0.500, 0.000, 7.000, 1.000, 1.000\n"
        "1.780, 3, 0.000, 1.000, 2.000, 1.000, 2.000, 3.000\n")
    assert not os.path.exists(path + ".tmp")


def test_restatement_reproduces_the_golden_file(gold, room):
    pts, plan, summary = room
    for k in ("bounds", "stats", "dims", "origin"):
        assert np.array_equal(plan[k], gold[k]), k
    assert np.array_equal(np.array(plan["counts"]), gold["counts"]) and np.array_equal(plan["close_size"], gold["close_size"])
    for s in range(5):
        assert np.array_equal(plan["cleaned"][s], gold[f"slice{s}_cleaned"])
        for k in ("polygons", "offsets", "stats"):
            assert np.array_equal(plan["polygons"][s][k], gold[f"slice{s}_poly_{k}"]), (s, k)
        assert np.abs(plan["polygons"][s]["vertices"] - gold[f"slice{s}_poly_vertices"]).max(initial=0.0) <= 1e-12
    # what the end-to-end device test stands on: polygons in at least three slices, two closing sizes, an empty slice,
    # and a gap that the 3 x 3 closing leaves open and the slice's own size closes
    assert sum(1 for sl in summary if sl["polygons"]) >= 3 and len({sl["close_size"] for sl in summary if sl["status"] == "ok"}) >= 2
    assert [sl["status"] for sl in summary].count("too_few_points") == 1 and summary[2]["participants"] == 0
    s = 3
    assert plan["close_size"][s] > 3
    open3 = FN.label(SL.slice_morphology(plan["grids"][s]["occupied"], 3))[1]
    assert open3 == summary[s]["region_stats"]["regions"] + 1 == 3
    json.dumps(summary)


def test_simplification_parameters_change_what_is_kept():
    """On the fixtures of golden_outline.npz a region is kept under (min_area / 4, 0.005) and dropped under (0.1, 0.01);
    with the first pair simplify_outlines_with's restatement is outline_numpy's simplify_outlines."""
    og = np.load(os.path.join(GOLDEN, "golden_outline.npz"))
    flipped = 0
    for name in OUTLINE_FIXTURES:
        o = ON.region_outlines(og[f"{name}_labels"])
        a, b = SL.simplify_outlines_with(o, 0.1, 0.025 / 4, 0.005), SL.simplify_outlines_with(o, 0.1, 0.1, 0.01)
        want = ON.simplify_outlines(o, 0.1, 0.025)
        for k in ("offsets", "vertices", "polygons", "stats"):
            assert np.array_equal(a[k], want[k]), (name, k)
        flipped += int(((a["polygons"][:, 6] == 0) & (b["polygons"][:, 6] == 1)).sum())
    assert flipped >= 1


def test_parser_and_stage_table(monkeypatch, tmp_path):
    import sys

    import generate_depth_maps as G

    got = G.resolve_stages(output_dir="OUT", floor_slices=5)
    assert list(got) == ["cloud", "ground", "clean", "slices"]
    assert got["slices"] == {"num_slices": 5, "height_min": 0.1, "height_max": 2.5, "resolution": 0.05, "min_area": 0.1}
    assert "slices" not in G.resolve_stages(output_dir="OUT", floor_polygons=True, floor_slice_min=9.0)      # off: not looked at
    st = {s.name: s for s in G.STAGES}["slices"]
    assert st.implies == "clean" and st.suffixes == ("_floorslices.txt", "_floorslices.json")
    for kw in (dict(floor_slices=33), dict(floor_slices=-1), dict(floor_slices=5, floor_slice_min=2.5),
               dict(floor_slices=5, floor_slice_resolution=0.0), dict(floor_slices=5, floor_slice_min_area=-1.0)):
        with pytest.raises(ValueError, match="--floor_slice"):
            G.resolve_stages(output_dir="OUT", **kw)
    seen = []
    monkeypatch.setattr(G, "batch_generate_depth_maps", lambda *a, **kw: seen.append(kw) or 0)
    monkeypatch.setattr(G, "_model", lambda *a, **k: pytest.fail("the model was loaded"))
    base = ["generate_depth_maps.py", "--input_dir", str(tmp_path)]
    monkeypatch.setattr(sys, "argv", base)
    G.main()
    new = {"floor_slices": 5, "floor_slice_min": 0.2, "floor_slice_max": 2.0, "floor_slice_resolution": 0.1, "floor_slice_min_area": 0.05}
    monkeypatch.setattr(sys, "argv", base + ["--floor_slices", "5", "--floor_slice_min", "0.2", "--floor_slice_max", "2.0",
                                             "--floor_slice_resolution", "0.1", "--floor_slice_min_area", "0.05"])
    G.main()
    assert not any(k.startswith("floor_slice") for k in seen[0])
    assert {k: v for k, v in seen[1].items() if k not in seen[0]} == new and {k: v for k, v in seen[1].items() if k in seen[0]} == seen[0]
    assert list(G.resolve_stages(**seen[1])) == ["cloud", "ground", "clean", "slices"]
    monkeypatch.setattr(sys, "argv", base + ["--floor_slices", "40"])
    with pytest.raises(SystemExit) as e:
        G.main()
    assert e.value.code == 2
    frames = [str(tmp_path / f"f{k}.png") for k in range(2)]
    for k in (0, 1):
        for s in ("depth.png", "clean.ply", "floorslices.txt"):
            (tmp_path / f"f{k}_{s}").write_bytes(b"")
    (tmp_path / "f0_floorslices.json").write_bytes(b"")
    assert G.plan_frames(frames, str(tmp_path), 1, 0, True, stages=("clean", "slices")) == [1]


def test_argument_errors_need_no_device():
    import ctypes

    import torch

    from depth_pro import _lib
    from depth_pro import pointcloud as PC

    lib = _lib.load()
    size = lib.dp_slices_workspace_size
    assert size(0, 0) > 0 and size(1, 1000) < size(2, 1000) < size(2, 2000) and size(5, 1 << 20) >= 4 * 5 * (1 << 20)
    assert _lib.DP_SLICE_MAX == SL.SLICE_MAX == PC.SLICE_MAX and _lib.DP_ABI_VERSION == 20 and len(PC.SLICE_STATS) == 8
    P, big, ARG, SHAPE = 4096, 1 << 40, 1000, 1001
    f64 = ctypes.c_double

    def grids(points=P, n=8, hmin=0.1, hmax=2.5, S=5, res=0.05, pad=0.5, mp=10, mc=64, den=P, hgt=P, occ=P, dims=P, org=P, bnd=P,
              st=P, ws=P, wsb=big):
        return lib.dp_slice_grids(points, None, n, f64(hmin), f64(hmax), S, f64(res), f64(pad), mp, mc, den, hgt, occ, dims, org, bnd,
                                  st, ws, wsb, None)

    def sizes(grid=P, dims=P, S=5, mc=64, out=P, counts=P, ws=P, wsb=big):
        return lib.dp_slice_closing_sizes(grid, dims, S, mc, out, counts, ws, wsb, None)

    def morph(grid=P, dims=P, S=5, mc=64, cs=P, iters=1, osz=3, out=P, ws=P, wsb=big):
        return lib.dp_slice_morphology(grid, dims, S, mc, cs, iters, osz, out, ws, wsb, None)

    def simp(off=P, verts=P, cols=P, meas=P, n=P, mr=16, mv=64, res=0.1, floor=0.1, alpha=0.01, mp=64, poff=P, pv=P, pol=P, stats=P,
             ws=P, wsb=big):
        return lib.dp_simplify_outlines_with(off, verts, cols, meas, n, mr, mv, f64(res), f64(floor), f64(alpha), mp, poff, pv, pol,
                                             stats, ws, wsb, None)

    for kw in ({"S": 0}, {"S": 33}, {"mc": -1}, {"S": 32, "mc": 1 << 26}, {"n": -1}, {"mp": -1}, {"res": 0.0}, {"res": float("nan")},
               {"pad": -1.0}, {"pad": float("inf")}, {"hmin": 2.5}, {"hmax": float("inf")}, {"hmin": float("nan")}):
        assert grids(**kw) == SHAPE, kw
    for kw in ({"points": None}, {"den": None}, {"hgt": None}, {"occ": None}, {"dims": None}, {"org": None}, {"bnd": None},
               {"st": None}, {"ws": None}, {"ws": P + 4}, {"wsb": size(5, 64) - 1}):
        assert grids(**kw) == ARG, kw
    for call in (sizes, morph):
        for kw in ({"S": 0}, {"S": 33}, {"mc": -1}, {"S": 32, "mc": 1 << 26}):
            assert call(**kw) == SHAPE, kw
        for kw in ({"grid": None}, {"dims": None}, {"out": None}, {"ws": None}, {"ws": P + 4}, {"wsb": size(5, 64) - 1}):
            assert call(**kw) == ARG, kw
    assert sizes(counts=None) == ARG and morph(cs=None) == ARG
    for kw in ({"iters": -1}, {"osz": 0}, {"osz": 4}, {"osz": 17}):
        assert morph(**kw) == SHAPE, kw
    for kw in ({"floor": -0.1}, {"floor": float("nan")}, {"alpha": -1.0}, {"alpha": float("inf")}, {"res": 0.0}, {"mp": -1}):
        assert simp(**kw) == SHAPE, kw
    for kw in ({"off": None}, {"pol": None}, {"ws": None}):
        assert simp(**kw) == ARG, kw
    host = torch.zeros(8, 3, dtype=torch.float64)
    with pytest.raises(_lib.DPError):
        PC.slice_grids(host)
    with pytest.raises(_lib.DPError):
        PC.slice_closing_sizes(torch.zeros(2, 16, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.int32))
    for call in (lambda: PC.slice_grids(host, num_slices=0), lambda: PC.slice_grids(host, num_slices=33),
                 lambda: PC.slice_grids(host, height_min=3.0), lambda: PC.sliced_floor_plan(host, alpha=-1.0),
                 lambda: PC.sliced_floor_plan(host, min_area=float("nan")), lambda: PC.sliced_floor_plan_summary({}),
                 lambda: PC.slice_morphology(torch.zeros(2, 16, dtype=torch.uint8), torch.zeros(2, 2, dtype=torch.int32),
                                             torch.zeros(2, dtype=torch.int32), open_size=4)):
        with pytest.raises(ValueError):
            call()


# ---- GPU ------------------------------------------------------------------------------------------------

def _dev(a, cuda):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _guarded(shape, dtype, fill, cuda, extra=64):
    """A flat buffer of prod(shape) + extra elements, all `fill`."""
    import torch

    return torch.full((int(np.prod(shape)) + extra,), fill, dtype=dtype, device=cuda)


def _stack(grids, mc, fill=GUARD8):
    """(S, mc) uint8: each grid row-major at the front of its row, `fill` behind it; and its dims."""
    out = np.full((len(grids), mc), fill, np.uint8)
    dims = np.zeros((len(grids), 2), np.int32)
    for s, g in enumerate(grids):
        out[s, :g.size] = g.reshape(-1)
        dims[s] = g.shape
    return out, dims


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 5, 7, 32])
def test_slice_grids_against_the_restatement(S, cuda):
    import torch

    from depth_pro import _lib

    lib = _lib.load()
    pts, n, roles = raster_cloud(S)
    mc = 8192
    want = SL.slice_grids(pts, n, HMIN, HMAX, S, 0.05, 0.5, 10, mc)
    b, st = want["bounds"], want["stats"]
    assert 4500 <= n <= 5500 and n < len(pts)
    both = np.sum(SL.masks(pts[:n], b), axis=0)
    inside = np.isfinite(pts[:n]).all(axis=1) & (pts[:n, 1] >= b[0, 0]) & (pts[:n, 1] < b[-1, 1])
    differs = any(b[s, 1] != b[s + 1, 0] for s in range(S - 1))
    assert differs == bool((both == 2).any() or (both[inside] == 0).any())    # a row in two slices, or between two
    assert differs or S != 7                                                  # (0.1, 2.5, 7): the non-GPU test's differing triple
    if S > 1:
        assert st[roles["nine"], 0] == 9 and st[roles["nine"], 5] == 1 and st[roles["ten"], 0] == 10 and st[roles["ten"], 5] == 0
        assert st[roles["big"], 5] == 2 and (st[[s for s in range(S) if s not in roles.values()], 5] == 0).all()
    assert max(g["density"].max() for g in want["grids"] if g is not None) >= 64
    stream = torch.cuda.current_stream(cuda).cuda_stream
    den = _guarded((S, mc), torch.int32, GUARD32, cuda)
    hgt = _guarded((S, mc), torch.float32, GUARDF, cuda)
    occ = _guarded((S, mc), torch.uint8, GUARD8, cuda)
    dims = _guarded((S, 2), torch.int32, GUARD32, cuda)
    org, bnd, stats = (_guarded((S, k), torch.float64, GUARDF, cuda) for k in (2, 3, 8))
    ws = torch.empty(int(lib.dp_slices_workspace_size(S, mc)), dtype=torch.uint8, device=cuda)
    dpts, dn = _dev(pts, cuda), _dev(np.array([n], np.int32), cuda)
    assert lib.dp_slice_grids(dpts.data_ptr(), dn.data_ptr(), len(pts), HMIN, HMAX, S,
                              0.05, 0.5, 10, mc, den.data_ptr(), hgt.data_ptr(), occ.data_ptr(), dims.data_ptr(), org.data_ptr(),
                              bnd.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), stream) == 0
    den, hgt, occ = den.cpu().numpy(), hgt.cpu().numpy(), occ.cpu().numpy()
    for t, k, guard in ((dims, 2, GUARD32), (org, 2, GUARDF), (bnd, 3, GUARDF), (stats, 8, GUARDF)):
        assert (t.cpu().numpy()[S * k:] == guard).all()
    assert np.array_equal(dims.cpu().numpy()[:2 * S].reshape(S, 2), want["dims"])
    assert np.array_equal(org.cpu().numpy()[:2 * S].reshape(S, 2), want["origin"])
    assert np.array_equal(bnd.cpu().numpy()[:3 * S].reshape(S, 3), b)
    assert np.array_equal(stats.cpu().numpy()[:8 * S].reshape(S, 8), st), (stats.cpu().numpy()[:8 * S].reshape(S, 8), st)
    assert (den[S * mc:] == GUARD32).all() and (hgt[S * mc:] == GUARDF).all() and (occ[S * mc:] == GUARD8).all()
    for s, g in enumerate(want["grids"]):
        cells = 0 if g is None else g["density"].size
        lo = s * mc
        assert (den[lo + cells:lo + mc] == GUARD32).all() and (hgt[lo + cells:lo + mc] == GUARDF).all(), s
        assert (occ[lo + cells:lo + mc] == GUARD8).all(), s
        if g is not None:
            assert np.array_equal(den[lo:lo + cells].view(np.uint32), g["density"].reshape(-1)), s
            assert np.array_equal(hgt[lo:lo + cells], g["height"].reshape(-1)) and np.array_equal(occ[lo:lo + cells], g["occupied"].reshape(-1)), s


@pytest.mark.gpu
def test_closing_sizes_against_the_restatement(cuda):
    import torch

    from depth_pro import _lib

    lib = _lib.load()
    cases = closing_grids()
    S, mc = len(cases), 70 * 130
    grid, dims = _stack([c[0] for c in cases], mc, fill=1)                  # set cells behind a grid are not its cells
    size = _guarded((S,), torch.int32, GUARD32, cuda)
    counts = _guarded((S, 2), torch.int64, GUARD32, cuda)
    ws = torch.empty(int(lib.dp_slices_workspace_size(S, mc)), dtype=torch.uint8, device=cuda)
    dgrid, ddims = _dev(grid, cuda), _dev(dims, cuda)
    assert lib.dp_slice_closing_sizes(dgrid.data_ptr(), ddims.data_ptr(), S, mc, size.data_ptr(),
                                      counts.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(cuda).cuda_stream) == 0
    size, counts = size.cpu().numpy(), counts.cpu().numpy()
    assert (size[S:] == GUARD32).all() and (counts[2 * S:] == GUARD32).all()
    assert counts[:2 * S].reshape(S, 2).tolist() == [[c[1], c[2]] for c in cases]
    assert size[:S].tolist() == [c[3] for c in cases] and set(size[:S].tolist()) == {3, 5, 7, 9, 11}


@pytest.mark.gpu
def test_morphology_with_device_sizes(cuda):
    import torch

    from depth_pro import pointcloud as PC

    g = np.random.default_rng(23)
    wide = (g.random((65, 130)) < 0.35).astype(np.uint8)
    wide[7, 58:71] = 1                                                       # a set run across the word boundary at 64
    wide[20:23, 60:68] = 0
    grids = [(g.random((5, 70)) < 0.5).astype(np.uint8), wide, np.ones((1, 1), np.uint8), np.zeros((0, 0), np.uint8)]
    mc = 65 * 130
    stack, dims = _stack(grids, mc)
    for sizes in ([3, 11, 7, 1], [4, 17, 0, -3], [11, 3, 15, 5]):
        out = torch.full((4 * mc + 64,), GUARD8, dtype=torch.uint8, device=cuda)
        got = PC.slice_morphology(_dev(stack, cuda), _dev(dims, cuda), _dev(np.array(sizes, np.int32), cuda), 1, 3,
                                  out=out[:4 * mc].view(4, mc))
        host = out.cpu().numpy()
        assert got.data_ptr() == out.data_ptr() and (host[4 * mc:] == GUARD8).all()
        for s, grid in enumerate(grids):
            want = SL.slice_morphology(grid, sizes[s], 1, 3)
            assert np.array_equal(host[s * mc:s * mc + grid.size].reshape(grid.shape), want), (sizes, s)
            assert (host[s * mc + grid.size:(s + 1) * mc] == GUARD8).all(), (sizes, s)
        if sizes[0] == 4:                                                    # not odd, too large, 0, negative: all act as 1
            for s, grid in enumerate(grids):
                assert np.array_equal(host[s * mc:s * mc + grid.size].reshape(grid.shape), FN.morphology(grid, 1, 1, 3))
    # two closings, no opening; in place
    buf = _dev(stack, cuda)
    PC.slice_morphology(buf, _dev(dims, cuda), _dev(np.array([5, 7, 3, 3], np.int32), cuda), 2, 1, out=buf)
    for s, grid in enumerate(grids):
        assert np.array_equal(buf[s, :grid.size].cpu().numpy().reshape(grid.shape), FN.morphology(grid, [5, 7, 3, 3][s], 2, 1))


@pytest.mark.gpu
def test_morphology_full_word_rows_inside_a_stack(cuda):
    """Rows of 63, 64 and 65 cells (the last word one bit short, exactly full, one bit into the next) stacked so that the
    full-word grid sits at a non-zero slice: the tail mask beside the slice's cell and word offsets."""
    import torch

    from depth_pro import pointcloud as PC

    fg = np.load(os.path.join(GOLDEN, "golden_floorplan.npz"))
    sizes, mc = [7, 3, 11, 5], 37 * 65 + 5
    for names in (("random_37x63", "random_37x64", "random_37x65", "random_1x1"), ("random_37x63", "holes_37x64", "frame_37x65", "random_1x1")):
        grids = [fg[f"morph_{n}"] for n in names]
        assert [g.shape for g in grids] == [(37, 63), (37, 64), (37, 65), (1, 1)]
        stack, dims = _stack(grids, mc)
        out = torch.full((4 * mc + 64,), GUARD8, dtype=torch.uint8, device=cuda)
        PC.slice_morphology(_dev(stack, cuda), _dev(dims, cuda), _dev(np.array(sizes, np.int32), cuda), 1, 3, out=out[:4 * mc].view(4, mc))
        host = out.cpu().numpy()
        assert (host[4 * mc:] == GUARD8).all()
        for s, grid in enumerate(grids):
            assert np.array_equal(host[s * mc:s * mc + grid.size].reshape(grid.shape), FN.morphology(grid, sizes[s], 1, 3)), (names, s)
            assert (host[s * mc + grid.size:(s + 1) * mc] == GUARD8).all(), (names, s)


@pytest.mark.gpu
@pytest.mark.parametrize("name", OUTLINE_FIXTURES)
def test_simplify_outlines_with(name, cuda):
    import torch

    from depth_pro import pointcloud as PC
    from test_outline import RES, _plan, _same_polygons

    og = np.load(os.path.join(GOLDEN, "golden_outline.npz"))
    lab = og[f"{name}_labels"]
    want = ON.region_outlines(lab)
    plan = PC.region_outlines(_plan(lab, cuda), max_vertices=1 << 14)
    keys = ("polygon_offsets", "polygon_vertices", "polygons", "polygon_stats")
    old = {k: v.clone() for k, v in PC.simplify_outlines(plan, max_polygon_vertices=1 << 13).items() if k in keys}
    used = int(old["polygon_offsets"].max().item())
    new = PC.simplify_outlines_with(plan, 0.025 / 4, 0.005, max_polygon_vertices=1 << 13)
    for k in keys:                                                           # bit for bit (vertices: the part that is written)
        a, b = (old[k][:used], new[k][:used]) if k == "polygon_vertices" else (old[k], new[k])
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b), k
    _same_polygons(PC.simplify_outlines_with(plan, 0.1, 0.01, max_polygon_vertices=1 << 13), SL.simplify_outlines_with(want, RES, 0.1, 0.01))


def _same_summary(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        for k in b:
            if k == "polygons":
                assert SL.polygon_lists_close(a[k], b[k], REL), (b["index"], a[k], b[k])
            elif k == "polygon_stats":
                assert {x: v for x, v in a[k].items()} == b[k], (b["index"], a[k], b[k])
            else:
                assert a[k] == b[k], (b["index"], k, a[k], b[k])
        assert set(a) == set(b)


@pytest.mark.gpu
def test_sliced_floor_plan_end_to_end(room, tmp_path, cuda):
    from depth_pro import pointcloud as PC

    pts, _, want = room
    plan = PC.sliced_floor_plan(_dev(pts, cuda), max_cells=1 << 14, max_regions=64, max_vertices=1 << 12, max_polygon_vertices=1 << 10)
    got = PC.sliced_floor_plan_summary(plan)
    json.dumps(got)
    assert got["resolution"] == 0.05 and got["parameters"]["min_area"] == 0.1 and got["parameters"]["alpha"] == 0.01
    _same_summary(got["slices"], want)
    path = PC.export_sliced_floorplan_text(str(tmp_path / "room_floorslices.txt"), got)
    assert open(path, "rb").read() == SL.floorplan_text(want).encode()
    assert len(open(path).read().splitlines()) == 5 + sum(len(sl["polygons"]) for sl in want) >= 8
