"""The L-shape split (additive to ABI 20, csrc/dp_lshape.hip): dp_shape_rectangles and dp_lshape_split against the
numpy restatement of the header's rules (tests/lshape_numpy.py), which the golden fixture
(tests/golden/golden_lshape.npz, computed a second way by make_golden_lshape.py) pins.

Tolerance of the GPU comparisons: statuses, counts, gw / gh, cell counts and the order of the output rows
are compared exactly.  An output row's numbers are compared within 16 * 2^-52 * (|cu| + |cv| + w + h) of the
input rectangle the row came from (`sources`): the device's sin and cos may differ from libm's by an ulp or
two, and each number is a handful of rounded operations on values of that size.
"""

import json
import math
import os

import numpy as np
import pytest

import lshape_numpy as LN
import shapes_numpy as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = ["slabs", "room", "true_L", "small", "few", "thin", "full", "sparse", "few_parts", "thin_parts", "holes",
          "halves", "long", "cap", "strangers"]
ULP = 2.0 ** -52


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(GOLDEN, "golden_lshape.npz")) as z:
        return {k: z[k] for k in z.files}


def scene(gold, name):
    return {k.split(".", 1)[1]: v for k, v in gold.items() if k.startswith(name + ".")}


def sources(rects, info):
    """The input rectangle of every output row: a split rectangle (status 0) gives one row per listed part, every
    other rectangle one row."""
    rects, info = np.asarray(rects).reshape(-1, 8), np.asarray(info).reshape(-1, 8)
    reps = [int(i[6]) if i[0] == 0 else 1 for i in info]
    return np.repeat(rects, reps, axis=0)


def rows_close(got, want, src):
    """Rows equal within the module's tolerance: row k within 16 ulp of |cu| + |cv| + w + h of src[k], the rectangle
    it came from.  Returns the largest error over its own bound."""
    got, want, src = np.asarray(got), np.asarray(want), np.asarray(src)
    assert got.shape == want.shape and len(src) == len(got), (got.shape, want.shape, src.shape)
    assert np.array_equal(got[:, 5:], want[:, 5:])
    if not len(got):
        return 0.0
    bound = 16 * ULP * (np.abs(src[:, 0]) + np.abs(src[:, 1]) + src[:, 2] + src[:, 3])
    err = np.abs(got[:, :5] - want[:, :5]).max(axis=1)
    print("largest error / bound per row:", np.round(err / bound, 3).tolist())
    assert (err <= bound).all(), (err, bound)
    return float((err / bound).max())


# ---- no GPU -------------------------------------------------------------------------------------------

def test_fixture_scenes_are_the_listed_ones(gold):
    assert sorted(gold["names"].tolist()) == sorted(SCENES)
    seen = set()
    for name in SCENES:
        seen |= set(scene(gold, name)["info"][:, 0].astype(int).tolist())
    assert seen == set(range(10))


@pytest.mark.parametrize("name", SCENES)
def test_restatement_equals_fixture(name, gold):
    sc = scene(gold, name)
    rows, n_out, info = LN.split_l_shapes(sc["points"], sc["labels"], sc["rects"], int(sc["max_cells"]))
    assert np.array_equal(info, sc["info"])
    assert n_out == (len(sc["out"]), 0) and np.array_equal(rows, sc["out"])
    if name == "halves":
        assert np.array_equal(LN.rectangle_list(sc["shapes"]), sc["rects"])


def test_what_the_scenes_pin(gold):
    """`true_L`, one connected L, is kept (status 6): the case the reference's name promises and its code does not
    deliver.  `strangers`: noise and another cluster's points decide the outcome; members only would keep it."""
    assert scene(gold, "true_L")["info"][0, 0] == 6
    sc = scene(gold, "strangers")
    assert sc["info"][0, 0] == 0 and len(sc["out"]) == 2
    own = np.where(sc["labels"] == 0, 0, -2)
    assert LN.split_l_shapes(sc["points"], own, sc["rects"])[2][0, 0] == 5
    sc = scene(gold, "holes")
    assert sc["info"][0, 4] == 6                       # of the 5- and the 6-cell region only the second counts
    room = scene(gold, "room")
    assert room["out"][0, 2] * room["out"][0, 3] > 0.95 * room["rects"][0, 2] * room["rects"][0, 3]


def test_shape_summary_without_the_new_arguments_is_unchanged(gold):
    from depth_pro import pointcloud as PC

    t = scene(gold, "halves")["shapes"]
    base = PC.shape_summary(t, {"eps": 0.2})
    assert sorted(base) == ["circles", "clusters_listed", "errors", "parameters", "rectangles", "skipped"]
    assert [r["split"] for r in base["rectangles"]] == [True, True] and "l_part" not in base["rectangles"][0]
    want = [tuple(float(v) for v in q) for q in PC.split_large_rectangle(2.0, 2.0, 12.1, 9.1, 20.0)]
    assert [(r["center"][0], r["center"][1], r["width"], r["height"], r["angle"]) for r in base["rectangles"]] == want
    # the host list is the restatement's rectangle list
    assert np.array_equal(np.array(want), LN.rectangle_list(t)[:, :5])
    sc = scene(gold, "slabs")
    shapes = np.zeros((3, 16))
    shapes[:, 0], shapes[:, 1] = 1, 720
    shapes[:, 2:7] = sc["rects"][:, :5]
    full = PC.shape_summary(shapes, {}, sc["out"], sc["info"])
    assert full["l_split"] is True and len(full["rectangles"]) == 6 and len(full["circles"]) == 0
    assert [r["cluster"] for r in full["rectangles"]] == [0, 0, 1, 1, 2, 2] and all(r["l_part"] for r in full["rectangles"])
    assert [i["status_name"] for i in full["l_shapes"]] == ["split"] * 3 and full["l_shapes"][0]["grid_width"] == 31
    assert PC.LSHAPE_STATUS == LN.STATUS and len(PC.LSHAPE_INFO) == 8
    with pytest.raises(ValueError):
        PC.shape_summary(shapes, {}, sc["out"])


def test_workspace_size_and_argument_errors_need_no_device():
    from depth_pro import _lib

    lib = _lib.load()
    assert _lib.DP_LSHAPE_MAX_SIDE == LN.MAX_SIDE == 1024 and 2 * _lib.DP_LSHAPE_MAX_SIDE <= 2048
    a, b = lib.dp_lshape_workspace_size(8, 4096), lib.dp_lshape_workspace_size(8192, 1 << 20)
    assert 0 < a < b < 40 * (1 << 20) and lib.dp_lshape_workspace_size(0, 0) > 0
    P = 4096
    ARG, SHAPE = 1000, 1001
    assert lib.dp_shape_rectangles(P, None, 4, P, P, None) == ARG
    assert lib.dp_shape_rectangles(P, P, -1, P, P, None) == SHAPE
    assert lib.dp_shape_rectangles(None, P, 4, P, P, None) == ARG

    def split(points=P, labels=P, n_max=10, rects=P, nr=P, mr=4, mo=8, mc=64, out=P, n_out=P, info=P, ws=P, wsb=1 << 30):
        return lib.dp_lshape_split(points, labels, None, n_max, rects, nr, mr, mo, mc, out, n_out, info, ws, wsb, None)

    for kw in (dict(points=None), dict(labels=None), dict(rects=None), dict(nr=None), dict(out=None), dict(n_out=None),
               dict(info=None), dict(ws=None), dict(wsb=16), dict(ws=P + 4)):
        assert split(**kw) == ARG, kw
    for kw in (dict(n_max=-1), dict(mr=-1), dict(mo=-1), dict(mc=-1)):
        assert split(**kw) == SHAPE, kw


def test_cli_knows_the_flag(monkeypatch, tmp_path):
    import sys

    import generate_depth_maps as G

    with pytest.raises(ValueError):     # implies --fit_shapes: its argument check runs
        G.batch_generate_depth_maps(str(tmp_path), str(tmp_path / "o"), split_l_shapes=True, circularity_threshold=float("nan"))
    seen = {}
    monkeypatch.setattr(G, "batch_generate_depth_maps", lambda *a, **kw: seen.update(kw) or 0)
    monkeypatch.setattr(sys, "argv", ["generate_depth_maps.py", "--input_dir", str(tmp_path), "--output_dir", str(tmp_path),
                                      "--split_l_shapes"])
    try:
        G.main()
    except SystemExit:
        pass
    assert seen.get("split_l_shapes") is True


# ---- GPU ------------------------------------------------------------------------------------------------

def _split(cuda, points, labels, rects, max_cells=1 << 20, max_out=None, count=None, n_rects=None):
    import torch
    from depth_pro import pointcloud as PC

    pts = torch.as_tensor(np.asarray(points, dtype=np.float64).reshape(-1, 3), device=cuda)
    lab = torch.as_tensor(np.asarray(labels, dtype=np.int32).reshape(-1), device=cuda)
    r = torch.as_tensor(np.asarray(rects, dtype=np.float64).reshape(-1, 8), device=cuda)
    nr = torch.tensor(len(r) if n_rects is None else n_rects, dtype=torch.int32, device=cuda)
    out, n_out, info = PC.split_l_shapes(pts, lab, r, nr, count, max_out, max_cells)
    torch.cuda.synchronize()
    n_out = n_out.cpu().numpy()
    return out.cpu().numpy(), (int(n_out[0]), int(n_out[1])), info.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_fixture_scene(name, gold, cuda, record):
    sc = scene(gold, name)
    out, n_out, info = _split(cuda, sc["points"], sc["labels"], sc["rects"], int(sc["max_cells"]))
    print(name, "status", info[:, 0].astype(int).tolist(), "rows", n_out)
    assert np.array_equal(info, sc["info"]), (info, sc["info"])
    assert n_out == (len(sc["out"]), 0)
    record(f"lshape_{name}_err_over_bound", rows_close(out[:n_out[0]], sc["out"], sources(sc["rects"], sc["info"])))
    assert not out[n_out[0]:].any()                    # nothing lands past the rows


@pytest.mark.gpu
def test_rectangle_list_is_the_host_list(gold, cuda):
    import torch
    from depth_pro import pointcloud as PC

    g = np.random.default_rng(5)
    t = np.zeros((9, 16))
    t[:, 0] = [1, 2, 1, 0, 1, 1, 2, 1, 1]
    t[:, 1] = [50, 40, 1200, 3, 1001, 1000, 9, 5000, 2000]
    t[:, 2:4] = g.uniform(-20, 20, (9, 2))
    t[:, 4] = [3, 1, 12.1, 0, 8, 30, 2, 9, 10.5]
    t[:, 5] = [2, 1, 9.1, 0, 14, 30, 2, 30, 9.6]
    t[:, 6] = g.uniform(0, 90, 9)
    t[8] = scene(gold, "halves")["shapes"][0]
    for k, mc in ((9, 9), (9, 16), (4, 9)):
        rects, n = PC.rectangle_list(torch.as_tensor(np.r_[t, np.zeros((mc - 9, 16))], device=cuda),
                                     torch.tensor(k, dtype=torch.int32, device=cuda), mc)
        want = LN.rectangle_list(t[:min(k, mc)])
        host = PC.shape_summary(t[:min(k, mc)])["rectangles"]
        assert int(n) == len(want) == len(host) and rects.shape == (2 * mc, 8)
        got = rects.cpu().numpy()
        src = np.c_[t[want[:, 5].astype(int), 2:7], np.zeros((len(want), 3))]     # each row's cluster rectangle
        rows_close(got[:len(want)], want, src)
        assert not got[len(want):].any()
        assert [(h["cluster"], h["split"]) for h in host] == [(int(q[5]), bool(q[6])) for q in got[:len(want)]]
        rows_close(got[:len(want), :5], np.array([h["center"] + [h["width"], h["height"], h["angle"]] for h in host]), src)
    rects, n = PC.rectangle_list(torch.zeros(0, 16, dtype=torch.float64, device=cuda),
                                 torch.tensor(0, dtype=torch.int32, device=cuda), 0)
    assert int(n) == 0 and rects.shape == (0, 8)


@pytest.mark.gpu
def test_shuffled_points_and_live_count(gold, cuda):
    sc = scene(gold, "room")
    p = np.random.default_rng(8).permutation(len(sc["points"]))
    a = _split(cuda, sc["points"], sc["labels"], sc["rects"])
    b = _split(cuda, sc["points"][p], sc["labels"][p], sc["rects"])
    assert a[1] == b[1] and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    # rows past the live count take no part: the island's rows go last and are cut off
    ring = len(sc["points"]) - 15 * 20              # the fixture lists the wall ring first, then the 15 x 20 island cells
    c = _split(cuda, sc["points"], sc["labels"], sc["rects"], count=ring)
    want = LN.split_l_shapes(sc["points"][:ring], sc["labels"][:ring], sc["rects"])
    assert np.array_equal(c[2], want[2]) and c[1] == want[1] and c[2][0, 1] == ring
    # rectangles past the device count are not read
    two = np.r_[sc["rects"], sc["rects"]]
    d = _split(cuda, sc["points"], sc["labels"], two, n_rects=1)
    assert d[1] == a[1] and np.array_equal(d[2][0], a[2][0]) and not d[2][1].any()


@pytest.mark.gpu
def test_capacity_and_empty_inputs(gold, cuda):
    sc = scene(gold, "slabs")
    full = _split(cuda, sc["points"], sc["labels"], sc["rects"])
    assert full[1] == (6, 0)
    # more rows than max_out: the error word, the first max_out rows, nothing past them
    out, n_out, info = _split(cuda, sc["points"], sc["labels"], sc["rects"], max_out=3)
    assert n_out == (3, 1) and out.shape == (3, 8) and np.array_equal(out, full[0][:3]) and np.array_equal(info, full[2])
    out, n_out, info = _split(cuda, sc["points"], sc["labels"], sc["rects"], max_out=0)
    assert n_out == (0, 1)
    # the grids' capacity: 651 cells each; the second and third do not fit 700, all three fit 1953 exactly
    for cells, want in ((700, [0, 9, 9]), (1953, [0, 0, 0]), (1952, [0, 0, 9]), (0, [9, 9, 9])):
        out, n_out, info = _split(cuda, sc["points"], sc["labels"], sc["rects"], max_cells=cells)
        ref = LN.split_l_shapes(sc["points"], sc["labels"], sc["rects"], max_cells=cells)
        assert info[:, 0].astype(int).tolist() == want and np.array_equal(info, ref[2]) and n_out == ref[1]
        rows_close(out[:n_out[0]], ref[0], sources(sc["rects"], ref[2]))
    # no points, no rectangles
    out, n_out, info = _split(cuda, np.zeros((0, 3)), np.zeros(0), sc["rects"])
    assert n_out == (3, 0) and info[:, 0].tolist() == [2, 2, 2] and np.array_equal(out[:3], sc["rects"])
    out, n_out, info = _split(cuda, sc["points"], sc["labels"], np.zeros((0, 8)))
    assert n_out == (0, 0) and info.shape == (0, 8)
    out, n_out, info = _split(cuda, sc["points"], sc["labels"], sc["rects"], count=0)
    assert info[:, 0].tolist() == [2, 2, 2] and info[:, 1].tolist() == [0, 0, 0]


@pytest.mark.gpu
def test_room_end_to_end(gold, cuda, tmp_path):
    """cluster_shapes -> rectangle_list -> split_l_shapes on `room` lifted to 3-D: the wall ring and the island are
    separate DBSCAN clusters; the ring's rectangle holds the island and is split into the two.  (At the default
    circularity threshold the reference's decision calls the wall ring a circle, circ 0.96; 0.99 keeps it a rectangle.)"""
    import torch
    from depth_pro import pointcloud as PC

    g = np.random.default_rng(13)
    # dense enough for DBSCAN at eps 0.2: walls of an 8 x 6 room and a filled 4 x 3 island, turned by 15 degrees
    t, q = np.arange(0.025, 8.0, 0.05), np.arange(0.025, 6.0, 0.05)
    wall = np.r_[np.c_[t, np.zeros_like(t)], np.c_[t, np.full_like(t, 6.0)],
                 np.c_[np.zeros_like(q), q], np.c_[np.full_like(q, 8.0), q]]
    gx, gy = np.meshgrid(np.arange(2.15, 5.9, 0.1), np.arange(1.65, 4.4, 0.1))
    isl = np.c_[gx.ravel(), gy.ravel()]
    uv = np.r_[wall, isl] + g.uniform(-0.013, 0.013, (len(wall) + len(isl), 2)) - [4.0, 3.0]
    a = math.radians(15.0)
    uv = np.c_[uv[:, 0] * math.cos(a) - uv[:, 1] * math.sin(a), uv[:, 0] * math.sin(a) + uv[:, 1] * math.cos(a)] + [3.0, -2.0]
    pts = np.c_[-uv[:, 0], g.uniform(1.4, 2.0, len(uv)), uv[:, 1]]
    pts = pts[g.permutation(len(pts))]
    P = torch.as_tensor(pts, device=cuda)
    labels, ncl, stats, table, order, offsets, shapes, _, _ = PC.cluster_shapes(P, max_clusters=16, circularity_threshold=0.99)
    rects, n_rects = PC.rectangle_list(shapes, ncl, 16)
    torch.cuda.synchronize()
    assert int(ncl) == 2 and int(n_rects) == 2
    lab, sh = labels.cpu().numpy(), shapes.cpu().numpy()
    want_rects = LN.rectangle_list(sh[:2])
    rows_close(rects.cpu().numpy()[:2], want_rects, want_rects)
    # A cluster's own rectangle has its extreme members exactly on its boundary, where an ulp of sin / cos decides
    # "inside".  The split gets the rectangles a millimetre wider and higher, so every count is exact.
    wide = rects.clone()
    wide[:, 2:4] += 0.001
    out, n_out, info = PC.split_l_shapes(P, labels, wide, n_rects)
    torch.cuda.synchronize()
    wide = wide.cpu().numpy()[:2]
    for r in range(2):
        xr, yr, _, _ = LN.rotated(LN.participants(pts, lab), wide[r])
        assert min(np.abs(np.abs(xr) - wide[r, 2] / 2).min(), np.abs(np.abs(yr) - wide[r, 3] / 2).min()) >= 1e-9
    rows, n_want, winfo = LN.split_l_shapes(pts, lab, wide)
    info = info.cpu().numpy()[:2]
    assert np.array_equal(info, winfo), (info, winfo)
    assert tuple(n_out.cpu().tolist()) == n_want
    rows_close(out.cpu().numpy()[:n_want[0]], rows, sources(wide, winfo))
    ring = int(np.argmax(sh[:2, 7]))                   # the larger rectangle is the wall ring's
    assert info[ring, 0] == 0 and info[ring, 6] == 2 and info[1 - ring, 0] != 0
    assert n_want[0] == 3
    js = PC.shape_summary(sh[:2], {}, out.cpu().numpy()[:3], info)
    assert [r["l_part"] for r in js["rectangles"]].count(True) == 2 and js["l_split"]
    # the text export lists the split list: three rectangles, the two parts in the ring's place
    PC.export_shape_text(js, str(tmp_path / "room.txt"))
    lines = [ln for ln in open(tmp_path / "room.txt").read().splitlines() if ln[:1].isdigit()]
    assert len(lines) == 3
    for ln, w in zip(lines, rows):
        assert ln.split(", ")[1:6] == [f"{w[0]:.3f}", f"{w[1]:.3f}", f"{w[2]:.3f}", f"{w[3]:.3f}", f"{w[4]:.1f}"]


@pytest.mark.gpu
def test_loop_split_l_shapes(tmp_path, cuda):
    """--split_l_shapes writes {base}_shapes.json / .txt with the list after the split; every other file of the
    --fit_shapes run stays byte for byte."""
    import test_shapes as TS
    from depth_pro import pointcloud as PC

    plain, out = tmp_path / "shapes", tmp_path / "lsplit"
    kw = dict(stray_radius=0.25, stray_neighbors=12, cluster_eps=0.12, cluster_min_samples=6,
              cluster_height=float("nan"), cluster_max_points=3000, circularity_threshold=0.8)
    TS._run_loop(tmp_path, cuda, plain, frames=1, fit_shapes=True, **kw)
    TS._run_loop(tmp_path, cuda, out, frames=1, split_l_shapes=True, ground_params_dir=str(plain), **kw)
    assert sorted(os.listdir(out)) == sorted(set(os.listdir(plain)) - {"ground.json"})
    for name in os.listdir(out):
        if "_shapes." in name or name.endswith("_clusters.json"):
            continue
        assert open(plain / name, "rb").read() == open(out / name, "rb").read(), name
    base, js = json.load(open(plain / "output_0000_shapes.json")), json.load(open(out / "output_0000_shapes.json"))
    assert "l_split" not in base and js["l_split"] is True and js["l_overflow"] is False
    assert js["parameters"] == base["parameters"] and len(js["circles"]) == len(base["circles"])
    pts, _ = PC.read_ply(str(out / "output_0000_clean.ply"))
    labels = np.load(out / "output_0000_labels.npy")
    rects = LN.rectangle_list(S.fit_shapes(pts, labels, thr=0.8)[0])
    rows, n_out, info = LN.split_l_shapes(pts, labels, rects)
    assert len(js["l_shapes"]) == len(rects) == len(base["rectangles"]) > 0
    assert [i["status"] for i in js["l_shapes"]] == info[:, 0].astype(int).tolist()
    assert [i["points_inside"] for i in js["l_shapes"]] == info[:, 1].astype(int).tolist()
    assert len(js["rectangles"]) == n_out[0]
    print("loop scene statuses:", info[:, 0].astype(int).tolist())
    # the rows are the restatement's on the WRITTEN cloud, through its own shape fit: test_shapes' bound for that fit
    for g, w in zip(js["rectangles"], rows):
        tol = TS.REL * max(np.hypot(w[2], w[3]), 1.0)
        assert g["cluster"] == int(w[5]) and g["split"] == bool(int(w[6]) & 1) and g["l_part"] == bool(int(w[6]) & 2)
        assert max(abs(g["center"][0] - w[0]), abs(g["center"][1] - w[1])) <= tol
        assert TS.close(g["width"], w[2]) and TS.close(g["height"], w[3]) and abs(g["angle"] - w[4]) <= 180 * TS.REL
    PC.export_shape_text(js, str(tmp_path / "again.txt"))
    assert open(tmp_path / "again.txt").read() == open(out / "output_0000_shapes.txt").read()
