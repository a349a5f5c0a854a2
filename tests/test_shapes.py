"""Cluster shapes (ABI 18, csrc/dp_shapes.hip): convex hull, minimum-area rectangle, circle, decision.

The expected values come from tests/shapes_numpy.py, a numpy restatement of the header's
specification, which the non-GPU tests pin to scipy's ConvexHull and leastsq through
tests/golden/golden_shapes.npz (made by tests/golden/make_golden_shapes.py, which also asserts that
every orientation sign in the fixture is exact and that no decision sits near its threshold).
Hull rows, offsets, kinds and counts are compared exactly; areas and extents within 1e-12 relative
(same operations, only a sum's order may differ); circles within the fixture's circle_tol, the
distance between the restatement and scipy itself.
"""

import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest

import cluster_numpy as CN
import shapes_numpy as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = ["rings", "noisy_ring", "filled", "boxes", "thin", "lattice"]
CHUNK = 2048            # members of one hull chunk = DP_SHAPES_H_MAX
REL = 1e-12


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_shapes.npz"))


@pytest.fixture(scope="module")
def restated(gold):
    out = {}
    for s in SCENES:
        pts = gold[f"{s}_points"]
        eps, ms = gold[f"{s}_params"]
        labels = CN.dbscan(pts, float(eps), int(ms))[0]
        out[s] = (labels,) + S.fit_shapes(pts, labels)
    return out


def close(a, b, rel=REL):
    return abs(a - b) <= rel * abs(b)


# ---- no GPU ---------------------------------------------------------------------------------------------

def test_fixture_scenes_are_the_listed_ones(gold):
    assert list(gold["scenes"]) == SCENES


def test_restatement_reproduces_scipy(gold, restated):
    tol = float(gold["circle_tol"])
    assert 0 < tol < 1e-6
    kinds = []
    for s in SCENES:
        labels, shapes, hrows, hoffs = restated[s]
        qoff = gold[f"{s}_qhull_offsets"]
        assert len(shapes) == len(qoff) - 1 == labels.max() + 1
        for c in range(len(shapes)):
            qv = gold[f"{s}_qhull_rows"][qoff[c]:qoff[c + 1]]
            vol = gold[f"{s}_qhull_volume"][c]
            mine = hrows[hoffs[c]:hoffs[c + 1]]
            if len(qv):                                                          # (b)
                assert np.array_equal(np.sort(mine), qv) and close(shapes[c, 12], vol), (s, c)
            else:
                assert len(mine) == 2 and shapes[c, 12] == 0 and shapes[c, 14] == 0
            xc, yc, r, err = gold[f"{s}_leastsq"][c]                              # (c)
            ref = S.criteria(vol, len(qv), r, err, shapes[c, 7])[1]
            assert ref == S.criteria(shapes[c, 12], shapes[c, 13], shapes[c, 10], shapes[c, 11], shapes[c, 7])[1], (s, c)
            assert shapes[c, 0] == gold[f"{s}_kind"][c] == (2 if all(ref) else 1) == S.decide(shapes[c])
            if shapes[c, 0] == 2:                                                # (d)
                assert max(abs(shapes[c, 8] - xc), abs(shapes[c, 9] - yc), abs(shapes[c, 10] - r)) <= tol
            kinds.append(int(shapes[c, 0]))
            assert 0 <= shapes[c, 6] < 90
            r_ = np.flatnonzero(labels == c)
            uv = np.c_[-gold[f"{s}_points"][r_, 0], gold[f"{s}_points"][r_, 2]]
            assert S.inside_rect(uv, shapes[c]) <= REL * np.hypot(shapes[c, 4], shapes[c, 5])
    assert kinds.count(2) == 4 and kinds.count(1) == len(kinds) - 4              # the thin rings, nothing else
    assert restated["lattice"][1][0, 13] == 4 and restated["lattice"][1][0, 7] == 4.75 ** 2
    # the boxes come back at their angles (0 / 90 fold onto each other); 1.2 x 0.5 up to the sampling
    for row in restated["boxes"][1]:
        if abs(row[4] * row[5] - 0.6) < 0.05:
            assert min(abs(row[6] - a) for a in (0, 30, 45, 60, 90)) < 3.0


def test_restatement_rules_on_small_cases():
    sq = np.array([[0, 0], [1, 0], [1, 1], [0, 1], [0.5, 0.5], [0.5, 0], [1, 1], [0, 0]], dtype=np.float64)
    assert list(S.hull(sq)) == [0, 1, 2, 3]                     # ccw from the smallest, collinear and later duplicates out
    assert S.hull_area(sq[S.hull(sq)]) == 1.0
    assert S.min_area_rect(sq[:4]) == (0.5, 0.5, 1.0, 1.0, 0.0, 1.0)
    same = np.tile([[3.0, -2.0]], (5, 1))
    row, hi = S.fit_cluster(same)
    assert list(hi) == [0] and list(row[:8]) == [1, 5, 3, -2, 0, 0, 0, 0] and row[13] == 1 and row[14] == 0
    assert S.fit_cluster(same[:4])[0][0] == 0
    tall = np.array([[0, 0], [1, 0], [1, 3], [0, 3], [0.5, 1]], dtype=np.float64)
    cu, cv, w, h, ang, area = S.min_area_rect(tall[S.hull(tall)])
    assert (cu, cv, w, h, ang, area) == (0.5, 1.5, 1.0, 3.0, 0.0, 3.0)
    t = np.linspace(0, 2 * np.pi, 40, endpoint=False)
    x, y, r, err, _ = S.fit_circle(np.c_[2 + 0.5 * np.cos(t), -1 + 0.5 * np.sin(t)])
    assert max(abs(x - 2), abs(y + 1), abs(r - 0.5)) < 1e-14 and err < 1e-28


def test_shape_summary_and_text_export(tmp_path):
    from depth_pro import pointcloud as PC

    assert PC.SHAPE_COLUMNS == S.COLUMNS and len(PC.SHAPE_COLUMNS) == 16
    t = np.zeros((5, 16))
    t[0] = [1, 40, 1.0, 2.0, 3.0, 0.5, 30.0, 1.5, 0, 0, 1, 0.2, 1.2, 7, 0.4, 0]
    t[1] = [2, 300, 0, 0, 1.1, 1.0, 0, 1.1, -8.832, 27.918, 0.193, 4e-4, 0.11, 30, 0.95, 0]
    t[2] = [0, 3] + [0] * 14
    t[3] = [1, 1001, 10.0, 20.0, 20.0, 6.0, 0.0, 120.0, 0, 0, 9, 0.3, 100, 9, 0.4, 0]      # split along the width
    t[4] = [0, 5000] + [0] * 13 + [1]
    s = PC.shape_summary(t, {"circularity_threshold": 0.85})
    json.dumps(s)
    assert s["parameters"] == {"circularity_threshold": 0.85} and s["clusters_listed"] == 5
    assert s["skipped"] == 2 and s["errors"] == 1
    assert [(r["cluster"], r["split"]) for r in s["rectangles"]] == [(0, False), (3, True), (3, True)]
    assert s["rectangles"][0]["center"] == [1.0, 2.0] and s["rectangles"][0]["angle"] == 30.0
    a, b = s["rectangles"][1:]
    assert (a["center"], a["width"], a["height"]) == ([5.0, 20.0], 10.0, 6.0) and b["center"] == [15.0, 20.0]
    assert s["circles"] == [{"cluster": 1, "count": 300, "center": [-8.832, 27.918], "radius": 0.193, "fit_error": 4e-4,
                             "circularity": 0.95}]
    tall = PC.split_large_rectangle(0.0, 0.0, 2.0, 8.0, 90.0)
    assert np.allclose(tall, [(-2.0, 0.0, 2.0, 4.0, 90.0), (2.0, 0.0, 2.0, 4.0, 90.0)], atol=1e-15)
    # a rectangle that large with 1000 members, or smaller with more, is left whole
    t[3, 1] = 1000
    assert [r["split"] for r in PC.shape_summary(t)["rectangles"]] == [False, False]
    PC.export_shape_text(s, str(tmp_path / "s.txt"))
    assert open(tmp_path / "s.txt").read() == (
        "# Floor Plan Shape Data\n# Units: meters\n\nTotal Shapes: 4\nRectangles: 3\nCircles: 1\n\n"
        "Total Area: 121.62 square meters\n\n# Rectangles\n"
        "# Format: ID, center_x, center_y, width, height, angle_degrees, area_m2\n"
        "1, 1.000, 2.000, 3.000, 0.500, 30.0, 1.500\n2, 5.000, 20.000, 10.000, 6.000, 0.0, 60.000\n"
        "3, 15.000, 20.000, 10.000, 6.000, 0.0, 60.000\n\n# Circles\n# Format: ID, center_x, center_y, radius, area_m2\n"
        "4, -8.832, 27.918, 0.193, 0.117\n")


def test_text_export_has_the_recorded_layout(tmp_path):
    """Against a recorded output of the reference's export_shape_data: the same lines, the same fields."""
    from depth_pro import pointcloud as PC

    want = open(os.path.join(GOLDEN, "shapes_layout_reference.txt")).read().split("\n")
    rects, circles = [], []
    for line in want:
        f = line.split(", ")
        if len(f) == 7 and not line.startswith("#"):
            rects.append({"center": [float(f[1]), float(f[2])], "width": float(f[3]), "height": float(f[4]), "angle": float(f[5])})
        elif len(f) == 5 and not line.startswith("#"):
            circles.append({"center": [float(f[1]), float(f[2])], "radius": float(f[3])})
    assert len(rects) == 22 and len(circles) == 1
    PC.export_shape_text({"rectangles": rects, "circles": circles}, str(tmp_path / "s.txt"))
    got = open(tmp_path / "s.txt").read().split("\n")
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if w.startswith("Total Area") or len(w.split(", ")) in (5, 7) and not w.startswith("#"):
            # areas are printed from the unrounded sizes there, from the 3-decimal ones here: same fields, same format
            assert g.split(", ")[:-1] == w.split(", ")[:-1] and re.sub(r"\d", "0", g)[-5:] == re.sub(r"\d", "0", w)[-5:]
            assert abs(float(re.findall(r"[\d.]+", g)[-1]) - float(re.findall(r"[\d.]+", w)[-1])) < 0.1
        else:
            assert g == w


def test_workspace_size_and_argument_errors_need_no_device():
    from depth_pro import _lib

    lib = _lib.load()
    sizes = [lib.dp_shapes_workspace_size(n, 4096) for n in (0, 1, 2048, 2049, 100003, 8294400)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert sizes[-1] >= 28 * 8294400 and lib.dp_shapes_workspace_size(-5, -1) == lib.dp_shapes_workspace_size(0, 0)
    assert lib.dp_shapes_workspace_size(1000, 10) < lib.dp_shapes_workspace_size(1000, 4096)
    P, big, ARG, SHAPE = 4096, 1 << 40, 1000, 1001

    def sh(points=P, n=8, order=P, offsets=P, ncl=P, mc=4, thr=0.85, shapes=P, hrows=P, hoffs=P, ws=P, wsb=big):
        return lib.dp_cluster_shapes(points, None, n, order, offsets, ncl, mc, ctypes.c_double(thr), shapes, hrows, hoffs,
                                     ws, wsb, None)

    assert sh(n=-1) == SHAPE and sh(mc=-1) == SHAPE and sh(thr=float("nan")) == SHAPE
    for kw in ({"points": None}, {"order": None}, {"offsets": None}, {"ncl": None}, {"shapes": None}, {"hrows": None},
               {"hoffs": None}, {"ws": None}, {"wsb": 16}, {"ws": P + 4}, {"wsb": lib.dp_shapes_workspace_size(8, 4) - 1}):
        assert sh(**kw) == ARG, kw


def test_python_layer_refuses_bad_arguments_and_host_tensors():
    import torch

    from depth_pro import _lib
    from depth_pro import pointcloud as PC

    pts = torch.zeros(4, 3, dtype=torch.float64)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)      # noqa: E731
    with pytest.raises(_lib.DPError):
        PC.fit_shapes(pts, i32(4), i32(4097), i32(()))
    with pytest.raises(_lib.DPError):
        PC.cluster_shapes(pts)
    with pytest.raises(ValueError):
        PC.fit_shapes(pts, i32(4), i32(4097), i32(()), max_clusters=-1)
    with pytest.raises(ValueError):
        PC.fit_shapes(pts, i32(4), i32(4097), i32(()), circularity_threshold=float("nan"))
    with pytest.raises(ValueError):
        PC.cluster_shapes(pts, eps=0.0)


def test_cli_and_resume_know_the_shapes_files(monkeypatch, tmp_path):
    import generate_depth_maps as G

    monkeypatch.setattr(sys, "argv", ["generate_depth_maps.py", "--input_dir", str(tmp_path), "--fit_shapes",
                                      "--circularity_threshold", "nan"])
    with pytest.raises(SystemExit) as e:
        G.main()
    assert e.value.code == 2
    with pytest.raises(ValueError):
        G.batch_generate_depth_maps(str(tmp_path), str(tmp_path / "o"), fit_shapes=True, circularity_threshold=float("nan"))
    frames = [str(tmp_path / f"f{k}.png") for k in range(3)]
    assert G.shapes_name(frames[0]) == "f0_shapes.json"
    for k in (0, 1):
        for s in ("depth.png", "clean.ply", "clusters.json"):
            (tmp_path / f"f{k}_{s}").write_bytes(b"")
    (tmp_path / "f0_shapes.json").write_bytes(b"")
    assert G.plan_frames(frames, str(tmp_path), 1, 0, True, cleaned=True, clustered=True) == [2]
    assert G.plan_frames(frames, str(tmp_path), 1, 0, True, cleaned=True, clustered=True, shaped=True) == [1, 2]
    assert G.plan_frames(frames, str(tmp_path), 1, 0, False, shaped=True) == [0, 1, 2]


# ---- GPU ------------------------------------------------------------------------------------------------

def _fit(pts, cuda, labels=None, eps=0.2, ms=5, count=None, max_clusters=4096, thr=0.85):
    """dbscan_labels (or hand-made labels) -> cluster_table -> fit_shapes; everything back on the host."""
    import torch

    from depth_pro import pointcloud as PC

    t = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)).to(cuda)
    if labels is None:
        lab, ncl, _ = PC.dbscan_labels(t, count, eps, ms)
    else:
        lab = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(cuda)
        ncl = torch.tensor(int(max(labels.max(), -1)) + 1 if len(labels) else 0, dtype=torch.int32, device=cuda)
    _, order, offsets = PC.cluster_table(t, lab, ncl, count, max_clusters)
    shapes, hrows, hoffs = PC.fit_shapes(t, order, offsets, ncl, count, max_clusters, thr)
    k = min(int(ncl.item()), max_clusters)
    hoffs = hoffs.cpu().numpy()
    return lab.cpu().numpy(), shapes.cpu().numpy()[:k], hrows.cpu().numpy()[:hoffs[k]], hoffs[:k + 1]


def _compare(got, want, pts, labels, tol=None):
    """Device rows against the restatement's: the exact columns, the 1e-12 columns, the geometry, the decision."""
    shapes, hrows, hoffs = got
    wshapes, wrows, woffs = want
    print(f"clusters={len(wshapes)} kinds={[int(v) for v in shapes[:, 0]]} hull vertices={[int(v) for v in shapes[:, 13]]}")
    assert np.array_equal(hoffs, woffs) and np.array_equal(hrows, wrows)
    assert np.array_equal(shapes[:, [0, 1, 13, 15]], wshapes[:, [0, 1, 13, 15]])
    for c, (g, w) in enumerate(zip(shapes, wshapes)):
        rel = [abs(g[j] - w[j]) / abs(w[j]) if w[j] else abs(g[j]) for j in (12, 7, 4, 5)]
        print(f"  [{c}] n={int(g[1])} rel err hull_area/area/width/height={rel} circle d="
              f"{max(abs(g[8:11] - w[8:11])) if g[0] == 2 else None}")
        assert S.decide(g) == g[0]
        if g[0] == 0:
            assert (g[2:15] == 0).all()
            continue
        for j in (12, 7, 4, 5):
            assert close(g[j], w[j]), (c, j, g[j], w[j])
        assert 0 <= g[6] < 90
        assert g[7] <= w[7] * (1 + REL)
        r = np.flatnonzero(labels == c)
        assert S.inside_rect(np.c_[-pts[r, 0], pts[r, 2]], g) <= REL * np.hypot(g[4], g[5])
        if g[0] == 2 and tol is not None:
            assert max(abs(g[8:11] - w[8:11])) <= tol, (c, g[8:11], w[8:11])


@pytest.mark.gpu
@pytest.mark.parametrize("scene", SCENES)
def test_fixture_scene(scene, gold, restated, cuda):
    pts = gold[f"{scene}_points"]
    eps, ms = gold[f"{scene}_params"]
    labels, shapes, hrows, hoffs = _fit(pts, cuda, eps=float(eps), ms=int(ms))
    want = restated[scene]
    assert np.array_equal(labels, want[0])
    _compare((shapes, hrows, hoffs), want[1:], pts, labels, float(gold["circle_tol"]))
    assert np.array_equal(shapes[:, 0], gold[f"{scene}_kind"])                   # the reference's decision


def _disc_lattice(g, size, centre):
    """`size` lattice points k / 1024 inside a disc of radius 48 / 1024 around centre / 1024 (integers)."""
    i, j = np.meshgrid(np.arange(-48, 49), np.arange(-48, 49), indexing="ij")
    inside = np.flatnonzero(i.ravel() ** 2 + j.ravel() ** 2 <= 48 * 48)
    assert len(inside) >= size
    pick = g.permutation(inside)[:size]
    return np.c_[i.ravel()[pick] + centre[0], j.ravel()[pick] + centre[1]] / 1024.0


@pytest.mark.gpu
def test_clusters_around_the_chunk_size(cuda):
    """One below, at and one above the chunk, and three chunks plus one: several rounds, exact predicate
    (products of 21-bit integers), collinear lattice triples across the chunk seams."""
    g = np.random.default_rng(11)
    sizes = [CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 1]
    uv = np.concatenate([_disc_lattice(g, s, (200 * k, 1000)) for k, s in enumerate(sizes)])
    labels = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    perm = g.permutation(len(uv))
    uv, labels = uv[perm], labels[perm]
    pts = np.c_[-uv[:, 0], np.full(len(uv), 2.0), uv[:, 1]]
    _, shapes, hrows, hoffs = _fit(pts, cuda, labels=labels)
    want = S.fit_shapes(pts, labels)
    assert list(want[0][:, 1]) == sizes and (want[0][:, 0] == 1).all() and (want[0][:, 13] < 100).all()
    _compare((shapes, hrows, hoffs), want, pts, labels)


@pytest.mark.gpu
def test_more_hull_vertices_than_h_max(cuda):
    """(k, k^2): every point a vertex.  The cluster is flagged; its neighbours in the call are not touched."""
    g = np.random.default_rng(12)
    k = np.arange(CHUNK + 9, dtype=np.float64)
    blob = lambda c: np.c_[g.uniform(0, 1, 50) + c, g.uniform(0, 1, 50)]         # noqa: E731
    uv = np.concatenate([blob(-10.0), np.c_[k, k * k], blob(-20.0)])
    labels = np.repeat([0, 1, 2], [50, len(k), 50]).astype(np.int32)
    perm = g.permutation(len(uv))
    uv, labels = uv[perm], labels[perm]
    pts = np.c_[-uv[:, 0], np.full(len(uv), 2.0), uv[:, 1]]
    _, shapes, hrows, hoffs = _fit(pts, cuda, labels=labels)
    want = S.fit_shapes(pts, labels)
    assert want[0][1, 15] == 1 and want[0][1, 0] == 0 and want[1].size == want[2][-1] and want[2][1] == want[2][2]
    assert list(shapes[1]) == [0, CHUNK + 9] + [0] * 13 + [1] and hoffs[1] == hoffs[2]
    _compare((shapes, hrows, hoffs), want, pts, labels)
    # at the cap itself the hull is kept
    uv = np.c_[k[:CHUNK], k[:CHUNK] ** 2]
    pts = np.c_[-uv[:, 0], np.full(CHUNK, 2.0), uv[:, 1]]
    _, shapes, hrows, hoffs = _fit(pts, cuda, labels=np.zeros(CHUNK, np.int32))
    assert shapes[0, 15] == 0 and shapes[0, 13] == CHUNK and np.array_equal(hrows, np.arange(CHUNK)) and shapes[0, 0] == 1


@pytest.mark.gpu
def test_empty_inputs_and_small_clusters(cuda):
    for pts, count in ((np.zeros((0, 3)), None), (np.ones((100, 3)), 0)):
        _, shapes, hrows, hoffs = _fit(pts, cuda, count=count)
        assert shapes.shape == (0, 16) and hrows.size == 0 and list(hoffs) == [0]
    # far apart, so no clusters at min_samples = 5
    far = np.c_[np.arange(20.0), np.full(20, 2.0), np.zeros(20)]
    _, shapes, hrows, hoffs = _fit(far, cuda)
    assert shapes.shape == (0, 16) and list(hoffs) == [0]
    # clusters of 1 to 4 members (min_samples = 1) beside one of 5 coincident points
    groups = [np.tile([[3.0 * m, 2.0, 1.0]], (m, 1)) + np.c_[0.01 * np.arange(m), np.zeros(m), np.zeros(m)] for m in (1, 2, 3, 4)]
    pts = np.concatenate(groups + [np.tile([[-7.0, 2.0, 5.0]], (5, 1))])
    labels, shapes, hrows, hoffs = _fit(pts, cuda, ms=1)
    assert [int(v) for v in shapes[:, 1]] == [1, 2, 3, 4, 5] and list(shapes[:, 0]) == [0, 0, 0, 0, 1]
    assert (shapes[:4, 2:] == 0).all() and list(hoffs) == [0, 0, 0, 0, 0, 1] and list(hrows) == [10]
    assert list(shapes[4, 2:8]) == [7.0, 5.0, 0, 0, 0, 0] and shapes[4, 13] == 1 and shapes[4, 14] == 0 and shapes[4, 15] == 0
    want = S.fit_shapes(pts, labels)
    assert np.array_equal(want[0][:, :8], shapes[:, :8]) and np.array_equal(want[1], hrows)


@pytest.mark.gpu
def test_nothing_lands_past_max_clusters_or_count(gold, restated, cuda):
    """More clusters than max_clusters, through the C entry with a guard region behind every output."""
    import torch

    from depth_pro import _lib
    from depth_pro import pointcloud as PC

    pts = gold["boxes_points"]
    labels, wshapes, wrows, woffs = restated["boxes"]
    lib = _lib.load()
    n, mc, G = len(pts), 3, 64
    assert len(wshapes) > mc
    t = torch.from_numpy(np.ascontiguousarray(pts)).to(cuda)
    lab, ncl, _ = PC.dbscan_labels(t, None, 0.2, 5)
    _, order, offsets = PC.cluster_table(t, lab, ncl, None, mc)
    shapes = torch.full((mc * 16 + G,), 7.0, dtype=torch.float64, device=cuda)
    hrows = torch.full((n + G,), -7, dtype=torch.int32, device=cuda)
    hoffs = torch.full((mc + 1 + G,), -7, dtype=torch.int32, device=cuda)
    ws = torch.empty(int(lib.dp_shapes_workspace_size(n, mc)), dtype=torch.uint8, device=cuda)
    assert lib.dp_cluster_shapes(t.data_ptr(), None, n, order.data_ptr(), offsets.data_ptr(), ncl.data_ptr(), mc, 0.85,
                                 shapes.data_ptr(), hrows.data_ptr(), hoffs.data_ptr(), ws.data_ptr(), ws.numel(),
                                 torch.cuda.current_stream(cuda).cuda_stream) == 0
    shapes, hrows, hoffs = shapes.cpu().numpy(), hrows.cpu().numpy(), hoffs.cpu().numpy()
    assert (shapes[mc * 16:] == 7.0).all() and (hoffs[mc + 1:] == -7).all()
    assert np.array_equal(hoffs[:mc + 1], woffs[:mc + 1]) and np.array_equal(hrows[:woffs[mc]], wrows[:woffs[mc]])
    assert (hrows[woffs[mc]:] == -7).all()
    got = shapes[:mc * 16].reshape(mc, 16)
    assert np.array_equal(got[:, [0, 1, 13]], wshapes[:mc][:, [0, 1, 13]]) and all(close(a, b) for a, b in zip(got[:, 7], wshapes[:mc, 7]))
    # a count smaller than the tensor: the rows past it are nobody's
    m = 900
    want = S.fit_shapes(pts[:m], CN.dbscan(pts[:m], 0.2, 5)[0])
    lab2, s2, r2, o2 = _fit(pts, cuda, count=m)
    _compare((s2, r2, o2), want, pts[:m], lab2[:m])


@pytest.mark.gpu
def test_two_streams_give_identical_results(gold, cuda):
    import torch

    pts = np.concatenate([gold["rings_points"], gold["boxes_points"] + [0.0, 0.0, 40.0]])
    outs = []
    streams = [torch.cuda.Stream(cuda), torch.cuda.Stream(cuda)]
    for st in streams:
        with torch.cuda.stream(st):
            outs.append(_fit(pts, cuda))
    torch.cuda.synchronize()
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
    assert len(outs[0][1]) == 11


# ---- the frame loop ---------------------------------------------------------------------------------------

class _FixtureModel:
    """Stands in for the engine in the loop test: returns a fixed depth map and focal length."""

    def __init__(self, depth, f, dev):
        import torch

        self.depth = torch.from_numpy(np.ascontiguousarray(depth)).to(dev)
        self.f = torch.tensor(float(f), dtype=torch.float32, device=dev)

    def infer(self, x, f_px=None):
        return {"depth": self.depth.clone(), "focallength_px": self.f}


def _run_loop(tmp_path, cuda, out, frames=2, **kw):
    import torch
    from PIL import Image

    import generate_depth_maps as G

    gg = np.load(os.path.join(GOLDEN, "golden_ground.npz"))
    src = tmp_path / "frames"
    if not src.exists():
        src.mkdir()
        rgb = np.random.default_rng(3).integers(0, 256, (96, 128, 3), dtype=np.uint8)
        for k in range(frames):
            Image.fromarray(rgb).save(src / f"output_{k:04d}.png")
    model = (_FixtureModel(gg["flat_depth"], gg["flat_f"], cuda), lambda im: torch.as_tensor(np.asarray(im)))
    assert G.batch_generate_depth_maps(str(src), str(out), pattern="output_*.png", model=model, **kw) == frames


@pytest.mark.gpu
def test_loop_fit_shapes(tmp_path, gold, cuda):
    """--fit_shapes adds {base}_shapes.json and {base}_shapes.txt to the cluster run's files, which stay
    byte for byte (the centroids of {base}_clusters.json within the cluster table's own bound); the JSON
    is shape_summary of the restatement on the written cloud and labels."""
    import generate_depth_maps as G
    from depth_pro import pointcloud as PC

    plain, out = tmp_path / "cluster", tmp_path / "shapes"
    kw = dict(cluster_pointcloud=True, stray_radius=0.25, stray_neighbors=12, cluster_eps=0.12, cluster_min_samples=6,
              cluster_height=float("nan"), cluster_max_points=3000)
    _run_loop(tmp_path, cuda, plain, **kw)
    _run_loop(tmp_path, cuda, out, fit_shapes=True, circularity_threshold=0.8, ground_params_dir=str(plain), **kw)
    names = sorted(set(os.listdir(plain)) - {"ground.json"})
    assert len(names) == 8
    assert sorted(os.listdir(out)) == sorted(names + [f"output_{k:04d}_shapes.{e}" for k in range(2) for e in ("json", "txt")])
    for name in names:
        if name.endswith("_clusters.json"):
            # not byte for byte even between two cluster runs: the table's sums (the centroids) are accumulated in
            # an unspecified order, each within (count - 1) * 2^-53 * sum |v| of the exact one (the ABI 17 contract)
            a, b = json.load(open(plain / name)), json.load(open(out / name))
            for ca, cb in zip(a["cluster_table"], b["cluster_table"]):
                for axis, (va, vb) in zip("xyz", zip(ca.pop("centroid"), cb.pop("centroid"))):
                    assert abs(va - vb) <= 2 * ca["count"] * 2.0 ** -53 * max(abs(v) for v in ca["bbox"][axis]) + 1e-15
            assert a == b
            continue
        assert open(plain / name, "rb").read() == open(out / name, "rb").read(), name
    for k in range(2):
        pts, _ = PC.read_ply(str(out / f"output_{k:04d}_clean.ply"))
        labels = np.load(out / f"output_{k:04d}_labels.npy")
        wshapes = S.fit_shapes(pts, labels, thr=0.8)[0]
        want = PC.shape_summary(wshapes, {})
        js = json.load(open(out / f"output_{k:04d}_shapes.json"))
        assert js["parameters"] == {"eps": 0.12, "min_samples": 6, "height_threshold": None, "max_points": 3000,
                                    "circularity_threshold": 0.8}
        assert len(wshapes) > 0 and js["clusters_listed"] == len(wshapes) and js["errors"] == 0
        assert js["skipped"] == want["skipped"] and len(js["rectangles"]) > 0
        for key in ("rectangles", "circles"):
            assert [(s["cluster"], s["count"]) for s in js[key]] == [(s["cluster"], s["count"]) for s in want[key]]
        for g, w in zip(js["rectangles"], want["rectangles"]):
            diag = np.hypot(w["width"], w["height"])
            assert close(g["width"], w["width"]) and close(g["height"], w["height"]) and close(g["hull_area"], w["hull_area"])
            assert max(abs(g["center"][0] - w["center"][0]), abs(g["center"][1] - w["center"][1])) <= REL * max(diag, 1.0)
            assert abs(g["angle"] - w["angle"]) <= 90 * REL and g["hull_vertices"] == w["hull_vertices"]
        for g, w in zip(js["circles"], want["circles"]):
            assert max(abs(g["center"][0] - w["center"][0]), abs(g["center"][1] - w["center"][1]),
                       abs(g["radius"] - w["radius"])) <= float(gold["circle_tol"])
        PC.export_shape_text(js, str(tmp_path / "again.txt"))
        assert open(tmp_path / "again.txt").read() == open(out / f"output_{k:04d}_shapes.txt").read()
    src = sorted(str(p) for p in (tmp_path / "frames").glob("*.png"))
    assert G.plan_frames(src, str(out), 1, 0, True, cleaned=True, clustered=True, shaped=True) == []
    assert G.plan_frames(src, str(plain), 1, 0, True, cleaned=True, clustered=True, shaped=True) == [0, 1]
