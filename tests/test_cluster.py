"""Clustered point clouds (ABI 17, csrc/dp_cluster.hip): exact DBSCAN labels and the cluster table.

The expected values come from tests/cluster_numpy.py, a numpy restatement of the header's
specification, which the non-GPU test below pins to sklearn's DBSCAN through
tests/golden/golden_cluster.npz (made by tests/golden/make_golden_cluster.py).  Labels, counts,
bounds, order and offsets are compared exactly; the table's sums against math.fsum within
(count - 1) * 2^-53 * sum |v|, the bound for any order of summation.
"""

import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest

import cluster_numpy as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = ["blobs0", "blobs1", "blobs2", "blobs3", "blobs4", "lattice", "levelled", "bridge", "border"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_cluster.npz"))


def _scene(gold, name):
    eps, ms, thr = gold[f"{name}_params"]
    return gold[f"{name}_points"], float(eps), int(ms), float(thr)


@pytest.fixture(scope="module")
def restated(gold):
    return {s: N.dbscan(*_scene(gold, s)) for s in SCENES}


# ---- no GPU ---------------------------------------------------------------------------------------------

def test_fixture_scenes_are_the_listed_ones(gold):
    assert list(gold["scenes"]) == SCENES


def test_restatement_reproduces_sklearn(gold, restated):
    for s in SCENES:
        pts, eps, ms, thr = _scene(gold, s)
        rows = N.participants(pts, thr)
        assert len(rows) >= 64
        labels, core_rows, stats = restated[s]
        assert np.array_equal(labels[rows], gold[f"{s}_labels"]), s
        assert np.array_equal(core_rows, rows[gold[f"{s}_core"]]), s
        assert (np.delete(labels, rows) == -2).all()
        assert stats[2] == len(rows) and stats[3] == len(core_rows) and stats[6] == labels.max() + 1
        assert stats[3] + stats[4] + stats[5] == stats[2] and stats[5] == (labels == -1).sum()
    # the scenes that pin rules 3 and 4
    assert restated["bridge"][2][6] == 1 and restated["border"][2][6] == 2
    lab, core_rows, _ = restated["border"]
    assert lab[0] == 0 and 0 not in core_rows                     # the shared border point, in front of every core row
    assert restated["lattice"][2][4] > 0 and restated["blobs0"][2][4] > 0


def test_fixture_has_no_pair_on_the_rounding_edge(gold):
    for s in SCENES:
        pts, eps, ms, thr = _scene(gold, s)
        xz = pts[N.participants(pts, thr)][:, [0, 2]]
        e2 = eps * eps
        exact = 0
        for a in range(0, len(xz), 512):
            d = xz[a:a + 512, None, :] - xz[None, :, :]
            d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
            assert not ((np.abs(d2 - e2) <= 1e-12 * e2) & (d2 != e2)).any(), s
            exact += int((d2 == e2).sum())
        assert (exact > 0) == (s == "lattice")


def test_sampling_rule_takes_exactly_max_points():
    pts = np.zeros((1000, 3))
    pts[::7, 1] = np.nan
    e = len(N.participants(pts))
    for m in (1, 2, 99, e - 1):
        rows = N.participants(pts, None, m)
        assert len(rows) == m and rows[0] == N.participants(pts)[0]
    assert len(N.participants(pts, None, e)) == e and len(N.participants(pts, None, e + 1)) == e


def test_workspace_size_and_argument_errors_need_no_device():
    from depth_pro import _lib

    lib = _lib.load()
    sizes = [lib.dp_cluster_workspace_size(n) for n in (0, 1, 2048, 2049, 4096, 4097, 100003, 8294400)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert sizes[-1] >= lib.dp_clean_workspace_size(8294400) + 40 * 8294400
    assert lib.dp_cluster_workspace_size(-5) == sizes[0]
    P, big, ARG, SHAPE = 4096, 1 << 40, 1000, 1001
    f64 = ctypes.c_double
    nan = float("nan")

    def db(points=P, n=8, eps=0.2, ms=5, thr=nan, mp=0, labels=P, ncl=P, stats=P, ws=P, wsb=big):
        return lib.dp_cluster_dbscan(points, None, n, f64(eps), ms, f64(thr), mp, labels, ncl, stats, ws, wsb, None)

    for eps in (0.0, -1.0, nan, float("inf")):
        assert db(eps=eps) == SHAPE
    assert db(ms=0) == SHAPE and db(ms=-2) == SHAPE and db(mp=-1) == SHAPE and db(n=-1) == SHAPE
    assert db(points=None) == ARG and db(labels=None) == ARG and db(ncl=None) == ARG and db(stats=None) == ARG
    assert db(ws=None) == ARG and db(wsb=16) == ARG and db(ws=P + 4) == ARG
    assert db(wsb=lib.dp_cluster_workspace_size(8) - 1) == ARG

    def tb(points=P, labels=P, n=8, ncl=P, mc=4, table=P, order=P, offsets=P, ws=P, wsb=big):
        return lib.dp_cluster_table(points, labels, None, n, ncl, mc, table, order, offsets, ws, wsb, None)

    assert tb(n=-1) == SHAPE and tb(mc=-1) == SHAPE
    for kw in ({"points": None}, {"labels": None}, {"ncl": None}, {"table": None}, {"order": None}, {"offsets": None},
               {"ws": None}, {"wsb": 16}):
        assert tb(**kw) == ARG, kw


def test_python_layer_refuses_bad_arguments_and_host_tensors():
    import torch

    from depth_pro import _lib
    from depth_pro import pointcloud as PC

    pts = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(_lib.DPError):
        PC.dbscan_labels(pts)
    with pytest.raises(_lib.DPError):
        PC.cluster_pointcloud(pts)
    with pytest.raises(_lib.DPError):
        PC.cluster_table(pts, torch.zeros(4, dtype=torch.int32), torch.zeros((), dtype=torch.int32))
    for kw in ({"eps": 0.0}, {"eps": -1.0}, {"eps": float("nan")}, {"eps": float("inf")}, {"min_samples": 0},
               {"max_points": -1}):
        with pytest.raises(ValueError):
            PC.dbscan_labels(pts, **kw)
        with pytest.raises(ValueError):
            PC.cluster_pointcloud(pts, **kw)
    with pytest.raises(ValueError):
        PC.cluster_table(pts, torch.zeros(4, dtype=torch.int32), torch.zeros((), dtype=torch.int32), max_clusters=-1)


def test_cluster_summary_is_host_only():
    from depth_pro import pointcloud as PC

    t = np.zeros((2, 12))
    t[0] = [4, 7, -1, 1, 2, 3, 0.5, 1.5, 2.0, 4.0, 10.0, 0]
    t[1] = [1, 9, 0, 0, 0, 0, 0, 0, 3.0, 2.0, 1.0, 0]
    s = PC.cluster_summary(t, [20, 1, 15, 4, 1, 10, 2, 0], {"eps": 0.2})
    assert s["parameters"] == {"eps": 0.2} and s["participants"] == 15 and s["core"] == 4 and s["border"] == 1
    assert s["noise"] == 10 and s["clusters"] == 2 and s["error"] == 0
    c = s["cluster_table"][0]
    assert c == {"id": 0, "count": 4, "min_core_row": 7, "bbox": {"x": [-1.0, 1.0], "z": [2.0, 3.0], "y": [0.5, 1.5]},
                 "centroid": [0.5, 1.0, 2.5]}
    json.dumps(s)


@pytest.mark.parametrize("flag,value", [("--cluster_eps", "0"), ("--cluster_eps", "-1"), ("--cluster_eps", "nan"),
                                        ("--cluster_min_samples", "0"), ("--cluster_max_points", "-1")])
def test_cli_refuses_cluster_values(monkeypatch, flag, value, tmp_path):
    import generate_depth_maps as G

    monkeypatch.setattr(sys, "argv", ["generate_depth_maps.py", "--input_dir", str(tmp_path), "--cluster_pointcloud",
                                      flag, value])
    with pytest.raises(SystemExit) as e:
        G.main()
    assert e.value.code == 2
    key = flag[2:]
    kw = {key: float(value) if key == "cluster_eps" else int(value)}
    with pytest.raises(ValueError):
        G.batch_generate_depth_maps(str(tmp_path), str(tmp_path / "o"), cluster_pointcloud=True, **kw)


def test_resume_looks_for_the_clusters_file(tmp_path):
    import generate_depth_maps as G

    frames = [str(tmp_path / f"f{k}.png") for k in range(3)]
    assert G.clusters_name(frames[0]) == "f0_clusters.json" and G.labels_name(frames[0]) == "f0_labels.npy"
    for k in (0, 1):
        (tmp_path / f"f{k}_depth.png").write_bytes(b"")
        (tmp_path / f"f{k}_clean.ply").write_bytes(b"")
    (tmp_path / "f0_clusters.json").write_bytes(b"")
    assert G.plan_frames(frames, str(tmp_path), 1, 0, True, cleaned=True) == [2]
    assert G.plan_frames(frames, str(tmp_path), 1, 0, True, cleaned=True, clustered=True) == [1, 2]


# ---- GPU ------------------------------------------------------------------------------------------------

def _run(pts, cuda, eps=0.2, ms=5, thr=None, mp=0, count=None):
    import torch

    from depth_pro import pointcloud as PC

    t = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)).to(cuda)
    labels, ncl, stats = PC.dbscan_labels(t, count, eps, ms, thr, mp)
    n = len(pts) if count is None else int(count)
    return labels.cpu().numpy()[:n], int(ncl.item()), stats.cpu().numpy()


def _check(pts, cuda, eps=0.2, ms=5, thr=None, mp=0, count=None):
    """Device == restatement: labels, every count, the cluster number."""
    n = len(pts) if count is None else int(count)
    want, core_rows, wst = N.dbscan(np.asarray(pts).reshape(-1, 3)[:n], eps, ms, thr, mp)
    got, ncl, st = _run(pts, cuda, eps, ms, thr, mp, count)
    print(f"n={n} participants={int(wst[2])} core={int(wst[3])} border={int(wst[4])} noise={int(wst[5])} "
          f"clusters={int(wst[6])} label mismatches={int((got != want).sum())}")
    assert np.array_equal(got, want)
    assert np.array_equal(st, wst) and ncl == int(wst[6])
    return want, core_rows, wst


@pytest.mark.gpu
@pytest.mark.parametrize("scene", SCENES)
def test_fixture_scene_labels_are_sklearns(scene, gold, restated, cuda):
    pts, eps, ms, thr = _scene(gold, scene)
    got, ncl, st = _run(pts, cuda, eps, ms, thr)
    want, core_rows, wst = restated[scene]
    rows = N.participants(pts, thr)
    assert np.array_equal(got[rows], gold[f"{scene}_labels"])     # sklearn itself
    assert np.array_equal(got, want) and np.array_equal(st, wst) and ncl == gold[f"{scene}_labels"].max() + 1
    assert st[3] == len(gold[f"{scene}_core"])


@pytest.mark.gpu
@pytest.mark.parametrize("scene", SCENES)
def test_fixture_scene_reversed_rows(scene, gold, cuda):
    """The numbering follows row order: the reversed input against the restatement of the reversed input."""
    pts, eps, ms, thr = _scene(gold, scene)
    _check(pts[::-1].copy(), cuda, eps, ms, thr)


@pytest.mark.gpu
def test_too_few_points_are_noise(cuda):
    g = np.random.default_rng(0)
    for n in (0, 1, 4):                                           # min_samples - 1 = 4
        pts = np.c_[0.01 * g.random(n), np.full(n, 2.0), 0.01 * g.random(n)]
        got, ncl, st = _run(pts, cuda, 0.2, 5)
        assert (got == -1).all() and ncl == 0 and list(st) == [n, 0, n, 0, 0, n, 0, 0]
    # live count 0 of a non-empty buffer
    got, ncl, st = _run(np.zeros((100, 3)), cuda, 0.2, 5, count=0)
    assert ncl == 0 and list(st) == [0] * 8


@pytest.mark.gpu
def test_min_samples_one_makes_everyone_core(cuda):
    g = np.random.default_rng(1)
    pts = np.c_[g.uniform(0, 3, 500), np.full(500, 2.0), g.uniform(0, 3, 500)]
    want, core_rows, st = _check(pts, cuda, 0.1, 1)
    assert st[3] == 500 and st[4] == 0 and st[5] == 0 and (want >= 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 65])
def test_chain_at_spacing_exactly_eps(n, cuda):
    """dx*dx == eps*eps exactly (eps = 0.25, a power of two): one chain cluster across wave boundaries;
    one part in 2^40 further apart, nobody has a neighbour."""
    line = lambda s: np.c_[s * np.arange(n), np.full(n, 2.0), np.zeros(n)]      # noqa: E731
    want, _, st = _check(line(0.25), cuda, 0.25, 3)
    assert (want == 0).all() and st[3] == n - 2 and st[4] == 2 and st[6] == 1
    s = 0.25 * (1 + 2.0 ** -40)
    assert np.all(np.diff(line(s)[:, 0]) > 0.25)
    for ms in (2, 3):
        want, _, st = _check(line(s), cuda, 0.25, ms)
        assert (want == -1).all() and st[5] == n
    _check(line(0.25).reshape(-1, 3)[::-1].copy(), cuda, 0.25, 2)


@pytest.mark.gpu
def test_points_on_cell_edges_and_corners(cuda):
    """Points on the corners, edge midpoints and centres of the kernel's own cells (edge
    eps / sqrt(2) * (1 - 2^-20), origin at the smallest x and z): the floor of a quotient may fall to
    either side there; the labels must not care."""
    eps = 0.2
    g = eps / math.sqrt(2.0) * (1.0 - 2.0 ** -20)
    k = np.arange(24)
    u, v = np.meshgrid(k * g, k * g, indexing="ij")
    corners = np.c_[u.ravel(), v.ravel()]
    mids = np.c_[(u + 0.5 * g).ravel(), v.ravel()]
    rng = np.random.default_rng(5)
    for ms, keep in ((5, 0.6), (9, 0.8), (3, 0.35)):
        xz = np.concatenate([corners, mids, corners + 0.5 * g])
        xz = xz[rng.random(len(xz)) < keep]
        rng.shuffle(xz)
        xz = np.concatenate([[[0.0, 0.0]], xz])                  # the grid's origin
        want, _, st = _check(np.c_[xz[:, 0], np.full(len(xz), 2.0), xz[:, 1]], cuda, eps, ms)
        assert st[3] > 0 and st[2] == len(xz)
    # pairs across a corner of the 5 x 5 block: two cells apart on both axes and still within eps
    a = np.array([[g * (1 - 1e-9), g * (1 - 1e-9)], [2 * g, 2 * g]])
    assert np.hypot(*(a[1] - a[0])) < eps
    xz = np.concatenate([[[0.0, 0.0]], a, a + [5 * g, 0], a[:1] + [9 * g, 0]])
    want, _, st = _check(np.c_[xz[:, 0], np.full(len(xz), 2.0), xz[:, 1]], cuda, eps, 2)
    assert st[6] == 2 and st[3] == 5 and st[5] == 1


@pytest.mark.gpu
def test_coincident_points_and_one_far_away(cuda):
    pts = np.tile([[1.0, 2.0, -3.0]], (20001, 1))
    pts[12345] = [4.0, 2.0, 4.0]
    got, ncl, st = _run(pts, cuda, 0.2, 5)
    assert ncl == 1 and got[12345] == -1 and (np.delete(got, 12345) == 0).all()
    assert list(st) == [20001, 0, 20001, 20000, 0, 1, 1, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("n,side", [(4097, 4.0), (100003, 20.0)])
def test_random_points_cross_the_sort_tiles(n, side, cuda):
    g = np.random.default_rng(n)
    pts = np.c_[g.uniform(0, side, n), g.uniform(1.0, 2.0, n), g.uniform(0, side, n)]
    pts[: n // 3, [0, 2]] = g.normal(side / 2, side / 20, (n // 3, 2))       # a dense middle: cells above min_samples
    want, _, st = _check(pts, cuda, 0.05, 5)
    assert st[6] > 10 and st[4] > 0 and st[5] > 0


@pytest.mark.gpu
def test_non_finite_rows(cuda):
    g = np.random.default_rng(2)
    pts = np.c_[g.uniform(0, 1, 600), np.full(600, 2.0), g.uniform(0, 1, 600)]
    bad = g.choice(600, 60, replace=False)
    for k, r in enumerate(bad):
        pts[r, k % 3] = (np.nan, np.inf, -np.inf)[(k // 3) % 3]
    want, _, st = _check(pts, cuda, 0.06, 5)
    assert (want[bad] == -2).all() and st[1] == 60 and st[0] == 540 and st[2] == 540
    # with the bad rows taken out nothing else changes: they are nobody's neighbour
    keep = np.setdiff1d(np.arange(600), bad)
    alone = N.dbscan(pts[keep], 0.06, 5)[0]
    assert np.array_equal(want[keep], alone)


@pytest.mark.gpu
def test_height_threshold(cuda):
    g = np.random.default_rng(3)
    pts = np.c_[g.uniform(0, 1, 800), g.uniform(1.0, 1.6, 800), g.uniform(0, 1, 800)]
    pts[::5, 1] = 1.3                                            # exactly at the threshold: takes part
    pts[1::5, 1] = np.nextafter(1.3, 0.0)
    want, _, st = _check(pts, cuda, 0.06, 5, thr=1.3)
    assert (want[::5] >= -1).all() and (want[1::5] == -2).all() and 160 < st[2] < 800
    for thr in (None, float("nan")):
        want, _, st = _check(pts, cuda, 0.06, 5, thr=thr)
        assert st[2] == 800
    _check(pts, cuda, 0.06, 5, thr=-np.inf)


@pytest.mark.gpu
def test_sampling_rule(cuda):
    g = np.random.default_rng(4)
    n = 340
    pts = np.c_[g.uniform(0, 1, n), np.where(g.random(n) < 0.1, 0.0, 2.0), g.uniform(0, 1, n)]
    pts[:39, 1] = 0.0
    pts[39:, 1] = 2.0                                            # e = 301 eligible rows
    g.shuffle(pts)
    e = int((pts[:, 1] >= 1.3).sum())
    assert e == 301
    for m, taken in ((400, e), (301, e), (300, 300), (100, 100), (1, 1)):     # e < m, e == m, e = m + 1, e = 3 m + 1
        want, _, st = _check(pts, cuda, 0.08, 3, thr=1.3, mp=m)
        assert st[2] == taken and (want == -2).sum() == n - taken


@pytest.mark.gpu
def test_overflowing_extent_raises_the_flag(cuda):
    g = np.random.default_rng(6)
    pts = np.c_[g.uniform(0, 0.01, 200), np.full(200, 2.0), g.uniform(0, 0.01, 200)]
    pts[100:, 0] += 1e4                                          # 1e4 / (0.001 / sqrt 2) cells > 2^21
    pts[7, 1] = 0.0
    got, ncl, st = _run(pts, cuda, 0.001, 3, thr=1.3)
    assert ncl == 0 and st[7] == 1 and st[6] == 0 and st[2] == 199 and st[3] == 0 and st[4] == 0 and st[5] == 199
    assert got[7] == -2 and (np.delete(got, 7) == -1).all()
    # an extent that overflows fp64 itself
    pts[0, 2], pts[1, 2] = -1.7e308, 1.7e308
    got, ncl, st = _run(pts, cuda, 0.001, 3, thr=1.3)
    assert ncl == 0 and st[7] == 1 and (np.delete(got, 7) == -1).all()


def _table(pts, cuda, eps, ms, thr, max_clusters=4096, keep_ws=True):
    import torch

    from depth_pro import pointcloud as PC

    t = torch.from_numpy(np.ascontiguousarray(pts)).to(cuda)
    labels, ncl, _ = PC.dbscan_labels(t, None, eps, ms, thr)
    if not keep_ws:
        labels = labels.clone()
    table, order, offsets = PC.cluster_table(t, labels, ncl, None, max_clusters)
    return labels.cpu().numpy(), int(ncl.item()), table.cpu().numpy(), order.cpu().numpy(), offsets.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["blobs0", "levelled", "border"])
def test_table_on_fixture(scene, gold, restated, cuda):
    pts, eps, ms, thr = _scene(gold, scene)
    want_labels, core_rows, _ = restated[scene]
    labels, k, table, order, offsets = _table(pts, cuda, eps, ms, thr)
    assert np.array_equal(labels, want_labels)
    wt, worder, woff = N.table(pts, want_labels, core_rows)
    assert k == len(wt) and np.array_equal(table[:k, :8], wt) and (table[:k, 11] == 0).all() and (table[k:] == 0).all()
    assert np.array_equal(offsets[:k + 1], woff) and np.array_equal(order[:woff[-1]], worder)
    for c in range(k):
        r = worder[woff[c]:woff[c + 1]]
        assert np.array_equal(r, np.flatnonzero(want_labels == c))          # points_2d[labels == c]
        for col, axis in ((8, 0), (9, 1), (10, 2)):
            v = pts[r, axis]
            bound = (len(r) - 1) * 2.0 ** -53 * math.fsum(np.abs(v))
            err = abs(table[c, col] - math.fsum(v))
            assert err <= bound, (c, col, err, bound)
    # labels that did not come straight from dbscan_labels: everything but the smallest core row
    _, _, t2, o2, f2 = _table(pts, cuda, eps, ms, thr, keep_ws=False)
    assert (t2[:k, 1] == -1).all() and np.array_equal(t2[:k, [0, 2, 3, 4, 5, 6, 7]], wt[:, [0, 2, 3, 4, 5, 6, 7]])
    assert np.array_equal(o2[:woff[-1]], worder) and np.array_equal(f2[:k + 1], woff)


@pytest.mark.gpu
def test_table_truncates_at_max_clusters(gold, restated, cuda):
    """max_clusters below the cluster count: rows and offsets up to it, nothing written past them."""
    import torch

    from depth_pro import _lib

    pts, eps, ms, thr = _scene(gold, "blobs0")
    want_labels, core_rows, _ = restated["blobs0"]
    wt, worder, woff = N.table(pts, want_labels, core_rows)
    lib = _lib.load()
    n, mc = len(pts), 3
    assert len(wt) > mc
    t = torch.from_numpy(np.ascontiguousarray(pts)).to(cuda)
    ws = torch.zeros(int(lib.dp_cluster_workspace_size(n)), dtype=torch.uint8, device=cuda)
    labels = torch.empty(n, dtype=torch.int32, device=cuda)
    ncl = torch.empty((), dtype=torch.int32, device=cuda)
    stats = torch.empty(8, dtype=torch.float64, device=cuda)
    table = torch.full((10, 12), 7.0, dtype=torch.float64, device=cuda)
    order = torch.full((n,), -7, dtype=torch.int32, device=cuda)
    offsets = torch.full((11,), -7, dtype=torch.int32, device=cuda)
    s = torch.cuda.current_stream(cuda).cuda_stream
    assert lib.dp_cluster_dbscan(t.data_ptr(), None, n, eps, ms, thr, 0, labels.data_ptr(), ncl.data_ptr(),
                                 stats.data_ptr(), ws.data_ptr(), ws.numel(), s) == 0
    assert lib.dp_cluster_table(t.data_ptr(), labels.data_ptr(), None, n, ncl.data_ptr(), mc, table.data_ptr(),
                                order.data_ptr(), offsets.data_ptr(), ws.data_ptr(), ws.numel(), s) == 0
    table, order, offsets = table.cpu().numpy(), order.cpu().numpy(), offsets.cpu().numpy()
    assert np.array_equal(table[:mc, :8], wt[:mc]) and (table[mc:] == 7.0).all()
    assert np.array_equal(offsets[:mc + 1], woff[:mc + 1]) and (offsets[mc + 1:] == -7).all()
    assert np.array_equal(order[:woff[-1]], worder) and (order[woff[-1]:] == -7).all()


# ---- the frame loop ---------------------------------------------------------------------------------------

class _FixtureModel:
    """Stands in for the engine in the loop tests: returns a fixed depth map and focal length."""

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
def test_loop_cluster_pointcloud(tmp_path, cuda):
    """--cluster_pointcloud adds {base}_clusters.json and {base}_labels.npy (labels of the rows of
    {base}_clean.ply = the restatement on that file's points); without the flag the loop writes exactly
    the files it wrote before, byte for byte."""
    import generate_depth_maps as G
    from depth_pro import pointcloud as PC

    plain, out = tmp_path / "clean", tmp_path / "cluster"
    clean_kw = dict(clean_pointcloud=True, stray_radius=0.25, stray_neighbors=12)
    par = dict(cluster_eps=0.12, cluster_min_samples=6, cluster_height=float("nan"), cluster_max_points=3000)
    _run_loop(tmp_path, cuda, plain, **clean_kw)
    # the same plane for both runs (a fit of its own could differ in its last digits): read from the first run's directory
    _run_loop(tmp_path, cuda, out, cluster_pointcloud=True, ground_params_dir=str(plain), **clean_kw, **par)
    assert "ground.json" in os.listdir(plain)
    names = sorted(set(os.listdir(plain)) - {"ground.json"})
    assert names == ["output_0000_clean.ply", "output_0000_depth.png", "output_0001_clean.ply", "output_0001_depth.png"]
    assert sorted(os.listdir(out)) == sorted(names + [f"output_{k:04d}_{s}" for k in range(2)
                                                      for s in ("clusters.json", "labels.npy")])
    for name in names:
        assert open(plain / name, "rb").read() == open(out / name, "rb").read(), name
    for k in range(2):
        pts, _ = PC.read_ply(str(out / f"output_{k:04d}_clean.ply"))
        labels = np.load(out / f"output_{k:04d}_labels.npy")
        assert labels.dtype == np.int32 and labels.shape == (len(pts),)
        want, core_rows, st = N.dbscan(pts, 0.12, 6, None, 3000)
        assert len(pts) > 3000 and st[2] == 3000 and st[6] > 0
        assert np.array_equal(labels, want)
        js = json.load(open(out / f"output_{k:04d}_clusters.json"))
        assert js["parameters"] == {"eps": 0.12, "min_samples": 6, "height_threshold": None, "max_points": 3000}
        assert [js[key] for key in PC.CLUSTER_STATS] == [int(v) for v in st]
        wt, _, _ = N.table(pts, want, core_rows)
        assert [(c["id"], c["count"], c["min_core_row"]) for c in js["cluster_table"]] == \
            [(c, int(r[0]), int(r[1])) for c, r in enumerate(wt)]
        assert [c["bbox"]["x"] + c["bbox"]["z"] + c["bbox"]["y"] for c in js["cluster_table"]] == \
            [list(r[2:8]) for r in wt]
    src = sorted(str(p) for p in (tmp_path / "frames").glob("*.png"))
    assert G.plan_frames(src, str(out), 1, 0, True, cleaned=True, clustered=True) == []
    assert G.plan_frames(src, str(plain), 1, 0, True, cleaned=True, clustered=True) == [0, 1]
