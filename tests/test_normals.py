"""Oriented mesh points (ABI 19, csrc/dp_normals.hip): voxel grid, hybrid neighbour search, normals, orientation.

The expected values come from tests/normals_numpy.py, a numpy restatement of the header's specification, which
the non-GPU tests pin to scipy's cKDTree, numpy's eigh and np.unique through tests/golden/golden_normals.npz
(made by tests/golden/make_golden_normals.py, which also asserts that cloud A has no distance ties and no small
eigen-gap).  Voxel membership, counts, colours, neighbour lists and counts are compared exactly; voxel points
within the summation bound 4 * 2^-53 * m * max |coordinate|; normals by length (4 * 2^-52), Rayleigh excess
(1e-9 * l2: two-pass fp64 rounding over <= 64 neighbours and a converged 3 x 3 solver stay near 1e-13 * l2, the
wrong eigenvector costs at least l1 - l0) and direction (|sin| <= 1e-9 / relative gap).
"""

import ctypes
import json
import os
import sys

import numpy as np
import pytest

import normals_numpy as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RADIUS, MAX_NN, VOXEL = 0.1, 30, 0.05
CENTRE = (1.5, 0.6, 3.0)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_normals.npz"))


@pytest.fixture(scope="module")
def clouds(gold):
    """name -> (points, colours or None, live count or None, max_nn)"""
    return {"A": (gold["A_points"], gold["A_colors"], None, MAX_NN), "B": (gold["B_points"], None, None, 8),
            "C": (gold["C_points"], gold["A_colors"], int(gold["C_count"]), MAX_NN)}


@pytest.fixture(scope="module")
def restated(clouds):
    """The restatement's voxels and neighbour lists, computed once per cloud and never changed."""
    out = {}
    for name, (pts, cols, count, k) in clouds.items():
        out[name] = {"vox": N.voxel_downsample(pts, cols, count, VOXEL), "knn": N.knn_search(pts, count, RADIUS, k)}
    down = out["A"]["vox"]["points"]
    out["A_down"] = {"points": down, "knn": N.knn_search(down, None, RADIUS, MAX_NN)}
    return out


# ---- no GPU ---------------------------------------------------------------------------------------------

def test_restatement_is_pinned_to_ckdtree_eigh_and_unique(gold, restated):
    assert list(gold["params"]) == [RADIUS, MAX_NN, VOXEL] and tuple(gold["sphere_centre"]) == CENTRE
    nbr, cnt, stats, total, ties = restated["A"]["knn"]
    assert np.array_equal(nbr, gold["A_kd"].astype(np.int32)) and not ties
    assert (stats[2], stats[3], total.max()) == (60, 101, 41)
    out = N.estimate_normals(gold["A_points"], nbr, cnt)
    rows = cnt >= 3
    w = gold["A_eigh"]
    assert (np.abs(out["lam"][rows] - w[rows]).max(axis=1) <= 1e-13 * w[rows, 2]).all()
    assert ((w[rows, 1] - w[rows, 0]) / w[rows, 2]).min() >= 1e-6
    vox = restated["A"]["vox"]
    assert vox["n_out"] == 1664 and np.array_equal(vox["voxel_of"], gold["A_unique_inverse"].astype(np.int32))
    assert (np.diff(vox["keys"]) > 0).all() and vox["count"].sum() == 3000
    dn = restated["A_down"]["knn"]
    assert dn[2][2] == 65 and not dn[4]
    b = restated["B"]["knn"]
    assert b[4] and (b[3] > 8).all() and b[2][3] == len(gold["B_points"])
    c = restated["C"]
    assert c["knn"][2][1] == 5 and c["vox"]["stats"][1] == 5 and (c["vox"]["voxel_of"][gold["C_bad"]] == -1).all()


def test_restatement_rules_on_small_cases():
    flat = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 1e-3]], dtype=np.float64) * 0.01 + [0, 0, 2.0]
    nbr, cnt, stats, _, _ = N.knn_search(flat, None, 0.1, 4)
    assert (cnt == 4).all() and stats[3] == 5 and list(nbr[:, 0]) == [0, 1, 2, 3, 4]
    assert list(nbr[0]) == [0, 4, 1, 2]                       # (d2, row): rows 1 and 2 tie, the smaller first
    out = N.estimate_normals(flat, *N.knn_search(flat, None, 0.1, 5)[:2])
    assert (np.abs(out["normals"][:, 2]) > 0.999).all() and (out["normals"][:, 2] < 0).all() and out["stats"][4] == 5
    away = N.estimate_normals(flat, *N.knn_search(flat, None, 0.1, 5)[:2], camera=(0, 0, 9.0))
    assert (away["normals"][:, 2] > 0).all()
    two = N.estimate_normals(flat[:2], *N.knn_search(flat[:2], None, 0.1, 5)[:2])
    assert np.array_equal(two["normals"], [[0, 0, -1.0], [0, 0, -1.0]]) and two["stats"][2] == 2
    v = N.voxel_downsample(np.array([[0, 0, 0], [0.01, 0, 0], [1.0, 0, 0]]), np.array([[1, 0, 255], [2, 0, 255], [9, 9, 9]]), None, 0.05)
    assert v["n_out"] == 2 and list(v["count"]) == [2, 1] and list(v["voxel_of"]) == [0, 0, 1]
    assert v["colors"].tolist() == [[2, 0, 255], [9, 9, 9]] and v["points"][0, 0] == 0.005       # 1.5 rounds up
    far = np.array([[0.0, 0, 0], [1e6, 0, 0]])
    assert N.knn_search(far, None, 0.1, 5)[2][5] == 1 and N.voxel_downsample(far, None, None, 0.05)["n_out"] == 0


def test_workspace_size_and_argument_errors_need_no_device():
    from depth_pro import _lib

    lib = _lib.load()
    sizes = [lib.dp_normals_workspace_size(n) for n in (0, 1, 2048, 2049, 100003, 8294400)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert lib.dp_normals_workspace_size(-5) == sizes[0]
    assert sizes[-1] >= 41 * 8294400 + lib.dp_clean_workspace_size(8294400)
    P, big, ARG, SHAPE = 4096, 1 << 40, 1000, 1001
    f64 = ctypes.c_double

    def vox(points=P, colors=None, n=8, voxel=0.05, out=P, cout=None, members=P, voxel_of=P, n_out=P, stats=P, ws=P, wsb=big):
        return lib.dp_voxel_downsample(points, colors, None, n, f64(voxel), out, cout, members, voxel_of, n_out, stats, ws,
                                       wsb, None)

    def knn(points=P, n=8, radius=0.1, k=30, nbr=P, cnt=P, stats=P, ws=P, wsb=big):
        return lib.dp_knn_search(points, None, n, f64(radius), k, nbr, cnt, stats, ws, wsb, None)

    def nrm(points=P, n=8, nbr=P, cnt=P, k=30, cam=(0.0, 0.0, 0.0), normals=P, stats=P):
        return lib.dp_estimate_normals(points, None, n, nbr, cnt, k, None if cam is None else (f64 * 3)(*cam), 1, normals,
                                       stats, None)

    short = lib.dp_normals_workspace_size(8) - 1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert vox(voxel=bad) == SHAPE and knn(radius=bad) == SHAPE, bad
    assert vox(n=-1) == SHAPE and knn(n=-1) == SHAPE and nrm(n=-1) == SHAPE
    for k in (0, -3, 65):
        assert knn(k=k) == SHAPE and nrm(k=k) == SHAPE, k
    assert nrm(cam=(0.0, float("nan"), 0.0)) == SHAPE and nrm(cam=(float("inf"), 0.0, 0.0)) == SHAPE
    for kw in ({"points": None}, {"out": None}, {"members": None}, {"voxel_of": None}, {"n_out": None}, {"stats": None},
               {"colors": P}, {"ws": None}, {"ws": P + 4}, {"wsb": 16}, {"wsb": short}):
        assert vox(**kw) == ARG, kw
    for kw in ({"points": None}, {"nbr": None}, {"cnt": None}, {"stats": None}, {"ws": None}, {"ws": P + 4}, {"wsb": short}):
        assert knn(**kw) == ARG, kw
    for kw in ({"points": None}, {"nbr": None}, {"cnt": None}, {"cam": None}, {"normals": None}, {"stats": None}):
        assert nrm(**kw) == ARG, kw


def test_python_layer_refuses_bad_arguments_and_host_tensors():
    import torch

    from depth_pro import _lib
    from depth_pro import pointcloud as PC

    assert len(PC.VOXEL_STATS) == len(PC.KNN_STATS) == len(PC.NORMAL_STATS) == 8
    assert PC.NORMAL_STATS.index("error") == PC.KNN_STATS.index("error") == PC.VOXEL_STATS.index("error") == 5
    pts = torch.zeros(4, 3, dtype=torch.float64)
    for call in (lambda: PC.voxel_downsample(pts), lambda: PC.knn_search(pts), lambda: PC.estimate_normals(pts),
                 lambda: PC.oriented_points(pts)):
        with pytest.raises(_lib.DPError):
            call()
    for call in (lambda: PC.voxel_downsample(pts, voxel_size=0.0), lambda: PC.knn_search(pts, radius=float("nan")),
                 lambda: PC.knn_search(pts, max_nn=65), lambda: PC.estimate_normals(pts, max_nn=0),
                 lambda: PC.oriented_points(pts, voxel_size=-1.0)):
        with pytest.raises(ValueError):
            call()


def test_ply_with_normals_round_trips_byte_exact(tmp_path):
    from depth_pro import pointcloud as PC

    g = np.random.default_rng(5)
    pts, nrm = g.normal(size=(37, 3)), g.normal(size=(37, 3))
    nrm[3] = [0.0, -0.0, np.nan]
    cols = g.integers(0, 256, (37, 3), dtype=np.uint8)
    for c in (cols, None):
        a = PC.write_ply_normals(str(tmp_path / "a"), pts, nrm, c)
        assert a.endswith("a.ply")
        p2, n2, c2 = PC.read_ply_normals(a)
        assert p2.tobytes() == pts.tobytes() and n2.tobytes() == nrm.tobytes()
        assert (c2 is None) if c is None else np.array_equal(c2, c)
        b = PC.write_ply_normals(str(tmp_path / "b.ply"), p2, n2, c2)
        raw = open(a, "rb").read()
        assert raw == open(b, "rb").read()
        head, body = raw.split(b"end_header\n", 1)
        want = ["ply", "format binary_little_endian 1.0", "element vertex 37"] + [f"property double {k}" for k in
                                                                                    ("x", "y", "z", "nx", "ny", "nz")]
        want += [f"property uchar {k}" for k in ("red", "green", "blue")] if c is not None else []
        assert head.decode("ascii").splitlines() == want and len(body) == 37 * (51 if c is not None else 48)
        rec = np.frombuffer(body, dtype=np.uint8).reshape(37, -1)
        assert PC.write_ply_normals_records(str(tmp_path / "c.ply"), rec) and open(tmp_path / "c.ply", "rb").read() == raw
    assert PC.read_ply_normals(PC.write_ply_normals(str(tmp_path / "e.ply"), np.zeros((0, 3)), np.zeros((0, 3))))[0].shape == (0, 3)
    with pytest.raises(ValueError):
        PC.read_ply_normals(PC.write_ply(str(tmp_path / "plain.ply"), pts, cols))
    # files without normals read as before
    assert PC.read_ply(str(tmp_path / "plain.ply"))[0].tobytes() == pts.tobytes()


def test_cli_and_resume_know_the_oriented_files(monkeypatch, tmp_path):
    import generate_depth_maps as G

    for extra in (["--voxel_size", "0"], ["--voxel_size", "-0.05"], ["--voxel_size", "nan"], ["--normals_max_nn", "0"],
                  ["--normals_max_nn", "65"]):
        monkeypatch.setattr(G, "_model", lambda *a, **k: pytest.fail("the model was loaded"))
        monkeypatch.setattr(sys, "argv", ["generate_depth_maps.py", "--input_dir", str(tmp_path), "--mesh_points"] + extra)
        with pytest.raises(SystemExit) as e:
            G.main()
        assert e.value.code == 2, extra
    with pytest.raises(ValueError):
        G.batch_generate_depth_maps(str(tmp_path), str(tmp_path / "o"), mesh_points=True, voxel_size=0.0)
    with pytest.raises(ValueError):
        G.batch_generate_depth_maps(str(tmp_path), str(tmp_path / "o"), mesh_points=True, normals_max_nn=65)
    frames = [str(tmp_path / f"f{k}.png") for k in range(3)]
    assert G.oriented_name(frames[0]) == "f0_oriented.ply" and G.oriented_json_name(frames[0]) == "f0_oriented.json"
    for k in (0, 1):
        for s in ("depth.png", "clean.ply"):
            (tmp_path / f"f{k}_{s}").write_bytes(b"")
    (tmp_path / "f0_oriented.ply").write_bytes(b"")
    (tmp_path / "f0_oriented.json").write_bytes(b"")
    (tmp_path / "f1_oriented.ply").write_bytes(b"")              # the json is missing: not done
    assert G.plan_frames(frames, str(tmp_path), 1, 0, True, cleaned=True) == [2]
    assert G.plan_frames(frames, str(tmp_path), 1, 0, True, cleaned=True, oriented=True) == [1, 2]
    assert G.plan_frames(frames, str(tmp_path), 1, 0, False, oriented=True) == [0, 1, 2]


# ---- GPU ------------------------------------------------------------------------------------------------

def _dev(a, cuda):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _vox(pts, cols, count, cuda, voxel=VOXEL):
    from depth_pro import pointcloud as PC

    out, cout, members, voxel_of, n_out, stats = PC.voxel_downsample(_dev(pts, cuda), None if cols is None else _dev(cols, cuda),
                                                                     count, voxel)
    k = int(n_out.item())
    n = len(pts) if count is None else count
    return {"points": out.cpu().numpy()[:k], "colors": None if cout is None else cout.cpu().numpy()[:k],
            "count": members.cpu().numpy()[:k], "voxel_of": voxel_of.cpu().numpy()[:n], "n_out": k, "stats": stats.cpu().numpy()}


def _knn(pts, count, cuda, radius=RADIUS, k=MAX_NN):
    from depth_pro import pointcloud as PC

    nbr, cnt, stats = PC.knn_search(_dev(pts, cuda), count, radius, k)
    n = len(pts) if count is None else count
    return nbr.cpu().numpy()[:n], cnt.cpu().numpy()[:n], stats.cpu().numpy()


def _normals(pts, nbr, cnt, count, cuda, camera=(0, 0, 0), orient=True):
    """Device normals on device-made lists of the first `count` rows (nbr / cnt hold exactly those rows)."""
    import torch

    from depth_pro import pointcloud as PC

    n = len(pts)
    full_nbr = np.full((n, nbr.shape[1]), -1, np.int32)
    full_cnt = np.zeros(n, np.int32)
    full_nbr[:len(nbr)], full_cnt[:len(cnt)] = nbr, cnt
    normals, stats = PC.normals_from_neighbors(_dev(pts, cuda), _dev(full_nbr, cuda), _dev(full_cnt, cuda), count, camera, orient)
    torch.cuda.synchronize()
    return normals.cpu().numpy()[:len(nbr)], stats.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "C"])
def test_voxel_downsample(name, clouds, restated, cuda):
    pts, cols, count, _ = clouds[name]
    want, got = restated[name]["vox"], _vox(pts, cols, count, cuda)
    print(f"{name}: voxels {got['n_out']} (want {want['n_out']}), stats {got['stats']}")
    assert got["n_out"] == want["n_out"] and np.array_equal(got["voxel_of"], want["voxel_of"])
    assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["colors"], want["colors"])
    assert np.array_equal(got["stats"], want["stats"])
    err = np.abs(got["points"] - want["points"])
    print(f"  largest point error / bound {np.max(err / want['bound']):.3f}")
    assert (err <= want["bound"]).all()
    # ascending key order: the restatement numbers its voxels by ascending key, and voxel_of agrees row for row
    assert (np.diff(want["keys"]) > 0).all() and len(want["keys"]) == got["n_out"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_knn_search(name, clouds, restated, cuda):
    """Fails on the parent commit: dp_knn_search does not exist there."""
    pts, _, count, k = clouds[name]
    wnbr, wcnt, wstats, _, _ = restated[name]["knn"]
    nbr, cnt, stats = _knn(pts, count, cuda, k=k)
    print(f"{name}: stats {stats} (want {wstats}); rows that differ {np.count_nonzero((nbr != wnbr).any(axis=1))}")
    assert np.array_equal(cnt, wcnt) and np.array_equal(nbr, wnbr)
    assert stats[3] == wstats[3] and np.array_equal(stats, wstats)


def _check_normals(normals, pts, nbr, cnt, camera=(0, 0, 0), orient=True):
    """Length, Rayleigh excess, direction, defaults and non-finite rows against the restatement on these very lists.
    Returns the restatement's output."""
    n = len(nbr)
    want = N.estimate_normals(pts, nbr, cnt, n, camera, orient)
    fin = np.isfinite(pts[:n]).all(axis=1)
    few = fin & (cnt < 3)
    rows = np.flatnonzero(fin & (cnt >= 3))
    assert (normals[~fin] == 0).all() and len(rows) > 0
    assert (np.abs(normals[few][:, 2]) == 1).all() and (normals[few][:, :2] == 0).all()
    ln = np.sqrt((normals[rows] ** 2).sum(axis=1))
    lam, C = want["lam"][rows], want["C"][rows]
    excess = np.einsum("ni,nij,nj->n", normals[rows], C, normals[rows]) - lam[:, 0]
    gap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
    keep = gap >= 1e-6
    sin = np.linalg.norm(np.cross(normals[rows], want["normals"][rows]), axis=1)
    if keep.any():
        print(f"  rows {len(rows)}: | |n| - 1 | <= {np.abs(ln - 1).max():.3e}; Rayleigh excess / l2 <= {np.max(excess / lam[:, 2]):.3e}; "
              f"sin * gap <= {np.max((sin * gap)[keep]):.3e}; direction check skips {np.count_nonzero(~keep)}")
    assert (np.abs(ln - 1) <= 4 * 2.0 ** -52).all()
    assert (excess <= 1e-9 * lam[:, 2]).all()
    assert np.count_nonzero(~keep) <= 0.01 * len(rows)
    assert (sin[keep] <= 1e-9 / gap[keep]).all()
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "C", "A_down"])
def test_estimate_normals(name, clouds, restated, cuda):
    if name == "A_down":
        pts, count = restated[name]["points"], None
    else:
        pts, _, count, _ = clouds[name]
    nbr, cnt, kst = _knn(pts, count, cuda)
    assert np.array_equal(nbr, restated[name]["knn"][0]) and np.array_equal(cnt, restated[name]["knn"][1])
    normals, stats = _normals(pts, nbr, cnt, count, cuda, orient=False)
    print(f"{name}: n={len(nbr)} knn stats {kst} normal stats {stats}")
    want = _check_normals(normals, pts, nbr, cnt, orient=False)
    assert np.array_equal(stats, want["stats"]) and stats[4] == 0 and stats[2] == kst[2]
    if name == "A_down":
        assert len(pts) == 1664 and kst[2] == 65


@pytest.mark.gpu
@pytest.mark.parametrize("camera", [(0.0, 0.0, 0.0), CENTRE])
def test_orientation(camera, clouds, cuda):
    from depth_pro import pointcloud as PC

    pts = clouds["A"][0]
    nbr, cnt, _ = _knn(pts, None, cuda)
    normals, stats = _normals(pts, nbr, cnt, None, cuda, camera=camera)
    want = _check_normals(normals, pts, nbr, cnt, camera=camera)
    to = np.asarray(camera) - pts
    dist = np.sqrt((to * to).sum(axis=1))
    dot = (normals * to).sum(axis=1)
    assert (dot >= -1e-12 * dist).all()
    keep = np.abs(want["dot"]) > 1e-12 * want["dist"]
    assert ((normals[keep] * want["normals"][keep]).sum(axis=1) > 0).all()
    lo = np.count_nonzero(want["flip"] & keep)
    print(f"camera {camera}: flipped {stats[4]} (restatement {lo} in the {keep.sum()} rows kept, {np.count_nonzero(~keep)} dropped)")
    assert lo <= stats[4] <= lo + np.count_nonzero(~keep) and 0 < stats[4] < len(pts)
    if camera == CENTRE:
        # rows whose whole neighbourhood lies on the sphere: the normal is radial and must point inward
        on = np.abs(np.linalg.norm(pts - CENTRE, axis=1) - 0.4) < 1e-12
        rows = np.flatnonzero(on & (cnt >= 3) & np.array([on[nbr[i, :cnt[i]]].all() for i in range(len(pts))]))
        assert len(rows) > 900 and (dot[rows] / dist[rows] > 0.9).all()
    # the public call is the search and the normals in one, with the search's counts beside the normals' own
    n2, st2 = PC.estimate_normals(_dev(pts, cuda), None, RADIUS, MAX_NN, camera)
    assert np.array_equal(n2.cpu().numpy(), normals) and list(st2.cpu().numpy()) == [3000, 0, 60, 101, stats[4], 0, 0, 0]


@pytest.mark.gpu
def test_edges(clouds, restated, cuda):
    from depth_pro import pointcloud as PC

    A = clouds["A"][0]
    # a live count of 0
    v = _vox(A, clouds["A"][1], 0, cuda)
    assert v["n_out"] == 0 and list(v["stats"]) == [0] * 8
    nbr, cnt, st = _knn(A, 0, cuda)
    assert nbr.shape == (0, MAX_NN) and list(st) == [0] * 8
    assert list(_normals(A, nbr, cnt, 0, cuda)[1]) == [0] * 8
    for empty in (lambda: PC.oriented_points(_dev(np.zeros((0, 3)), cuda)), ):
        assert int(empty()[2].item()) == 0
    # one point
    one = np.array([[1.0, 2.0, 3.0]])
    v = _vox(one, np.array([[7, 8, 9]], np.uint8), None, cuda)
    assert v["n_out"] == 1 and np.array_equal(v["points"], one) and v["colors"].tolist() == [[7, 8, 9]] and list(v["count"]) == [1]
    nbr, cnt, st = _knn(one, None, cuda)
    assert list(nbr[0]) == [0] + [-1] * (MAX_NN - 1) and list(cnt) == [1] and list(st) == [1, 0, 1, 0, 0, 0, 0, 0]
    nrm, st = _normals(one, nbr, cnt, None, cuda)
    assert nrm.tolist() == [[0.0, 0.0, -1.0]] and list(st) == [1, 0, 1, 0, 1, 0, 0, 0]       # the default is flipped too
    assert _normals(one, nbr, cnt, None, cuda, orient=False)[0].tolist() == [[0.0, 0.0, 1.0]]
    # all points in one voxel
    g = np.random.default_rng(3)
    blob = g.uniform(0, 0.01, (100, 3)) + [0.5, -0.2, 2.0]
    v = _vox(blob, None, None, cuda)
    w = N.voxel_downsample(blob, None, None, VOXEL)
    assert v["n_out"] == 1 and list(v["count"]) == [100] and (v["voxel_of"] == 0).all() and v["colors"] is None
    assert (np.abs(v["points"] - w["points"]) <= w["bound"]).all()
    # max_nn = 1: the row itself; max_nn = 64: nothing is cut in A (largest neighbourhood 41) or B (63)
    nbr, cnt, st = _knn(clouds["C"][0], clouds["C"][2], cuda, k=1)
    fin = np.isfinite(clouds["C"][0][:len(cnt)]).all(axis=1)
    assert np.array_equal(nbr[:, 0], np.where(fin, np.arange(len(cnt)), -1)) and np.array_equal(cnt, fin.astype(np.int32))
    for name in ("A", "B"):
        pts = clouds[name][0]
        nbr, cnt, st = _knn(pts, None, cuda, k=64)
        wnbr, wcnt, wst, total, _ = N.knn_search(pts, None, RADIUS, 64)
        assert np.array_equal(nbr, wnbr) and np.array_equal(cnt, wcnt) and np.array_equal(cnt, total) and st[3] == 0
    # a span that raises the error flag: counts 0, no voxels, and nothing faults
    far = np.array([[0.0, 0.0, 0.0], [1e6, 0.0, 0.0]])
    nbr, cnt, st = _knn(far, None, cuda)
    assert (cnt == 0).all() and (nbr == -1).all() and list(st) == [2, 0, 2, 0, 0, 1, 0, 0]
    v = _vox(far, None, None, cuda)
    assert v["n_out"] == 0 and (v["voxel_of"] == -1).all() and list(v["stats"]) == [2, 0, 0, 0, 0, 1, 0, 0]
    assert _normals(far, nbr, cnt, None, cuda, orient=False)[0].tolist() == [[0.0, 0.0, 1.0]] * 2


@pytest.mark.gpu
def test_oriented_points_is_downsample_then_normals(clouds, restated, cuda):
    from depth_pro import pointcloud as PC

    pts, cols, _, _ = clouds["A"]
    out, cout, n_out, normals, vst, nst = PC.oriented_points(_dev(pts, cuda), _dev(cols, cuda))
    k = int(n_out.item())
    v = _vox(pts, cols, None, cuda)
    assert k == 1664 and np.array_equal(out.cpu().numpy()[:k], v["points"]) and np.array_equal(cout.cpu().numpy()[:k], v["colors"])
    nbr, cnt, _ = _knn(v["points"], None, cuda, radius=2 * VOXEL)
    assert np.array_equal(normals.cpu().numpy()[:k], _normals(v["points"], nbr, cnt, None, cuda)[0])
    assert vst.cpu().numpy()[2] == 1664 and list(nst.cpu().numpy()[:4]) == [1664, 0, 65, 0]


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
def test_loop_mesh_points(tmp_path, cuda):
    """--mesh_points adds {base}_oriented.ply and {base}_oriented.json to the clean run's files, which stay byte for
    byte; the oriented cloud is the restatement's voxel grid of the written clean cloud, with unit normals."""
    import generate_depth_maps as G
    from depth_pro import pointcloud as PC

    plain, out = tmp_path / "clean", tmp_path / "mesh"
    kw = dict(clean_pointcloud=True, stray_radius=0.25, stray_neighbors=12)
    _run_loop(tmp_path, cuda, plain, **kw)
    _run_loop(tmp_path, cuda, out, mesh_points=True, voxel_size=0.1, normals_max_nn=20, ground_params_dir=str(plain), **kw)
    names = [f"output_{k:04d}_{s}" for k in range(2) for s in ("clean.ply", "depth.png")]
    assert sorted(os.listdir(plain)) == sorted(names + ["ground.json"])           # what the loop wrote before this change
    assert sorted(os.listdir(out)) == sorted(names + [f"output_{k:04d}_oriented.{e}" for k in range(2) for e in ("ply", "json")])
    for name in names:
        assert open(plain / name, "rb").read() == open(out / name, "rb").read(), name
    for k in range(2):
        js = json.load(open(out / f"output_{k:04d}_oriented.json"))
        assert js["parameters"] == {"voxel_size": 0.1, "radius": 0.2, "max_nn": 20, "camera_location": [0.0, 0.0, 0.0]}
        pts, nrm, cols = PC.read_ply_normals(str(out / f"output_{k:04d}_oriented.ply"))
        n_out = js["points"]
        assert len(pts) == n_out == js["voxel_stats"]["voxels"] == js["normal_stats"]["finite"] > 10
        assert js["voxel_stats"]["error"] == js["normal_stats"]["error"] == 0 and cols.shape == (n_out, 3)
        assert (np.abs(np.sqrt((nrm ** 2).sum(axis=1)) - 1) <= 4 * 2.0 ** -52).all()
        assert ((nrm * (0 - pts)).sum(axis=1) >= -1e-12 * np.sqrt((pts ** 2).sum(axis=1))).all()
        cp, cc = PC.read_ply(str(out / f"output_{k:04d}_clean.ply"))
        want = N.voxel_downsample(cp, cc, None, 0.1)
        assert n_out == want["n_out"] and (np.abs(pts - want["points"]) <= want["bound"]).all() and np.array_equal(cols, want["colors"])
        assert js["voxel_stats"]["finite"] == len(cp)
    src = sorted(str(p) for p in (tmp_path / "frames").glob("*.png"))
    assert G.plan_frames(src, str(out), 1, 0, True, cleaned=True, oriented=True) == []
    assert G.plan_frames(src, str(plain), 1, 0, True, cleaned=True, oriented=True) == [0, 1]
    assert G.plan_frames(src, str(plain), 1, 0, True, cleaned=True) == []
