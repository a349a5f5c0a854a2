"""Triangle mesh (additive to ABI 20, csrc/dp_mesh.hip): the exact k nearest other rows, the fan of triangles, the
triangle clean-up, the mean neighbour distance, the mesh PLY and the frame loop's --simple_mesh.

The expected values come from tests/mesh_numpy.py, a numpy restatement of the header's numbered rules, which the
non-GPU tests pin to scipy's cKDTree through tests/golden/golden_mesh.npz (made by tests/golden/make_golden_mesh.py,
which also asserts that the pinned clouds have no tie at the cut).  Indices, counts, statistics and triangles are
compared exactly; d2 bit for bit (both sides round the same three operations); the mean neighbour distance bit for bit
(fp64 sqrt and division are correctly rounded and the header fixes the order of every sum).
"""

import ctypes
import json
import os
import sys

import numpy as np
import pytest

import mesh_numpy as M
import normals_numpy as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VOXEL = 0.05
SENTINEL = -7


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_mesh.npz"))


@pytest.fixture(scope="module")
def cloud_a():
    g = np.load(os.path.join(GOLDEN, "golden_normals.npz"))
    return g["A_points"], g["A_colors"]


@pytest.fixture(scope="module")
def a_down(cloud_a):
    """Cloud A through the restated voxel grid: the realistic case (1664 voxels, strays included)."""
    return np.ascontiguousarray(N.voxel_downsample(cloud_a[0], None, None, VOXEL)["points"])


def _lattice(shift=0.0):
    i, j, k = np.meshgrid(np.arange(5), np.arange(5), np.arange(5), indexing="ij")
    P = np.c_[i.ravel(), j.ravel(), k.ravel()].astype(np.float64) * 0.25 + shift       # exact in binary: every cut a tie
    return np.ascontiguousarray(P[np.random.default_rng(4).permutation(len(P))])


def _knn_cases(a_down):
    """name -> (points, live count or None, k, cell_edge): the smallest shapes at which the search can go wrong."""
    g = np.random.default_rng(21)
    few = g.uniform(0.0, 0.3, (8, 3))
    cell = g.uniform(0.0, 0.09, (129, 3)) + 0.001
    clump = g.uniform(0.0, 0.05, (4, 3))
    blob = np.r_[g.uniform(0.0, 0.3, (200, 3)), [[2.5 + 0.31, 0.1, 0.1]]]
    bad = np.r_[a_down[:300], g.uniform(-1e3, 1e3, (200, 3))]            # 200 poison rows past the live count
    rows = g.choice(300, 12, replace=False)
    for t, r in enumerate(rows):
        bad[r, t % 3] = (np.nan, np.inf, -np.inf)[t % 3] if t < 9 else np.nan
    bad[rows[9:]] = np.nan
    cases = {f"n{n}": (few[:n], None, 6, 0.1) for n in (0, 1, 2, 6, 7, 8)}
    cases.update({f"one_cell_{n}": (cell[:n], None, 6, 0.1) for n in (63, 64, 65, 129)})
    cases["one_cell_129_k64"] = (cell, None, 64, 0.1)
    cases.update({f"lattice_k{k}": (_lattice(), None, k, 0.25) for k in (1, 6, 20, 64)})
    cases.update({f"lattice_negative_k{k}": (_lattice(-3.0), None, k, 0.25) for k in (6, 64)})
    cases["two_clumps"] = (np.r_[clump, clump[::-1] + [4.03, 0.0, 0.0]], None, 6, 0.1)     # 40 cell edges apart
    cases["outlier"] = (blob, None, 6, 0.1)                                                  # 25 cells from the blob
    cases.update({f"blob_k{k}": (blob[:200], None, k, 0.1) for k in (1, 20, 64)})
    cases.update({f"a_down_edge{e}": (a_down, None, 6, e) for e in (0.05, 0.1, 0.4)})
    cases["a_down_k20"] = (a_down, None, 20, 0.1)
    cases["non_finite_and_poison"] = (bad, 300, 6, 0.1)
    cases["span_error"] = (np.array([[0.0, 0.0, 0.0], [1e6, 0.0, 0.0], [1e6, 0.1, 0.0]]), None, 6, 0.1)
    return cases


KNN_NAMES = [f"n{n}" for n in (0, 1, 2, 6, 7, 8)] + [f"one_cell_{n}" for n in (63, 64, 65, 129)] + ["one_cell_129_k64"] + \
    [f"lattice_k{k}" for k in (1, 6, 20, 64)] + [f"lattice_negative_k{k}" for k in (6, 64)] + ["two_clumps", "outlier"] + \
    [f"blob_k{k}" for k in (1, 20, 64)] + [f"a_down_edge{e}" for e in (0.05, 0.1, 0.4)] + \
    ["a_down_k20", "non_finite_and_poison", "span_error"]


@pytest.fixture(scope="module")
def knn_cases(a_down):
    cases = _knn_cases(a_down)
    assert list(cases) == KNN_NAMES
    return cases


@pytest.fixture(scope="module")
def restated():
    """The restatement's answer per case, computed once and never changed."""
    return {}


def _want(name, knn_cases, restated):
    if name not in restated:
        pts, count, k, edge = knn_cases[name]
        restated[name] = M.knn_exact(pts, count, k, edge)
    return restated[name]


# ---- no GPU ---------------------------------------------------------------------------------------------

def test_restatement_is_pinned_to_ckdtree(gold, a_down):
    for P, k, key in ((gold["R_points"], 6, "R_kd6"), (gold["R_points"], 20, "R_kd20"), (a_down, 6, "A_down_kd6")):
        nbr, cnt, d2, stats, ties = M.knn_exact(P, None, k, 0.1)
        assert not ties and (cnt == k).all() and np.array_equal(nbr, gold[key].astype(np.int32)), key
        d = P[nbr] - P[:, None, :]
        assert np.array_equal(d2, (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        assert (np.diff(d2, axis=1) >= 0).all() and list(stats[:3]) == [len(P), 0, 0] and stats[4] == 0
    assert M.knn_exact(a_down, None, 6, 0.1)[3][3] == 22                 # the strays: rings far past the cell walk


def test_restatement_rules_on_small_cases(knn_cases, restated):
    counts = {n: _want(f"n{n}", knn_cases, restated)[1] for n in (0, 1, 2, 6, 7, 8)}
    assert [list(np.unique(c)) for c in counts.values()] == [[], [0], [1], [5], [6], [6]]
    nbr, cnt, d2, stats, ties = _want("lattice_k6", knn_cases, restated)
    P = knn_cases["lattice_k6"][0]
    inner = np.flatnonzero(((P > 0) & (P < 1)).all(axis=1))
    assert ties and len(inner) == 27 and (d2[inner] == 0.0625).all()       # the six face neighbours, ordered by row
    assert (np.diff(nbr[inner], axis=1) > 0).all()
    assert np.array_equal(_want("lattice_negative_k6", knn_cases, restated)[0], nbr)
    nbr, cnt, d2, stats, _ = _want("two_clumps", knn_cases, restated)
    assert (cnt == 6).all() and stats[3] == 40 and (d2[:, 3:] > 15.0).all() and (d2[:, :3] < 0.01).all()
    nbr, cnt, d2, stats, _ = _want("outlier", knn_cases, restated)
    assert 25 < stats[3] <= 28 and (nbr[200] < 200).all() and not (nbr[:200] == 200).any()
    nbr, cnt, d2, stats, _ = _want("non_finite_and_poison", knn_cases, restated)
    assert list(stats[:2]) == [288, 12] and len(nbr) == 300 and np.count_nonzero(cnt == 0) == 12
    nbr, cnt, d2, stats, _ = _want("span_error", knn_cases, restated)
    assert list(stats) == [3, 0, 3, 0, 1, 0, 0, 0] and (nbr == -1).all() and (cnt == 0).all()
    same = [_want(f"a_down_edge{e}", knn_cases, restated) for e in (0.05, 0.1, 0.4)]
    assert all(np.array_equal(s[0], same[0][0]) and np.array_equal(s[2], same[0][2]) for s in same)
    rings = [s[3][3] for s in same]
    assert rings[1] == 22 and rings[0] > rings[1] > rings[2] >= 5          # the strays: far past the cell walk at every edge
    # the fan and the clean-up
    tri = M.fan(np.array([[1, 2, 3], [0, 2, -1], [-1, -1, -1]]), np.array([3, 2, 0]))
    assert tri.tolist() == [[0, 1, 2], [0, 2, 3], [1, 0, 2], [-1, -1, -1], [-1, -1, -1], [-1, -1, -1]]
    kept, st = M.clean_triangles([[0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1], [3, 3, 1], [0, 1, 4], [-1, -1, -1]], 4)
    assert kept.tolist() == [[0, 1, 2], [0, 2, 1]] and list(st) == [7, 2, 1, 2, 2, 0, 0, 0]
    assert M.mean_neighbor_distance(np.array([[4.0, 9.0], [1.0, 0.0], [0.0, 0.0]]), np.array([2, 1, 0])) == (1.75, 2.0)


def test_workspace_size_and_argument_errors_need_no_device():
    from depth_pro import _lib

    lib = _lib.load()
    sizes = [lib.dp_mesh_workspace_size(n, 0) for n in (0, 1, 2048, 2049, 100003, 8294400)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == len(sizes) and all(s % 8 == 0 for s in sizes)
    tsizes = [lib.dp_mesh_workspace_size(0, t) for t in (0, 1, 2048, 2049, 100003, 5 * 721146)]
    assert tsizes[0] == sizes[0] and tsizes == sorted(tsizes) and len(set(tsizes)) == len(tsizes) and all(s % 8 == 0 for s in tsizes)
    assert lib.dp_mesh_workspace_size(-5, -5) == sizes[0]
    for n, t in ((100, 7), (100, 5000), (5000, 100)):
        assert lib.dp_mesh_workspace_size(n, t) >= max(lib.dp_mesh_workspace_size(n, 0), lib.dp_mesh_workspace_size(0, t))
    P, big, ARG, SHAPE = 4096, 1 << 40, 1000, 1001
    f64 = ctypes.c_double

    def knn(points=P, n=8, k=6, edge=0.1, nbr=P, cnt=P, d2=P, stats=P, ws=P, wsb=big):
        return lib.dp_knn_exact(points, None, n, k, f64(edge), nbr, cnt, d2, stats, ws, wsb, None)

    def fan(nbr=P, cnt=P, n=8, k=6, tri=P):
        return lib.dp_mesh_fan(nbr, cnt, None, n, k, tri, None)

    def clean(tri=P, t=8, nv=10, out=P + 4096, t_out=P, stats=P, ws=P, wsb=big):
        return lib.dp_mesh_clean_triangles(tri, None, t, nv, out, t_out, stats, ws, wsb, None)

    def mean(d2=P, cnt=P, n=8, k=6, out=P, ws=P, wsb=big):
        return lib.dp_mesh_mean_distance(d2, cnt, None, n, k, out, ws, wsb, None)

    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert knn(edge=bad) == SHAPE, bad
    for k in (0, -3, 65):
        assert knn(k=k) == SHAPE and fan(k=k) == SHAPE and mean(k=k) == SHAPE, k
    assert knn(n=-1) == SHAPE and fan(n=-1) == SHAPE and clean(t=-1) == SHAPE and clean(nv=-1) == SHAPE and mean(n=-1) == SHAPE
    assert fan(n=(1 << 31) // 3 // 5 + 1, k=6) == SHAPE and fan(n=(1 << 31) - 1, k=2) == SHAPE
    short = lib.dp_mesh_workspace_size(8, 0) - 1
    for kw in ({"points": None}, {"nbr": None}, {"cnt": None}, {"stats": None}, {"ws": None}, {"ws": P + 4}, {"wsb": short}):
        assert knn(**kw) == ARG, kw
    for kw in ({"nbr": None}, {"cnt": None}, {"tri": None}):
        assert fan(**kw) == ARG, kw
    for kw in ({"tri": None}, {"out": None}, {"out": P}, {"t_out": None}, {"stats": None}, {"ws": None}, {"ws": P + 4},
               {"wsb": lib.dp_mesh_workspace_size(0, 8) - 1}):
        assert clean(**kw) == ARG, kw
    for kw in ({"d2": None}, {"cnt": None}, {"out": None}, {"ws": None}, {"wsb": short}):
        assert mean(**kw) == ARG, kw


def test_python_layer_refuses_bad_arguments_and_host_tensors():
    import torch

    from depth_pro import _lib
    from depth_pro import pointcloud as PC

    assert len(PC.KNN_EXACT_STATS) == len(PC.TRIANGLE_STATS) == 8
    assert PC.KNN_EXACT_STATS[:5] == M.KNN_STATS[:5] and PC.TRIANGLE_STATS[:6] == M.TRI_STATS[:6]
    pts = torch.zeros(4, 3, dtype=torch.float64)
    tri = torch.zeros(4, 3, dtype=torch.int32)
    for call in (lambda: PC.knn_exact(pts), lambda: PC.simple_mesh(pts), lambda: PC.mean_neighbor_distance(pts),
                 lambda: PC.clean_triangles(tri, 4), lambda: PC.fan_triangles(tri, tri[:, 0].contiguous()),
                 lambda: PC.triangulate(pts)):
        with pytest.raises(_lib.DPError):
            call()
    for call in (lambda: PC.knn_exact(pts, k=0), lambda: PC.knn_exact(pts, k=65), lambda: PC.knn_exact(pts, cell_edge=0.0),
                 lambda: PC.knn_exact(pts, cell_edge=float("nan")), lambda: PC.triangulate(pts, neighbors=1),
                 lambda: PC.clean_triangles(tri, -1), lambda: PC.clean_triangles(tri.to(torch.int64), 4),
                 lambda: PC.simple_mesh(pts, voxel_size=0.0)):
        with pytest.raises(ValueError):
            call()


def _records(pts, cols, tri):
    v = np.empty(len(pts), dtype=[("p", "<f8", 3), ("c", "u1", 3)] if cols is not None else [("p", "<f8", 3)])
    v["p"] = pts
    if cols is not None:
        v["c"] = cols
    f = np.empty(len(tri), dtype=[("k", "u1"), ("v", "<u4", 3)])
    f["k"], f["v"] = 3, tri
    return v.view(np.uint8).reshape(len(pts), -1), f.view(np.uint8).reshape(len(tri), 13)


def test_mesh_ply_round_trips_byte_exact(tmp_path):
    from depth_pro import pointcloud as PC

    g = np.random.default_rng(5)
    pts = g.normal(size=(37, 3))
    pts[3] = [0.0, -0.0, np.nan]
    cols = g.integers(0, 256, (37, 3), dtype=np.uint8)
    tri = g.integers(0, 37, (50, 3)).astype(np.uint32)
    for c in (cols, None):
        a = PC.write_mesh_ply(str(tmp_path / "a"), *_records(pts, c, tri))
        assert a.endswith("a.ply")
        p2, c2, t2 = PC.read_mesh_ply(a)
        assert p2.tobytes() == pts.tobytes() and np.array_equal(t2, tri) and t2.dtype == np.uint32
        assert (c2 is None) if c is None else np.array_equal(c2, c)
        b = PC.write_mesh_ply(str(tmp_path / "b.ply"), *_records(p2, c2, t2))
        raw = open(a, "rb").read()
        assert raw == open(b, "rb").read()
        head, body = raw.split(b"end_header\n", 1)
        want = ["ply", "format binary_little_endian 1.0", "element vertex 37"] + [f"property double {k}" for k in "xyz"]
        want += [f"property uchar {k}" for k in ("red", "green", "blue")] if c is not None else []
        want += ["element face 50", "property list uchar uint vertex_indices"]
        assert head.decode("ascii").splitlines() == want and len(body) == 37 * (27 if c is not None else 24) + 50 * 13
    e = PC.write_mesh_ply(str(tmp_path / "e.ply"), np.zeros((0, 27), np.uint8), np.zeros((0, 13), np.uint8))
    assert [x.shape for x in PC.read_mesh_ply(e)] == [(0, 3), (0, 3), (0, 3)]
    with pytest.raises(ValueError):
        PC.read_mesh_ply(PC.write_ply(str(tmp_path / "plain.ply"), pts, cols))
    with pytest.raises(ValueError):
        PC.write_mesh_ply(str(tmp_path / "bad.ply"), np.zeros((1, 27), np.uint8), np.zeros((1, 12), np.uint8))
    # the vertex element reads as a plain cloud
    assert PC.read_ply(a.replace("a.ply", "b.ply"))[0].tobytes() == pts.tobytes()


def test_cli_stage_table_and_resume_know_the_mesh_files(monkeypatch, tmp_path):
    import generate_depth_maps as G

    got = G.resolve_stages(output_dir="OUT", simple_mesh=True)
    assert list(got) == ["cloud", "ground", "clean", "mesh", "trimesh"] and got["trimesh"] == {"neighbors": 6}
    assert got["mesh"] == {"voxel_size": 0.05, "max_nn": 30}
    assert G.resolve_stages(output_dir="OUT", simple_mesh=True, mesh_neighbors=12.0)["trimesh"] == {"neighbors": 12}
    assert "trimesh" not in G.resolve_stages(output_dir="OUT", mesh_points=True, mesh_neighbors=1)      # off: not looked at
    for bad in (1, 0, 65):
        with pytest.raises(ValueError, match="--mesh_neighbors must be in"):
            G.batch_generate_depth_maps(str(tmp_path), str(tmp_path / "o"), simple_mesh=True, mesh_neighbors=bad)
    st = {s.name: s for s in G.STAGES}["trimesh"]
    assert st.implies == "mesh" and st.suffixes == ("_mesh.ply", "_mesh.json")
    # main(): without the new flags no new keyword; with them exactly those
    seen = []
    monkeypatch.setattr(G, "batch_generate_depth_maps", lambda *a, **kw: seen.append(kw) or 0)
    monkeypatch.setattr(G, "_model", lambda *a, **k: pytest.fail("the model was loaded"))
    base = ["generate_depth_maps.py", "--input_dir", str(tmp_path)]
    monkeypatch.setattr(sys, "argv", base)
    G.main()
    monkeypatch.setattr(sys, "argv", base + ["--simple_mesh", "--mesh_neighbors", "9"])
    G.main()
    assert "simple_mesh" not in seen[0] and "mesh_neighbors" not in seen[0]
    assert {k: v for k, v in seen[1].items() if k not in seen[0]} == {"simple_mesh": True, "mesh_neighbors": 9}
    assert {k: v for k, v in seen[1].items() if k in seen[0]} == seen[0]
    for extra in (["--simple_mesh", "--mesh_neighbors", "1"], ["--mesh_neighbors", "1"], ["--simple_mesh", "--mesh_neighbors", "65"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        with pytest.raises(SystemExit) as e:
            G.main()
        assert e.value.code == 2, extra
    # --resume
    frames = [str(tmp_path / f"f{k}.png") for k in range(3)]
    for k in (0, 1):
        for s in ("depth.png", "clean.ply", "oriented.ply", "oriented.json", "mesh.ply"):
            (tmp_path / f"f{k}_{s}").write_bytes(b"")
    (tmp_path / "f0_mesh.json").write_bytes(b"")                     # f1's json is missing: not done
    assert G.plan_frames(frames, str(tmp_path), 1, 0, True, cleaned=True, oriented=True) == [2]
    assert G.plan_frames(frames, str(tmp_path), 1, 0, True, cleaned=True, oriented=True, meshed=True) == [1, 2]
    assert G.plan_frames(frames, str(tmp_path), 1, 0, True, stages=G.resolve_stages(simple_mesh=True)) == [1, 2]
    assert G.plan_frames(frames, str(tmp_path), 1, 0, False, meshed=True) == [0, 1, 2]


# ---- GPU ------------------------------------------------------------------------------------------------

def _dev(a, cuda):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _knn(pts, count, k, edge, cuda):
    """dp_knn_exact through ctypes on outputs filled with a sentinel -> (nbr, cnt, d2, stats), whole buffers."""
    import torch

    from depth_pro import _lib

    lib = _lib.load()
    n = len(pts)
    p = _dev(np.asarray(pts, dtype=np.float64).reshape(n, 3), cuda)
    nbr = torch.full((n, k), SENTINEL, dtype=torch.int32, device=cuda)
    cnt = torch.full((n,), SENTINEL, dtype=torch.int32, device=cuda)
    d2 = torch.full((n, k), float(SENTINEL), dtype=torch.float64, device=cuda)
    stats = torch.full((8,), float(SENTINEL), dtype=torch.float64, device=cuda)
    ws = torch.empty(int(lib.dp_mesh_workspace_size(n, 0)), dtype=torch.uint8, device=cuda)
    c = None if count is None else torch.tensor([count], dtype=torch.int32, device=cuda)
    _lib.check(lib.dp_knn_exact(p.data_ptr(), None if c is None else c.data_ptr(), n, k, float(edge), nbr.data_ptr(),
                                cnt.data_ptr(), d2.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(),
                                torch.cuda.current_stream(cuda).cuda_stream), "dp_knn_exact")
    torch.cuda.synchronize()
    return nbr.cpu().numpy(), cnt.cpu().numpy(), d2.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", KNN_NAMES)
def test_knn_exact(name, knn_cases, restated, cuda):
    """Fails on the parent commit: dp_knn_exact does not exist there."""
    pts, count, k, edge = knn_cases[name]
    wnbr, wcnt, wd2, wstats, _ = _want(name, knn_cases, restated)
    nbr, cnt, d2, stats = _knn(pts, count, k, edge, cuda)
    n = len(wnbr)
    print(f"{name}: n={n} k={k} stats {stats} (want {wstats}); rows that differ {np.count_nonzero((nbr[:n] != wnbr).any(axis=1))}")
    assert np.array_equal(cnt[:n], wcnt) and np.array_equal(nbr[:n], wnbr)
    listed = np.arange(k)[None, :] < wcnt[:, None]
    assert np.array_equal(d2[:n][listed].view(np.int64), wd2[listed].view(np.int64))          # bit for bit
    assert (d2[:n][~listed] == SENTINEL).all()                                               # past the count: not written
    assert (nbr[n:] == SENTINEL).all() and (cnt[n:] == SENTINEL).all() and (d2[n:] == SENTINEL).all()
    assert np.array_equal(stats, wstats)


@pytest.mark.gpu
def test_cell_edge_never_changes_the_lists(knn_cases, a_down, cuda):
    from depth_pro import pointcloud as PC

    base = _knn(a_down, None, 6, 0.1, cuda)
    for e in (0.05, 0.4, 3.0, 0.013):                      # 0.013: below the spacing, nearly every row takes every point
        got = _knn(a_down, None, 6, e, cuda)
        assert all(np.array_equal(x, y) for x, y in zip(got[:3], base[:3])), e
    nbr, cnt, d2, stats = PC.knn_exact(_dev(a_down, cuda), None, 6, 0.1)
    assert np.array_equal(nbr.cpu().numpy(), base[0]) and np.array_equal(d2.cpu().numpy(), base[2])
    assert np.array_equal(stats.cpu().numpy(), base[3]) and np.array_equal(cnt.cpu().numpy(), base[1])


@pytest.mark.gpu
def test_mean_neighbor_distance(a_down, knn_cases, restated, cuda):
    from depth_pro import pointcloud as PC

    for pts, count, k in ((a_down, None, 20), (a_down, 1000, 5), (knn_cases["n1"][0], None, 20), (a_down[:0], None, 20)):
        _, cnt, d2, _, _ = M.knn_exact(pts, count, k, 0.1)
        want, rows = M.mean_neighbor_distance(d2, cnt)
        got = float(PC.mean_neighbor_distance(_dev(pts.reshape(-1, 3), cuda), count, k, 0.1).item())
        print(f"n={len(cnt)} k={k}: mean {got!r} (want {want!r}), relative difference {abs(got - want) / max(want, 1e-300):.3e}, "
              f"bound {(k + 1) * 2.0 ** -52:.3e}")
        assert got == want, (got, want)


def _clean(tri, nv, count, cuda):
    """dp_mesh_clean_triangles through ctypes on an output filled with a sentinel -> (tri_out whole, t_out, stats)."""
    import torch

    from depth_pro import _lib

    lib = _lib.load()
    tri = np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    t = len(tri)
    src = _dev(np.r_[tri, np.full((1, 3), 5, np.int32)], cuda)                  # one spare row: never a null pointer
    out = torch.full((t + 1, 3), SENTINEL, dtype=torch.int32, device=cuda)
    t_out = torch.full((1,), SENTINEL, dtype=torch.int32, device=cuda)
    stats = torch.full((8,), float(SENTINEL), dtype=torch.float64, device=cuda)
    ws = torch.empty(int(lib.dp_mesh_workspace_size(0, t)), dtype=torch.uint8, device=cuda)
    c = None if count is None else torch.tensor([count], dtype=torch.int32, device=cuda)
    _lib.check(lib.dp_mesh_clean_triangles(src.data_ptr(), None if c is None else c.data_ptr(), t, nv,
                                           out.data_ptr(), t_out.data_ptr(), stats.data_ptr(), ws.data_ptr(),
                                           ws.numel(), torch.cuda.current_stream(cuda).cuda_stream), "dp_mesh_clean_triangles")
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(t_out.item()), stats.cpu().numpy()


def _tri_cases():
    g = np.random.default_rng(31)
    big = (1 << 21) + 3
    rot = lambda t, s: np.roll(t, -s, axis=-1)                                                   # noqa: E731
    uniq = np.array([[3 * i, 3 * i + 1, 3 * i + 2] for i in range(300)])
    cases = {
        "rotations_and_mirror": ([[5, 1, 3], [1, 3, 5], [3, 5, 1], [5, 3, 1]], 6, None),
        "degenerate": ([[2, 2, 4], [2, 4, 2], [2, 4, 4], [1, 2, 3]], 5, None),
        "invalid": ([[-1, -1, -1], [0, 1, 7], [0, 1, 6], [-1, 2, 3], [7, 7, 7], [0, -2, 1]], 7, None),
        "all_duplicates": ([[4, 9, 2], [9, 2, 4], [2, 4, 9]] * 100, 10, None),
        "no_duplicates": (uniq, 900, None),
        "straddle_2_21": ([[1, 3, 2], [1, 3, big - 1], [(1 << 21) - 1, 1 << 21, big - 2], [big - 2, (1 << 21) - 1, 1 << 21],
                           [1 << 21, 0, 0], [0, 1 << 21, 1], [0, 0, 1], [1, 0, 1 << 21], [1, 3, big], [big - 1, 1, 3]], big, None),
        "copies_in_other_blocks": (np.r_[uniq, uniq[::-1] + 0, rot(uniq[:200], 1), rot(uniq[100:], 2), uniq[:, ::-1]], 900, None),
        "count_and_poison": (np.r_[uniq[:50], rot(uniq[:50], 1), g.integers(-5, 900, (40, 3))], 900, 100),
    }
    for t in (0, 1, 255, 256, 257, 65537):
        tri = g.integers(-1, 42, (t, 3))                    # 41^3 forms and their rotations: copies, degenerates, invalids
        cases[f"t{t}"] = (tri, 41, None)
    return cases


TRI_CASES = _tri_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TRI_CASES))
def test_clean_triangles(name, cuda):
    """Fails on the parent commit: dp_mesh_clean_triangles does not exist there."""
    tri, nv, count = TRI_CASES[name]
    want, wstats = M.clean_triangles(tri, nv, count)
    out, t_out, stats = _clean(tri, nv, count, cuda)
    print(f"{name}: stats {stats} (want {wstats})")
    assert t_out == len(want) and np.array_equal(out[:t_out], want) and (out[t_out:] == SENTINEL).all()
    assert np.array_equal(stats, wstats) and stats[0] == stats[1:5].sum()
    if name == "rotations_and_mirror":
        assert out[:2].tolist() == [[5, 1, 3], [5, 3, 1]]                    # the first of them as it came
    if name == "straddle_2_21":
        assert out[:4].tolist() == [list(TRI_CASES[name][0][i]) for i in (0, 1, 2, 5)] and list(stats[1:5]) == [1, 2, 3, 4]
    if name == "t65537":
        assert stats[3] > 1000 and stats[2] > 1000 and stats[1] > 1000 and t_out > 10000


@pytest.mark.gpu
def test_fan_and_python_wrappers(knn_cases, restated, cuda):
    import torch

    from depth_pro import pointcloud as PC

    for name in ("n2", "n7", "lattice_k20", "non_finite_and_poison"):
        pts, count, k, edge = knn_cases[name]
        nbr, cnt, _, _ = PC.knn_exact(_dev(pts, cuda), count, k, edge)
        tri = torch.full((len(pts) * (k - 1), 3), SENTINEL, dtype=torch.int32, device=cuda)
        got = PC.fan_triangles(nbr, cnt, count)
        n = len(pts) if count is None else count
        want = M.fan(_want(name, knn_cases, restated)[0], _want(name, knn_cases, restated)[1])
        assert np.array_equal(got.cpu().numpy()[:n * (k - 1)], want), name
        # the slots of rows past the count are not written
        from depth_pro import _lib
        c = None if count is None else torch.tensor([count], dtype=torch.int32, device=cuda)
        _lib.check(_lib.load().dp_mesh_fan(nbr.data_ptr(), cnt.data_ptr(), None if c is None else c.data_ptr(), len(pts), k,
                                           tri.data_ptr(), torch.cuda.current_stream(cuda).cuda_stream), "dp_mesh_fan")
        assert (tri.cpu().numpy()[n * (k - 1):] == SENTINEL).all() and np.array_equal(tri.cpu().numpy()[:n * (k - 1)], want)
        out, n_out, stats = PC.clean_triangles(got, len(pts), n * (k - 1))
        wtri, wst = M.clean_triangles(want, len(pts))
        assert np.array_equal(out.cpu().numpy()[:int(n_out.item())], wtri) and np.array_equal(stats.cpu().numpy(), wst)
    one = PC.knn_exact(_dev(knn_cases["n8"][0], cuda), None, 1, 0.1)
    assert PC.fan_triangles(one[0], one[1]).shape == (0, 3)


@pytest.mark.gpu
def test_simple_mesh_end_to_end(cloud_a, tmp_path, cuda):
    """simple_mesh on cloud A: the voxel grid's vertices, and the restatement's triangles over them, one for one."""
    from depth_pro import pointcloud as PC

    pts, cols = cloud_a
    out, cout, n_out, tri, n_tri, stats = PC.simple_mesh(_dev(pts, cuda), _dev(cols, cuda), None, VOXEL, 6)
    n, t = int(n_out.item()), int(n_tri.item())
    vox = PC.voxel_downsample(_dev(pts, cuda), _dev(cols, cuda), None, VOXEL)
    verts, vcols = out.cpu().numpy()[:n], cout.cpu().numpy()[:n]
    assert n == 1664 and np.array_equal(verts, vox[0].cpu().numpy()[:n]) and np.array_equal(vcols, vox[1].cpu().numpy()[:n])
    want, kst, tst = M.simple_mesh(verts, 6, 2 * VOXEL)
    got = tri.cpu().numpy()[:t]
    print(f"vertices {n}, triangles {t} of {5 * n} (want {len(want)}); knn {stats['knn'].cpu().numpy()} triangles "
          f"{stats['triangles'].cpu().numpy()}")
    assert t == len(want) and np.array_equal(got, want)
    assert np.array_equal(stats["knn"].cpu().numpy(), kst) and stats["voxel"].cpu().numpy()[2] == n
    # the triangle stats count the fan's slots of every buffer row the voxel count makes live
    assert np.array_equal(stats["triangles"].cpu().numpy(), tst) and tst[0] == 5 * n and tst[4] == t
    assert ((got >= 0) & (got < n)).all() and (got[:, 0] != got[:, 1]).all() and (got[:, 1] != got[:, 2]).all() and \
        (got[:, 0] != got[:, 2]).all()
    assert len({M.canonical(x) for x in got}) == t
    vrec, frec = PC.mesh_ply_records_async(out, cout, tri)
    path = PC.write_mesh_ply(str(tmp_path / "m.ply"), vrec.cpu().numpy()[:n], frec.cpu().numpy()[:t])
    p2, c2, t2 = PC.read_mesh_ply(path)
    assert p2.tobytes() == verts.tobytes() and np.array_equal(c2, vcols) and np.array_equal(t2, got.astype(np.uint32))
    again = PC.write_mesh_ply(str(tmp_path / "m2.ply"), *_records(p2, c2, t2))
    assert open(path, "rb").read() == open(again, "rb").read()
    # without colours, and an empty cloud
    bare = PC.simple_mesh(_dev(pts, cuda), None, None, VOXEL, 6)
    assert bare[1] is None and np.array_equal(bare[3].cpu().numpy()[:t], got)
    assert PC.mesh_ply_records_async(bare[0], None, bare[3])[0].shape == (len(pts), 24)
    empty = PC.simple_mesh(_dev(np.zeros((0, 3)), cuda))
    assert int(empty[2].item()) == 0 and int(empty[4].item()) == 0


@pytest.mark.gpu
def test_loop_simple_mesh(tmp_path, cuda):
    """--simple_mesh adds {base}_mesh.ply and {base}_mesh.json to the --mesh_points run's files; the mesh's vertices are
    the oriented cloud's, its faces the restatement's over them."""
    import generate_depth_maps as G
    from depth_pro import pointcloud as PC
    from test_normals import _run_loop

    out = tmp_path / "mesh"
    kw = dict(clean_pointcloud=True, stray_radius=0.25, stray_neighbors=12, mesh_points=True, voxel_size=0.1, normals_max_nn=20)
    _run_loop(tmp_path, cuda, out, frames=3, simple_mesh=True, mesh_neighbors=5, **kw)
    names = [f"output_{k:04d}_{s}" for k in range(3) for s in ("clean.ply", "depth.png", "oriented.ply", "oriented.json")]
    assert sorted(os.listdir(out)) == sorted(names + ["ground.json"] + [f"output_{k:04d}_mesh.{e}" for k in range(3)
                                                                        for e in ("ply", "json")])
    js = json.load(open(out / "output_0000_mesh.json"))
    assert js["parameters"] == {"voxel_size": 0.1, "neighbors": 5, "cell_edge": 0.2, "method": "simple"}
    pts, cols, faces = PC.read_mesh_ply(str(out / "output_0000_mesh.ply"))
    head = open(out / "output_0000_mesh.ply", "rb").read().split(b"end_header\n")[0].decode("ascii")
    assert f"element vertex {js['vertices']}\n" in head and f"element face {js['triangles']}\n" in head
    assert len(pts) == js["vertices"] == js["knn_stats"]["finite"] > 10 and len(faces) == js["triangles"] > 10
    assert js["triangle_stats"]["kept"] == len(faces) and js["triangle_stats"]["input"] == 4 * len(pts)
    assert js["knn_stats"]["error"] == js["triangle_stats"]["error"] == 0 and set(js["knn_stats"]) == set(PC.KNN_EXACT_STATS)
    op, _, oc = PC.read_ply_normals(str(out / "output_0000_oriented.ply"))
    assert pts.tobytes() == op.tobytes() and np.array_equal(cols, oc)
    want, kst, tst = M.simple_mesh(pts, 5, 0.2)
    assert np.array_equal(faces, want.astype(np.uint32)) and js["knn_stats"]["max_ring"] == kst[3]
    _, cnt, d2, _, _ = M.knn_exact(pts, None, 20, 0.2)
    mean = M.mean_neighbor_distance(d2, cnt)[0]
    assert js["mean_neighbor_distance"] == mean and js["ball_pivoting_radii"] == [f * mean for f in (2, 4, 8, 16)]
    for k in (1, 2):                        # the fixture's frames are one picture: every frame's files are frame 0's
        for e in ("ply", "json"):
            assert open(out / f"output_{k:04d}_mesh.{e}", "rb").read() == open(out / f"output_0000_mesh.{e}", "rb").read(), (k, e)
    src = sorted(str(p) for p in (tmp_path / "frames").glob("*.png"))
    on = dict(cleaned=True, oriented=True, meshed=True)
    assert G.plan_frames(src, str(out), 1, 0, True, **on) == []
    for k, s in ((1, "_mesh.ply"), (2, "_mesh.json")):
        os.rename(out / f"output_{k:04d}{s}", out / "away")
        assert G.plan_frames(src, str(out), 1, 0, True, **on) == [k]
        os.rename(out / "away", out / f"output_{k:04d}{s}")
    # --resume skips every frame: nothing is processed, nothing changes
    before = {f: os.path.getmtime(out / f) for f in os.listdir(out)}
    assert G.batch_generate_depth_maps(str(tmp_path / "frames"), str(out), pattern="output_*.png", resume=True, simple_mesh=True,
                                       mesh_neighbors=5, model=(None, None), **kw) == 0
    assert before == {f: os.path.getmtime(out / f) for f in os.listdir(out)}
