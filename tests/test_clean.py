"""Cleaned point clouds (ABI 16, csrc/dp_clean.hip): the stable radix sort, stray-point removal, shadow
columns, compaction, `clean_pointcloud` and the loop's --clean_pointcloud.

References: tests/golden/golden_clean.npz holds the masks of the reference's own `remove_stray_points`
and `clean_shadows` (tests/golden/make_golden_clean.py); tests/clean_numpy.py restates them in numpy /
scipy.  Everything here is compared exactly: the kernels do the restatement's fp64 operations in its
order, and the fixture keeps every decision at least 1e-9 away from its threshold.
"""

import ctypes
import os
import sys

import numpy as np
import pytest

import clean_numpy as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "golden_clean.npz"))


@pytest.fixture(scope="module")
def restated(gold):
    """The restatement on the fixture scenes, computed once."""
    return {str(s): C.clean(gold[f"{s}_points"], gold[f"{s}_colors"]) for s in gold["scenes"]}


# ---- CPU ----------------------------------------------------------------------------------------------

def test_restatement_reproduces_the_reference_masks(gold, restated):
    for s in gold["scenes"]:
        _, _, k1, k2, s1, s2 = restated[str(s)]
        assert np.array_equal(k1, gold[f"{s}_stray_keep"]) and np.array_equal(k2, gold[f"{s}_shadow_keep"])
        kept, total, removed, total1 = gold[f"{s}_printed"]
        assert (s1[2], s1[0] + s1[1], s2[5], s2[0]) == (kept, total, removed, total1)
        assert s2[6] == gold[f"{s}_cell"]


@pytest.mark.parametrize("flag,value", [("--stray_radius", "0"), ("--stray_radius", "-0.1"), ("--stray_radius", "nan"),
                                        ("--stray_radius", "inf"), ("--stray_neighbors", "0"),
                                        ("--stray_neighbors", "-3")])
def test_cli_refuses_stray_values(monkeypatch, flag, value, tmp_path):
    import generate_depth_maps as G

    monkeypatch.setattr(sys, "argv", ["generate_depth_maps.py", "--input_dir", str(tmp_path), "--clean_pointcloud",
                                      flag, value])
    with pytest.raises(SystemExit) as e:
        G.main()
    assert e.value.code == 2
    kw = {"stray_radius": float(value)} if flag == "--stray_radius" else {"stray_neighbors": int(value)}
    with pytest.raises(ValueError):
        G.batch_generate_depth_maps(str(tmp_path), str(tmp_path / "o"), clean_pointcloud=True, **kw)


def test_resume_looks_for_the_clean_file(tmp_path):
    import generate_depth_maps as G

    frames = [str(tmp_path / f"f{k}.png") for k in range(3)]
    assert G.cloud_name(frames[0]) == "f0_points.ply" and G.cloud_name(frames[0], True) == "f0_clean.ply"
    for k in (0, 1):
        (tmp_path / f"f{k}_depth.png").write_bytes(b"")
    (tmp_path / "f0_clean.ply").write_bytes(b"")
    (tmp_path / "f1_points.ply").write_bytes(b"")
    assert G.plan_frames(frames, str(tmp_path), 1, 0, True) == [2]
    assert G.plan_frames(frames, str(tmp_path), 1, 0, True, cleaned=True) == [1, 2]


def test_workspace_size_and_argument_errors_need_no_device():
    from depth_pro import _lib

    lib = _lib.load()
    sizes = [lib.dp_clean_workspace_size(n) for n in (0, 1, 4096, 4097, 8294400)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[4] >= 48 * 8294400
    assert lib.dp_clean_workspace_size(-5) == sizes[0]
    P, big, ARG, SHAPE = 4096, 1 << 40, 1000, 1001
    f64 = ctypes.c_double
    assert lib.dp_sort_pairs(P, P, None, 8, 9, 8, P, big, None) == SHAPE            # bit_lo > bit_hi
    assert lib.dp_sort_pairs(P, P, None, 8, 0, 65, P, big, None) == SHAPE
    assert lib.dp_sort_pairs(P, P, None, -1, 0, 64, P, big, None) == SHAPE
    assert lib.dp_sort_pairs(None, P, None, 8, 0, 64, P, big, None) == ARG
    assert lib.dp_sort_pairs(P, P, None, 8, 0, 64, P, 16, None) == ARG              # workspace too small
    for r in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.dp_clean_stray(P, None, 8, f64(r), 20, P, P, P, big, None) == SHAPE
    assert lib.dp_clean_stray(P, None, 8, f64(0.1), 0, P, P, P, big, None) == SHAPE
    assert lib.dp_clean_stray(P, None, 8, f64(0.1), 20, None, P, P, big, None) == ARG
    assert lib.dp_clean_stray(P, None, 8, f64(0.1), 20, P, P, P, 16, None) == ARG
    assert lib.dp_clean_shadows(P, None, 8, f64(0.1), f64(75), 0, P, P, P, big, None) == SHAPE
    assert lib.dp_clean_shadows(P, None, 8, f64(float("nan")), f64(75), 3, P, P, P, big, None) == SHAPE
    assert lib.dp_clean_shadows(P, None, 8, f64(0.1), f64(75), 3, P, None, P, big, None) == ARG
    assert lib.dp_compact_points(P, None, P, None, -1, P, None, P, P, big, None) == SHAPE
    assert lib.dp_compact_points(P, P, P, None, 8, P, None, P, P, big, None) == ARG   # colours without an output
    assert lib.dp_compact_points(P, None, P, None, 8, P, None, None, P, big, None) == ARG


def test_python_layer_refuses_bad_arguments_and_host_tensors():
    import torch

    from depth_pro import _lib
    from depth_pro import pointcloud as PC

    pts = torch.zeros(4, 3, dtype=torch.float64)
    for fn in (PC.remove_stray_points, PC.clean_shadows, PC.clean_pointcloud):
        with pytest.raises(_lib.DPError):
            fn(pts)
    with pytest.raises(ValueError):
        PC.stray_mask(pts, radius=0.0)
    with pytest.raises(ValueError):
        PC.stray_mask(pts, nb_points=0)
    with pytest.raises(_lib.DPError):
        PC.sort_pairs(torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int32))


# ---- GPU: the sort ----------------------------------------------------------------------------------------

def _key_sets(n, rng):
    rnd = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    base = np.uint64(0x0123456789ABCDEF)
    return {
        "random": (rnd, 0, 64),
        "equal": (np.full(n, base), 0, 64),
        "top_byte": ((base & np.uint64(0x00FFFFFFFFFFFFFF)) | (rng.integers(0, 256, n).astype(np.uint64) << np.uint64(56)), 0, 64),
        "bottom_byte": ((base & np.uint64(0xFFFFFFFFFFFFFF00)) | rng.integers(0, 256, n).astype(np.uint64), 0, 64),
        "63_bits": (rnd, 0, 63),
        # bits 13..26 sorted; the bits below and above differ too and must not matter
        "partial": (rnd, 13, 27),
        "partial_few_values": (rng.integers(0, 2 ** 64, 7, dtype=np.uint64)[rng.integers(0, 7, n)], 21, 30),
        "one_bit": (rnd, 40, 41),
        "no_bits": (rnd, 17, 17),
    }


def _field(keys, lo, hi):
    if hi == lo:
        return np.zeros(len(keys), dtype=np.uint64)
    k = keys >> np.uint64(lo)
    return k if hi - lo == 64 else k & np.uint64((1 << (hi - lo)) - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 4097, 100003])
def test_sort_pairs_equals_stable_argsort(n, cuda):
    import torch

    from depth_pro import pointcloud as PC

    rng = np.random.default_rng(n)
    n_max = n + 37                                   # the live count comes from the device and is smaller than n_max
    count = torch.tensor([n], dtype=torch.int32, device=cuda)
    for name, (keys, lo, hi) in _key_sets(n_max, rng).items():
        vals = rng.integers(0, 2 ** 32, n_max, dtype=np.uint64).astype(np.uint32)
        k, v = PC.sort_pairs(torch.from_numpy(keys.view(np.int64)).to(cuda), torch.from_numpy(vals.view(np.int32)).to(cuda),
                             count, lo, hi)
        k, v = k.cpu().numpy().view(np.uint64), v.cpu().numpy().view(np.uint32)
        order = np.argsort(_field(keys[:n], lo, hi), kind="stable")
        assert np.array_equal(k[:n], keys[:n][order]), (name, n)
        assert np.array_equal(v[:n], vals[:n][order]), (name, n)
        assert np.array_equal(k[n:], keys[n:]) and np.array_equal(v[n:], vals[n:]), (name, n, "past the live count")


@pytest.mark.gpu
def test_two_sorts_make_a_lexicographic_sort(cuda):
    """Low field first, then the high field: stable passes give np.lexsort's order."""
    import torch

    from depth_pro import pointcloud as PC

    rng = np.random.default_rng(5)
    n = 20011
    keys = (rng.integers(0, 9, n).astype(np.uint64) << np.uint64(16)) | rng.integers(0, 50, n).astype(np.uint64)
    vals = np.arange(n, dtype=np.int32)
    k, v = PC.sort_pairs(torch.from_numpy(keys.view(np.int64)).to(cuda), torch.from_numpy(vals).to(cuda), None, 0, 16)
    k, v = PC.sort_pairs(k, v, None, 16, 32)
    want = np.lexsort((vals, keys & np.uint64(0xFFFF), keys >> np.uint64(16)))
    assert np.array_equal(v.cpu().numpy(), vals[want])
    assert np.array_equal(k.cpu().numpy().view(np.uint64), keys[want])


# ---- GPU: stray points ---------------------------------------------------------------------------------------

def _check_stray(pts, cuda, nb=20, radius=0.1, count=None):
    import torch

    from depth_pro import pointcloud as PC

    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    live = len(pts) if count is None else count
    keep, stats = PC.stray_mask(torch.from_numpy(pts).to(cuda), count, nb, radius)
    want, wstats = C.stray_mask(pts[:live], nb, radius)
    got = keep.cpu().numpy()[:live].astype(bool)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(stats.cpu().numpy(), wstats)
    return want


@pytest.mark.gpu
def test_stray_fixture(gold, cuda):
    for s in gold["scenes"]:
        want = _check_stray(gold[f"{s}_points"], cuda)
        assert np.array_equal(want, gold[f"{s}_stray_keep"])


@pytest.mark.gpu
def test_stray_lattice_on_cell_boundaries(cuda):
    """A lattice of pitch radius / 2 at negative and positive coordinates: points sit on cell borders and many
    pairs are at the radius itself, where only the fp64 rounding of the formula decides."""
    ax = np.arange(-10, 11) * 0.05
    pts = np.stack(np.meshgrid(ax, ax[:9] - 3.0, ax[:7], indexing="ij"), axis=-1).reshape(-1, 3)
    for nb in (20, 33, 27):               # 27 lattice offsets lie inside the radius, 6 more at it
        want = _check_stray(pts, cuda, nb=nb)
    assert 0 < want.sum() < len(want)
    _check_stray(pts * 2.0, cuda, nb=7)                      # pitch == radius: every axis neighbour at the radius


@pytest.mark.gpu
def test_stray_cluster_sizes_and_dense_cell(cuda):
    rng = np.random.default_rng(11)
    parts = [c + rng.uniform(-0.01, 0.01, (k, 3)) for k, c in ((19, (0, 0, 0)), (20, (5, 0, 0)), (21, (0, 5, -3)))]
    want = _check_stray(np.concatenate(parts), cuda)
    assert want.tolist() == [False] * 19 + [True] * 41
    blob = 0.01 * rng.standard_normal((5000, 3)) + 0.5       # one cell, the early exit after 20 tests
    assert _check_stray(np.concatenate([blob, [[3.0, 3.0, 3.0]]]), cuda).sum() == 5000
    far = np.concatenate([0.02 * rng.standard_normal((300, 3)), 0.02 * rng.standard_normal((25, 3)) + [1.0e4, -1.0e4, 1.0e4]])
    assert _check_stray(far, cuda).sum() > 300               # two clusters 10 km apart: 1e5 cells per axis
    dup = np.repeat(rng.uniform(-1, 1, (40, 3)), rng.integers(1, 40, 40), axis=0)
    want = _check_stray(dup, cuda)
    assert 0 < want.sum() < len(want)


@pytest.mark.gpu
def test_stray_edge_cases(cuda):
    rng = np.random.default_rng(12)
    pts = 0.05 * rng.standard_normal((3000, 3))
    bad = pts.copy()
    bad[::7, 0] = np.nan
    bad[3::11, 2] = np.inf
    bad[5::13, 1] = -np.inf
    want = _check_stray(bad, cuda)
    assert not want[::7].any() and want.any()
    _check_stray(np.zeros((0, 3)), cuda)
    _check_stray(np.array([[1.0, 2.0, 3.0]]), cuda)
    assert _check_stray(np.array([[1.0, 2.0, 3.0]]), cuda, nb=1).all()
    assert _check_stray(bad, cuda, nb=1).sum() == np.isfinite(bad).all(axis=1).sum()     # nb_points = 1: every finite point
    _check_stray(pts, cuda, nb=1500, radius=100.0)           # a radius far larger than the cloud
    _check_stray(pts, cuda, nb=3001, radius=100.0)
    _check_stray(bad, cuda, count=1234)                      # a device count below n_max
    _check_stray(bad, cuda, count=0)


@pytest.mark.gpu
def test_stray_overflow_flag_keeps_everything(cuda):
    import torch

    from depth_pro import pointcloud as PC

    pts = np.array([[0.0, 0.0, 0.0], [1.0e7, 0.0, 0.0], [np.nan, 0.0, 0.0]])       # 1e8 cells of 0.1 on x
    keep, stats = PC.stray_mask(torch.from_numpy(pts).to(cuda), None, 1, 0.1)
    assert keep.cpu().tolist() == [1, 1, 1] and stats.cpu().tolist() == [2, 1, 3, 0, 1, 0, 0, 0]


# ---- GPU: shadows ---------------------------------------------------------------------------------------------

def _check_shadows(pts, cuda, count=None, **kw):
    import torch

    from depth_pro import pointcloud as PC

    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    live = len(pts) if count is None else count
    keep, stats = PC.shadow_mask(torch.from_numpy(pts).to(cuda), count, **kw)
    want, wstats, info = C.shadow_mask(pts[:live], **kw)
    got = keep.cpu().numpy()[:live].astype(bool)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(stats.cpu().numpy(), wstats), (stats.cpu().numpy(), wstats)      # the cell size bit for bit
    return want, wstats, info


@pytest.mark.gpu
def test_shadows_fixture(gold, cuda):
    for s in gold["scenes"]:
        p1 = gold[f"{s}_points"][gold[f"{s}_stray_keep"]]
        want, stats, _ = _check_shadows(p1, cuda)
        assert np.array_equal(want, gold[f"{s}_shadow_keep"]) and stats[6] == gold[f"{s}_cell"]


def _zigzag(angles, dy):
    x, y, out = 0.0, 0.0, [(0.0, 0.0, 0.0)]
    for a in angles:
        x += (-1.0 if x > 0 else 1.0) * dy * np.tan(np.radians(a))
        y += dy
        out.append((x, y, 0.0))
    return np.array(out)


def hand_columns():
    """(points, {name: (slice, removed?)}): one rule of the column test per column.  Two flat fillers at the
    corners fix the extent and the density, hence the cell (~0.6 m); every column is then centred in a cell
    of its own.  Expected outcomes are worked out by hand."""
    v = lambda ys: np.c_[np.zeros(len(ys)), ys, np.zeros(len(ys))]          # noqa: E731  a vertical column
    cols = {
        "two_points": (v([0.0, 0.5]), False),                                # fewer than 3 points: never tested
        "three_vertical": (v([0.0, 0.2, 0.4]), True),
        "height_below": (v([0.0, 0.05, 0.0999]), False),                     # 0.0999 > 0.1 is false: not tested
        "height_above": (v([0.0, 0.05, 0.1001]), True),
        "odd_removed": (_zigzag([10, 80, 20, 82, 30], 0.03), True),          # 5 angles, 3 below
        "odd_kept": (_zigzag([10, 80, 82, 81, 30], 0.03), False),            # 5 angles, 2 below
        "even_removed": (_zigzag([10, 20, 30, 82], 0.03), True),             # 4 angles, 3 below
        "even_kept": (_zigzag([10, 80, 82, 81], 0.03), False),               # 4 angles, 1 below
        "half_below": (_zigzag([10, 60, 80, 82], 0.03), True),               # c == m/2: (60 + 80) / 2 < 75
        "half_above": (_zigzag([10, 72, 80, 82], 0.03), False),              # c == m/2: (72 + 80) / 2 > 75
        "duplicate": (v([0.0, 0.1, 0.1, 0.2, 0.3]), False),                  # a zero-length step: NaN median
        # equal y: index order A, B, C gives angles (70, 90) -> 80, kept; the order A, C, B would give (0, 90) -> 45
        "tie_kept": (np.array([[0.0, 0.0, 0.0], [0.11 * np.tan(np.radians(70)), 0.11, 0.0], [0.0, 0.11, 0.0]]), False),
        "tie_removed": (np.array([[0.0, 0.0, 0.0], [0.0, 0.11, 0.0], [0.11 * np.tan(np.radians(70)), 0.11, 0.0]]), True),
    }
    rng = np.random.default_rng(21)
    flat = lambda c: np.c_[rng.uniform(0, 0.1, 1500), rng.uniform(0, 0.05, 1500), rng.uniform(0, 0.1, 1500)] + c   # noqa: E731
    fill = np.concatenate([flat(np.array([-2.0, 0.0, -1.0])), flat(np.array([16.0, 0.0, 5.0]))])
    n = len(fill) + sum(len(p) for p, _ in cols.values())
    ext = fill[:, [0, 2]].max(axis=0) - fill[:, [0, 2]].min(axis=0)
    cell = 1.0 / np.sqrt(n / (ext[0] * ext[1]) / 10)                       # checked against the restatement's below
    x0, z0 = fill[:, 0].min(), fill[:, 2].min()
    parts, where, at = [fill], {}, len(fill)
    for i, (name, (p, removed)) in enumerate(cols.items()):
        p = p - np.array([(p[:, 0].min() + p[:, 0].max()) / 2, 0.0, 0.0])
        ix, iz = 3 + 3 * (i // 2), 3 + 3 * (i % 2)                          # cells apart from each other and the fillers
        parts.append(p + np.array([x0 + (ix + 0.5) * cell, 0.0, z0 + (iz + 0.5) * cell]))
        where[name] = (slice(at, at + len(p)), removed)
        at += len(p)
    return np.concatenate(parts), where


def test_hand_columns_are_what_they_claim():
    """CPU: the hand-built scene under the restatement -- every column alone in its cell, outcomes as listed."""
    pts, where = hand_columns()
    keep, stats, info = C.shadow_mask(pts)
    assert stats[7] == 0 and 0.5 < stats[6] < 1.0, stats
    col = info["column_of"]
    for name, (sl, removed) in where.items():
        assert len(set(col[sl])) == 1 and (col == col[sl][0]).sum() == sl.stop - sl.start, name
        assert (keep[sl] == (not removed)).all(), name
    assert keep[:3000].all() and pts[:, 0].max() < 16.1 and pts[:, 2].max() < 5.1      # the fillers set the extent


@pytest.mark.gpu
def test_shadows_hand_built_columns(cuda):
    pts, where = hand_columns()
    want, _, _ = _check_shadows(pts, cuda)
    for name, (sl, removed) in where.items():
        assert (want[sl] == (not removed)).all(), name
    # other parameters: a lower limit flips the c == m/2 column, a higher minimum count skips the 3-point ones
    _check_shadows(pts, cuda, max_shadow_angle=65)
    _check_shadows(pts, cuda, min_points_per_column=4, shadow_height_threshold=0.25)


@pytest.mark.gpu
def test_shadows_degenerate_and_non_finite(cuda):
    rng = np.random.default_rng(22)
    line = np.c_[np.full(500, 1.25), rng.uniform(0, 2, 500), rng.uniform(0, 1, 500)]     # all x equal: area 0
    _, stats, _ = _check_shadows(line, cuda)
    assert stats[6] == 0.05 and stats[7] == 0
    _, stats, _ = _check_shadows(np.zeros((0, 3)), cuda)
    assert stats[6] == 0.05
    _check_shadows(np.array([[0.5, 1.0, 2.0]]), cuda)
    pts, _ = hand_columns()
    bad = np.concatenate([pts, pts[:50] + 0.3])
    bad[5::9, 1] = np.nan
    bad[3000::4, 0] = np.inf
    want, stats, _ = _check_shadows(bad, cuda)
    assert want[~np.isfinite(bad).all(axis=1)].all() and stats[1] > 0                     # in no column, kept, counted
    _check_shadows(bad, cuda, count=3033)
    _check_shadows(bad, cuda, count=0)


@pytest.mark.gpu
def test_shadows_overflow_flag_keeps_everything(cuda):
    import torch

    from depth_pro import pointcloud as PC

    # 2^31 columns of >= 0.05 m need more points than a test can hold (columns ~ points / 10); the flag's other
    # cause is reachable: an x extent that overflows fp64 leaves no finite number of columns
    pts = np.array([[-1.5e308, 0.0, 0.0], [-1.5e308, 1.0, 0.0], [-1.5e308, 2.0, 0.0], [1.5e308, 0.0, 3.0]])
    keep, stats = PC.shadow_mask(torch.from_numpy(pts).to(cuda))
    want, wstats, _ = C.shadow_mask(pts)
    assert wstats[7] == 1 and keep.cpu().tolist() == [1, 1, 1, 1] and np.array_equal(stats.cpu().numpy(), wstats)


# ---- GPU: compaction ----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "all", "none", "per_wave"])
def test_compaction(kind, cuda):
    import torch

    from depth_pro import _lib
    from depth_pro import pointcloud as PC

    rng = np.random.default_rng(31)
    n_max, n = 10007, 9001
    pts = rng.standard_normal((n_max, 3))
    pts[::17, 1] = np.nan                                    # rows are copied as bytes
    cols = rng.integers(0, 256, (n_max, 3), dtype=np.uint8)
    mask = {"random": rng.random(n_max) < 0.6, "all": np.ones(n_max, bool), "none": np.zeros(n_max, bool),
            "per_wave": (np.arange(n_max) // 64) % 2 == 0}[kind]
    lib = _lib.load()
    P, Cc, K = (torch.from_numpy(a).to(cuda) for a in (pts, cols, mask.astype(np.uint8)))
    count = torch.tensor([n], dtype=torch.int32, device=cuda)
    out = torch.full((n_max, 3), -7.25, dtype=torch.float64, device=cuda)        # canaries
    cout = torch.full((n_max, 3), 201, dtype=torch.uint8, device=cuda)
    n_out = torch.full((1,), -1, dtype=torch.int32, device=cuda)
    ws = torch.empty(int(lib.dp_clean_workspace_size(n_max)), dtype=torch.uint8, device=cuda)
    _lib.check(lib.dp_compact_points(P.data_ptr(), Cc.data_ptr(), K.data_ptr(), count.data_ptr(), n_max, out.data_ptr(),
                                     cout.data_ptr(), n_out.data_ptr(), ws.data_ptr(), ws.numel(),
                                     torch.cuda.current_stream(cuda).cuda_stream), "dp_compact_points")
    m = int(n_out.item())
    assert m == mask[:n].sum()
    assert out.cpu().numpy()[:m].tobytes() == pts[:n][mask[:n]].tobytes()
    assert cout.cpu().numpy()[:m].tobytes() == cols[:n][mask[:n]].tobytes()
    assert (out[m:] == -7.25).all().item() and (cout[m:] == 201).all().item()
    # the Python wrapper, without colours and without a count
    o2, c2, n2 = PC.compact_points(P, None, K)
    assert c2 is None and int(n2.item()) == mask.sum()
    assert o2.cpu().numpy()[:int(n2.item())].tobytes() == pts[mask].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n,kind", [(2047, "random"), (2048, "random"), (2049, "random"), (524288, "random"),
                                    (524289, "random"), (2049, "none"), (2049, "all")])
def test_flag_scan_across_tile_edges(n, kind, cuda):
    """The byte-flag scan the compaction and the clustering share (csrc/dp_points.h), one row either side of a
    2048-row tile, and at 256 tiles and 256 tiles + 1 row: from there on a thread of the block-offsets kernel
    walks more than one tile count.  Compaction: kept rows and the device count, exactly.  Clustering (random
    flags only): the stride sample ranks every eligible row with the same scan; max_points is a third of the
    eligible rows (1000 at the most, to keep the numpy side quick), against tests/cluster_numpy.py."""
    import torch

    import cluster_numpy as N
    from depth_pro import pointcloud as PC

    rng = np.random.default_rng(41)
    pts = rng.random((n, 3))
    keep = {"random": rng.random(n) < 0.5, "none": np.zeros(n, bool), "all": np.ones(n, bool)}[kind]
    P = torch.from_numpy(pts).to(cuda)
    out, _, n_out = PC.compact_points(P, None, torch.from_numpy(keep).to(cuda))
    m = int(n_out.item())
    assert m == keep.sum()
    assert np.array_equal(out[:m].cpu().numpy(), pts[np.flatnonzero(keep)])
    if kind != "random":
        return
    pts[:, 1] = np.where(keep, 2.0, 0.0)                         # the same flags as eligibility: y >= 1.3
    mp = min(int(keep.sum()) // 3, 1000)
    labels, ncl, stats = PC.dbscan_labels(torch.from_numpy(pts).to(cuda), None, 0.05, 4, 1.3, mp)
    want, _, wstats = N.dbscan(pts, 0.05, 4, 1.3, mp)
    assert wstats[2] == mp and (want == -2).sum() == n - mp
    assert np.array_equal(labels.cpu().numpy(), want)
    assert np.array_equal(stats.cpu().numpy(), wstats) and int(ncl.item()) == int(wstats[6])


# ---- GPU: the whole stage and the frame loop ----------------------------------------------------------------------

@pytest.mark.gpu
def test_clean_pointcloud_equals_the_reference_sequence(gold, restated, cuda):
    import torch

    from depth_pro import pointcloud as PC

    for s in gold["scenes"]:
        pts, cols = gold[f"{s}_points"], gold[f"{s}_colors"]
        k1, k2 = gold[f"{s}_stray_keep"], gold[f"{s}_shadow_keep"]
        pad = np.concatenate([pts, np.full((100, 3), 9.0)])                  # rows past the device count
        cpad = np.concatenate([cols, np.zeros((100, 3), np.uint8)])
        out, cout, n, st1, st2 = PC.clean_pointcloud(torch.from_numpy(pad).to(cuda), torch.from_numpy(cpad).to(cuda),
                                                     torch.tensor(len(pts), dtype=torch.int32, device=cuda))
        m = int(n.item())
        assert m == k2.sum()
        assert np.array_equal(out.cpu().numpy()[:m], pts[k1][k2]) and np.array_equal(cout.cpu().numpy()[:m], cols[k1][k2])
        _, _, _, _, ws1, ws2 = restated[str(s)]
        assert np.array_equal(st1.cpu().numpy(), ws1) and np.array_equal(st2.cpu().numpy(), ws2)


class _FixtureModel:
    """A stand-in for the network: every frame gets the ground fixture's depth and focal length."""

    def __init__(self, depth, f, cuda):
        import torch

        self.depth, self.f = torch.from_numpy(depth).to(cuda), torch.tensor(float(f), device=cuda)

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
def test_loop_clean_pointcloud(tmp_path, cuda):
    """--clean_pointcloud writes {base}_clean.ply = the restatement applied to the levelled cloud the loop
    writes with --normalize_ground alone, and no {base}_points.ply; --resume then has nothing to do."""
    import generate_depth_maps as G
    from depth_pro import pointcloud as PC

    lev, out = tmp_path / "levelled", tmp_path / "clean"
    _run_loop(tmp_path, cuda, lev, normalize_ground=True)
    kw = dict(clean_pointcloud=True, stray_radius=0.25, stray_neighbors=12)
    _run_loop(tmp_path, cuda, out, **kw)
    assert sorted(os.listdir(out)) == ["ground.json", "output_0000_clean.ply", "output_0000_depth.png",
                                       "output_0001_clean.ply", "output_0001_depth.png"]
    for k in range(2):
        pts, cols = PC.read_ply(str(lev / f"output_{k:04d}_points.ply"))
        p2, c2, k1, k2, _, _ = C.clean(pts, cols, nb_points=12, radius=0.25)
        assert 0 < k1.sum() < len(pts) and 0 < len(p2)
        want = tmp_path / "want.ply"
        PC.write_ply(str(want), p2, c2)
        assert open(out / f"output_{k:04d}_clean.ply", "rb").read() == open(want, "rb").read()
    src = sorted(str(p) for p in (tmp_path / "frames").glob("*.png"))
    assert G.plan_frames(src, str(out), 1, 0, True, cleaned=True) == []
    assert G.plan_frames(src, str(lev), 1, 0, True, cleaned=True) == [0, 1]


@pytest.mark.gpu
def test_loop_without_the_flag_writes_the_parents_files(tmp_path, cuda):
    """Without --clean_pointcloud: {base}_points.ply, equal to what the existing PC functions give."""
    import torch

    from depth_pro import pointcloud as PC

    gg = np.load(os.path.join(GOLDEN, "golden_ground.npz"))
    out = tmp_path / "plain"
    _run_loop(tmp_path, cuda, out, frames=1, normalize_ground=True)
    assert sorted(os.listdir(out)) == ["ground.json", "output_0000_depth.png", "output_0000_points.ply"]
    depth = torch.from_numpy(gg["flat_depth"]).to(cuda)
    rgb = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (96, 128, 3), dtype=np.uint8)).to(cuda)
    xyz, _, cols, count = PC.depth_to_points_async(depth, float(gg["flat_f"]), 128, 96, rgb=rgb)
    plane = PC.load_ground_plane_params("x", str(out))
    xyz, _ = PC.normalize_to_ground(xyz, plane, count)
    xyz, _ = PC.ground_adjust(xyz, 20, 5, count)
    n = int(count.item())
    want = tmp_path / "want.ply"
    PC.write_ply(str(want), xyz[:n].cpu().numpy(), cols[:n].cpu().numpy())
    assert open(out / "output_0000_points.ply", "rb").read() == open(want, "rb").read()
