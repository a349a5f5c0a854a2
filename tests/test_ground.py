"""Ground-normalised point clouds: fit, level, grid-adjust (csrc/dp_ground.hip, depth_pro/pointcloud.py).

Expected values: the reference's own functions through tests/golden/golden_ground.npz
(make_golden_ground.py), and tests/ground_numpy.py -- pinned to that fixture by the CPU tests here --
at the sizes the fixture lacks.

Tolerance of the GPU comparisons: ATOL = 1e-10 m on coordinates and on the model.  numpy's BLAS dot
products and pairwise means fix no summation order, so bit-exactness is not available; the rounding
bound of three fp64 terms at coordinates <= 100 m is about 4e-14, 1e-10 is > 1000 x that and 8
orders below the smallest decision threshold, and every comparison first asserts that no point
lies within 1e-6 of a discontinuous decision (the `margin` of ground_numpy; 1e-12, with the reason
given there, for the 1080p frame that is compared with the restatement alone), so no classification
can flip inside it.  Zero points may differ by more than ATOL.  The selection primitive itself is
compared exactly (the lerp formula is fixed).
"""

import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ground_numpy as GN  # noqa: E402

ATOL = 1e-10
ADJUST_CASES = ((20, 5), (7, 50))


@pytest.fixture(scope="module")
def gold(golden_dir):
    z = np.load(os.path.join(golden_dir, "golden_ground.npz"))
    return {k: z[k] for k in z.files}


def _host_points(depth, f):
    """depth_to_3d (img_to_normalized_pointcloud.py:819-856) as the oracle restates it."""
    from oracle import depth_pro_oracle as O

    h, w = depth.shape
    return O.depth_to_3d(depth, float(f), w, h)[0]


def _model_of(vec):
    return {"normal": vec[:3].copy(), "d": float(vec[3]), "origin": vec[4:7].copy()}


def _gold_normalized(gold, name, pts):
    n = gold[f"{name}_normalized"]
    if gold[f"{name}_rotated"]:
        return n
    out = pts.copy()
    out[:, 1] = n
    return out


def _close(got, want, what):
    bad = int((~(np.abs(got - want) <= ATOL)).sum())
    assert bad == 0, f"{what}: {bad} values differ by more than {ATOL} (max {np.nanmax(np.abs(got - want)):.3e})"


# ---- CPU: the restatement against the reference fixture, the json helpers, the CLI ----------------

def test_fixture_covers_the_branches(gold):
    assert not gold["flat_rotated"] and gold["side_rotated"]          # no-rotation and Rodrigues branches
    assert gold["strip_fallback"] and not gold["flat_fallback"]      # < 10 trace bins -> lowest-5 % fallback


@pytest.mark.parametrize("name", ["flat", "side", "strip"])
def test_restatement_matches_reference(gold, name):
    pts = _host_points(gold[f"{name}_depth"], gold[f"{name}_f"])
    model, info = GN.fit(pts)
    assert info["tie_free"] and info["margin"] > 1e-6 and info["pushdown_safe"]
    want = gold[f"{name}_model"]
    _close(np.concatenate([model["normal"], [model["d"]], model["origin"]]), want, "model")
    ref_model = _model_of(want)
    normed, _, margin = GN.normalize(pts, ref_model)
    assert margin > 1e-6
    want_n = _gold_normalized(gold, name, pts)
    _close(normed, want_n, "normalised")
    for gs, pc in ADJUST_CASES:
        adj, _, margin = GN.adjust(want_n, gs, pc)
        assert margin > 1e-6
        assert np.array_equal(adj[:, [0, 2]], want_n[:, [0, 2]])
        _close(adj[:, 1], gold[f"{name}_adjusted_{gs}_{pc}"], f"adjusted {gs} {pc}")


def test_ground_json_round_trip(tmp_path, gold):
    from depth_pro import pointcloud as PC

    model = _model_of(gold["side_model"])
    path = PC.save_ground_plane_params(model, str(tmp_path / "frame_0001.png"))
    assert path == str(tmp_path / "ground.json")
    want = json.dumps({"normal": model["normal"].tolist(), "d": model["d"], "origin": model["origin"].tolist()},
                      indent=4)
    assert open(path).read() == want
    back = PC.load_ground_plane_params(str(tmp_path / "other.png"))
    assert np.array_equal(back["normal"], model["normal"]) and back["d"] == model["d"]
    assert np.array_equal(back["origin"], model["origin"])
    # legacy name, other directory
    legacy = tmp_path / "legacy"
    legacy.mkdir()
    os.rename(path, legacy / "frame_0001_ground_plane.json")
    assert PC.load_ground_plane_params(str(tmp_path / "frame_0001.png")) is None
    got = PC.load_ground_plane_params(str(tmp_path / "frame_0001.png"), str(legacy))
    assert got["d"] == model["d"]
    assert PC.load_ground_plane_params(str(tmp_path / "frame_0002.png"), str(legacy)) is None
    assert PC.save_ground_plane_params(None, str(tmp_path / "x.png")) is None


@pytest.mark.parametrize("name", ["flat", "side", "strip"])
def test_apply_rotation_to_plane(gold, name):
    from depth_pro import pointcloud as PC

    model = _model_of(gold[f"{name}_model"])
    rot = PC.apply_rotation_to_plane(model, gold["rot_offset"].tolist())
    got = np.concatenate([rot["normal"], [rot["d"]]])
    assert np.abs(got - gold[f"{name}_rot_model"]).max() <= 1e-15
    assert np.array_equal(rot["origin"], model["origin"])
    assert PC.apply_rotation_to_plane(None, [0, 0, 0]) is None


def test_fit_trace_plane_drops_outliers_and_refits():
    """The host fit, against plain numpy written here: a trace on a plane with noise below the
    threshold, one point 0.5 m above it and one that only the second pass sees as an outlier; the
    result is the least-squares plane through the remaining points."""
    from depth_pro.pointcloud import fit_trace_plane

    g = np.random.default_rng(0)
    x, z = g.uniform(-2, 2, 16), np.linspace(1.0, 8.0, 16)
    y = 0.02 * x - 0.06 * z - 1.4 + g.uniform(-0.01, 0.01, 16)
    y[3] += 0.5                 # pulls the first fit up by about 0.03
    y[9] -= 0.118               # residual < 0.1 against the first fit, > 0.1 once point 3 is gone
    trace = np.stack([x, y, z], axis=1)

    def lsq(keep):
        A = np.stack([x[keep], z[keep], np.ones(keep.sum())], axis=1)
        return np.linalg.lstsq(A, y[keep], rcond=None)[0]

    keep, passes = np.ones(16, dtype=bool), 0
    while True:
        a, c, d = lsq(keep)
        new = np.abs(y - (a * x + c * z + d)) <= 0.1
        passes += 1
        if (new == keep).all():
            break
        keep = new
    assert passes >= 3 and not keep[3] and not keep[9] and keep.sum() == 14    # two refits, each dropping a point
    normal, dd = fit_trace_plane(trace)
    want = np.array([-a, 1.0, -c])
    want /= np.linalg.norm(want)
    assert np.abs(normal - want).max() <= 1e-12 and abs(dd + d) <= 1e-12
    # fewer than 10 trace points, or steeper than 20 degrees: the horizontal plane at the median y
    n9, d9 = fit_trace_plane(trace[:9])
    assert np.array_equal(n9, [0.0, 1.0, 0.0]) and d9 == -np.median(y[:9])
    steep = trace.copy()
    steep[:, 1] = 0.5 * z
    ns, ds = fit_trace_plane(steep)
    assert np.array_equal(ns, [0.0, 1.0, 0.0]) and ds == -np.median(steep[:, 1])


def test_ground_rotation_is_the_rodrigues_rotation():
    """`ground_rotation` against its defining properties: R is a rotation taking the unit normal onto
    +y, const is the plane's height after it; the no-rotation branch starts at |n . y| > 0.99."""
    from depth_pro.pointcloud import ground_rotation

    n = np.array([0.2, 0.9, -0.3])
    n /= np.linalg.norm(n)
    m = ground_rotation({"normal": n, "d": 1.3})
    R = m[4:13].reshape(3, 3)
    assert m[14] == 1.0 and np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1) < 1e-14
    assert np.abs(R @ n - [0.0, 1.0, 0.0]).max() < 1e-14 and abs(m[13] + 1.3) < 1e-13
    flat = ground_rotation({"normal": np.array([0.0, 0.995, 0.0998749]), "d": 1.3})
    assert flat[14] == 0.0 and flat[13] == 0.0 and np.array_equal(flat[4:13].reshape(3, 3), np.eye(3))


@pytest.mark.parametrize("grid", ["0", "33", "-4"])
def test_cli_refuses_grid_size(monkeypatch, grid, tmp_path):
    import generate_depth_maps as G

    monkeypatch.setattr(sys, "argv", ["generate_depth_maps.py", "--input_dir", str(tmp_path), "--normalize_ground",
                                      "--grid_size", grid])
    with pytest.raises(SystemExit) as e:
        G.main()
    assert e.value.code == 2
    with pytest.raises(ValueError):
        G.batch_generate_depth_maps(str(tmp_path), str(tmp_path / "o"), normalize_ground=True, grid_size=int(grid))


# ---- GPU: the selection primitive -------------------------------------------------------------------

def _keys(kind, n, rng):
    if kind == "random":
        return rng.standard_normal(n) * 3.0
    if kind == "equal":
        return np.full(n, -0.1)
    if kind == "two":
        return rng.choice(np.array([0.0, -0.1]), n)
    if kind == "zeros":
        return rng.choice(np.array([0.0, -0.0, 1.5, -2.5]), n)
    if kind == "coarse":                      # many ties, negatives, a wide exponent range
        return np.round(rng.standard_normal(n) * 4.0) * 10.0 ** rng.integers(-3, 3, n)
    raise ValueError(kind)


QS = (0, 0.1, 2, 5, 50, 100)
KTH_RULES = ((0.05, 1, 10), (0.05, 10, 0))      # the ground trace's rule and the fallback's


def _expected_select(keys, seg, n_seg):
    """counts, {q: np.percentile per segment}, {rule: k-th smallest per segment}; one sort-and-group pass."""
    order = np.argsort(seg, kind="stable")
    ss, ks = seg[order], keys[order]
    lo, hi = np.searchsorted(ss, np.arange(n_seg)), np.searchsorted(ss, np.arange(n_seg), side="right")
    counts = (hi - lo).astype(np.int32)
    pct = {q: np.full(n_seg, np.nan) for q in QS}
    kth = {r: np.full(n_seg, np.nan) for r in KTH_RULES}
    for s in np.flatnonzero(counts):
        k = ks[lo[s]:hi[s]]
        for q, v in zip(QS, np.percentile(k, QS)):
            pct[q][s] = v
        k = np.sort(k)
        for r in KTH_RULES:
            frac, kmin, min_count = r
            if len(k) > min_count:
                kth[r][s] = k[min(len(k), max(kmin, int(frac * len(k)))) - 1]
    return counts, pct, kth


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 70001])
def test_select_primitive(cuda, n):
    """dp_seg_select == np.percentile / np.partition's k-th value, exactly, for every (segments, q, key kind)."""
    import torch

    from depth_pro import pointcloud as PC

    rng = np.random.default_rng(n)
    for n_seg in (1, 3, 400, 1024):
        for kind in ("random", "equal", "two", "zeros", "coarse"):
            keys = _keys(kind, n, rng)
            seg = rng.integers(-1, n_seg, n).astype(np.int32)     # -1: in no segment
            if n_seg >= 3 and n:
                seg[seg == 1] = 0                                 # segment 1 stays empty
            if kind == "equal":
                seg[:] = n_seg - 1                                # one segment holds every key
            wc, wpct, wkth = _expected_select(keys, seg, n_seg)
            kd, sd = torch.from_numpy(keys).to(cuda), torch.from_numpy(seg).to(cuda)
            for q in QS:
                counts, vals = PC.segmented_select(kd, sd, n_seg, q=q)
                assert np.array_equal(counts.cpu().numpy(), wc), (n_seg, kind, q)
                assert np.array_equal(vals.cpu().numpy(), wpct[q], equal_nan=True), (n_seg, kind, q)
            for r in KTH_RULES:
                counts, vals = PC.segmented_select(kd, sd, n_seg, frac=r[0], kmin=r[1], min_count=r[2])
                assert np.array_equal(counts.cpu().numpy(), wc), (n_seg, kind, r)
                assert np.array_equal(vals.cpu().numpy(), wkth[r], equal_nan=True), (n_seg, kind, r)


@pytest.mark.gpu
def test_select_lerp_sides_and_live_count(cuda):
    """A rank exactly on an index (t = 0), t < 0.5 and t >= 0.5 take numpy's two lerp forms; a device
    `count` limits the live keys."""
    import torch

    from depth_pro import pointcloud as PC

    keys = np.array([0.1, 0.7, 0.30000000000000004, 1e-3, 5.5, -2.25, 0.2, 9.0, 3.3, 0.1, 4.4])
    kd = torch.from_numpy(keys).to(cuda)
    sd = torch.zeros(len(keys), dtype=torch.int32, device=cuda)
    for live in (11, 5):
        cnt = torch.tensor([live], dtype=torch.int32, device=cuda)
        for q in (50, 30, 33, 77, 99.9, 10):          # (live - 1) * q / 100: integral, t < 0.5, t >= 0.5
            counts, vals = PC.segmented_select(kd, sd, 1, q=q, count=cnt)
            assert int(counts.cpu()[0]) == live
            assert vals.cpu().numpy()[0] == np.percentile(keys[:live], q), (live, q)


# ---- GPU: fit, normalise, adjust ----------------------------------------------------------------------

def _device_points(depth, f, cuda):
    import torch

    from depth_pro import pointcloud as PC

    h, w = depth.shape
    xyz, _, _, count = PC.depth_to_points_async(torch.from_numpy(depth).to(cuda), float(f), w, h)
    return xyz, count


def _stages_vs(cuda, xyz, count, pts, model_want, normed_want, adjusted_want):
    """fit / normalise / adjust on the device against the given expected values (host arrays)."""
    from depth_pro import pointcloud as PC

    n = len(pts)
    model = PC.fit_ground_plane(xyz, count)
    _close(np.concatenate([model["normal"], [model["d"]], model["origin"]]), model_want, "model")
    ref_model = _model_of(model_want)
    normed, nstats = PC.normalize_to_ground(xyz, ref_model, count)
    _close(normed[:n].cpu().numpy(), normed_want, "normalised")
    import torch

    want_dev = torch.from_numpy(np.ascontiguousarray(normed_want)).to(cuda)
    for (gs, pc), want in adjusted_want.items():
        adj, astats = PC.ground_adjust(want_dev, gs, pc)
        got = adj.cpu().numpy()
        assert np.array_equal(got[:, [0, 2]], normed_want[:, [0, 2]])
        _close(got[:, 1], want, f"adjusted {gs} {pc}")
    return nstats.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["flat", "side", "strip"])
def test_stages_match_reference_fixture(cuda, gold, name):
    depth, f = gold[f"{name}_depth"], gold[f"{name}_f"]
    pts = _host_points(depth, f)
    xyz, count = _device_points(depth, f, cuda)
    adjusted = {(gs, pc): gold[f"{name}_adjusted_{gs}_{pc}"] for gs, pc in ADJUST_CASES}
    _stages_vs(cuda, xyz, count, pts, gold[f"{name}_model"], _gold_normalized(gold, name, pts), adjusted)


@pytest.fixture(scope="module")
def terrain():
    """The 1080p frame and its restated stages, computed once.

    Two million points cannot all stay 1e-6 away from a threshold, and here they need not: the
    device is compared with the restatement on identical inputs.  Bin edges, the y < 0.2 test and
    the cell percentiles are then the same operations on the same numbers (exact on both sides);
    only |dist| sums three products, with a rounding bound of about 4e-14 at these coordinates, so a
    margin of 1e-12 on |dist| - 0.05 / 0.1 already excludes a flipped classification."""
    depth, f = GN.terrain(1080, 1920, 7)
    pts = _host_points(depth, f)
    model, info = GN.fit(pts)
    assert info["tie_free"] and not info["fallback"] and info["pushdown_safe"]
    normed, nstats, m1 = GN.normalize(pts, model)
    adj, astats, _ = GN.adjust(normed, 20, 5)
    assert m1 > 1e-12, m1
    return dict(depth=depth, f=f, pts=pts, model=model, normed=normed, nstats=nstats, adj=adj, astats=astats)


@pytest.mark.gpu
def test_stages_match_restatement_1080p(cuda, terrain):
    from depth_pro import pointcloud as PC

    t = terrain
    xyz, count = _device_points(t["depth"], t["f"], cuda)
    m = t["model"]
    vec = np.concatenate([m["normal"], [m["d"]], m["origin"]])
    nstats = _stages_vs(cuda, xyz, count, t["pts"], vec, t["normed"], {(20, 5): t["adj"][:, 1]})
    assert np.array_equal(nstats[[0, 1, 2, 4, 5, 6, 7]], t["nstats"][[0, 1, 2, 4, 5, 6, 7]])
    assert abs(nstats[3] - t["nstats"][3]) <= ATOL
    import torch

    _, astats = PC.ground_adjust(torch.from_numpy(t["normed"]).to(cuda), 20, 5)
    assert np.array_equal(astats.cpu().numpy(), t["astats"])


@pytest.mark.gpu
def test_single_pixel_and_empty_frames(cuda):
    import torch

    from depth_pro import pointcloud as PC

    # (1, 1): one point; the fit falls back to the horizontal plane through it
    depth = np.array([[2.5]], dtype=np.float32)
    pts = _host_points(depth, 3.0)
    xyz, count = _device_points(depth, 3.0, cuda)
    model, _ = GN.fit(pts)
    normed, _, _ = GN.normalize(pts, model)
    adj, _, _ = GN.adjust(normed, 20, 5)
    _stages_vs(cuda, xyz, count, pts, np.concatenate([model["normal"], [model["d"]], model["origin"]]), normed,
               {(20, 5): adj[:, 1]})
    # all-invalid frame: count = 0; nothing is touched, every counter is 0
    depth = np.full((5, 7), np.nan, dtype=np.float32)
    xyz, count = _device_points(depth, 3.0, cuda)
    flat = {"normal": np.array([0.0, 1.0, 0.0]), "d": 1.0, "origin": np.array([0.0, -1.0, 0.0])}
    _, nstats = PC.normalize_to_ground(xyz, flat, count)
    _, astats = PC.ground_adjust(xyz, 20, 5, count)
    assert np.array_equal(nstats.cpu().numpy(), np.zeros(8)) and np.array_equal(astats.cpu().numpy(), np.zeros(8))
    counts, vals = PC.segmented_select(xyz[:, 1].contiguous(), torch.zeros(35, dtype=torch.int32, device=cuda), 3,
                                       q=5, count=count)
    assert np.array_equal(counts.cpu().numpy(), np.zeros(3)) and np.isnan(vals.cpu().numpy()).all()
    with pytest.raises(ValueError):
        PC.fit_ground_plane(xyz, count)
    empty = torch.empty(0, 3, dtype=torch.float64, device=cuda)
    out, nstats = PC.normalize_to_ground(empty, flat)
    assert out.shape == (0, 3) and np.array_equal(nstats.cpu().numpy(), np.zeros(8))


@pytest.mark.gpu
def test_infinite_depths_are_counted_and_passed_through(cuda, gold):
    """+inf depths give non-finite points: counted, copied unchanged, and the finite points match the
    run without them."""
    from depth_pro import pointcloud as PC

    depth, f = gold["flat_depth"].copy(), gold["flat_f"]
    clean = _host_points(depth, f)
    g = np.random.default_rng(11)
    valid = np.isfinite(depth) & (depth > 0)
    hit = valid & (g.random(depth.shape) < 0.01)
    depth[hit] = np.inf
    inj = int(hit.sum())
    assert inj > 20
    xyz, count = _device_points(depth, f, cuda)
    n = int(count.item())
    assert n == len(clean)
    bad = ~np.isfinite(xyz[:n].cpu().numpy()).all(axis=1)
    assert int(bad.sum()) == inj
    kept = clean[~bad]
    model, info = GN.fit(kept)
    normed, nstats, m1 = GN.normalize(kept, model)
    adj, _, m2 = GN.adjust(normed, 20, 5)
    assert info["tie_free"] and min(info["margin"], m1, m2) > 1e-6 and info["pushdown_safe"]
    got_model = PC.fit_ground_plane(xyz, count)
    _close(np.concatenate([got_model["normal"], [got_model["d"]]]), np.concatenate([model["normal"], [model["d"]]]),
           "model")
    out, st = PC.normalize_to_ground(xyz, model, count)
    st = st.cpu().numpy()
    assert st[1] == inj and st[0] == len(kept)
    o = out[:n].cpu().numpy()
    _close(o[~bad], normed, "normalised (finite)")
    assert np.array_equal(o[bad], xyz[:n].cpu().numpy()[bad], equal_nan=True)
    out2, st2 = PC.ground_adjust(out, 20, 5, count)
    o2 = out2[:n].cpu().numpy()
    assert st2.cpu().numpy()[1] == inj
    _close(o2[~bad][:, 1], GN.adjust(o[~bad], 20, 5)[0][:, 1], "adjusted (finite)")
    assert np.array_equal(o2[bad], o[bad], equal_nan=True)


@pytest.mark.gpu
def test_cell_rule_edges(cuda):
    """Cells holding exactly 9 / 10 points, 4 / 5 low points and percentile 0.0100 / 0.0101: only the
    cells on the passing side of all three rules move."""
    import torch

    from depth_pro import pointcloud as PC

    g = 4
    # cell (xi, zi) centres on a 4 x 4 grid spanned by two corner points (in cells 0 and 15)
    def cell_pts(xi, zi, ys):
        k = len(ys)
        return np.stack([np.full(k, xi + 0.5) + np.linspace(-0.2, 0.2, k), ys, np.full(k, zi + 0.5)], axis=1)

    high = 0.5
    cells = {
        (0, 1): [0.05] * 5 + [high] * 4,                      # 9 points: too few
        (0, 2): [0.05] * 5 + [high] * 5,                      # 10 points, 5 low, p = 0.05: adjusted
        (1, 0): [0.05] * 4 + [high] * 8,                      # 4 low points: skipped
        (1, 1): [0.05] * 5 + [high] * 7,                      # 5 low points: adjusted
        (2, 0): [0.0100] * 6 + [high] * 6,                    # percentile 0.0100: not > 0.01
        (2, 1): [0.0101] * 6 + [high] * 6,                    # percentile 0.0101: adjusted
    }
    parts, where, at = [np.array([[0.0, 3.0, 0.0], [4.0, 3.0, 4.0]])], {}, 2   # corners: x, z in [0, 4], y > 1.5
    for (xi, zi), ys in cells.items():
        parts.append(cell_pts(xi, zi, np.array(ys)))
        where[(xi, zi)] = slice(at, at + len(ys))
        at += len(ys)
    pts = np.concatenate(parts)
    want, wstats, _ = GN.adjust(pts, g, 5)
    moved = {c: bool((want[sl, 1] != pts[sl, 1]).any()) for c, sl in where.items()}
    assert moved == {(0, 1): False, (0, 2): True, (1, 0): False, (1, 1): True, (2, 0): False, (2, 1): True}
    assert wstats[4] == 3
    out, stats = PC.ground_adjust(torch.from_numpy(pts).to(cuda), g, 5)
    assert np.array_equal(out.cpu().numpy(), want)            # same operations in the same order: exact
    assert np.array_equal(stats.cpu().numpy(), wstats)


# ---- GPU: the frame loop ------------------------------------------------------------------------------

class _FixtureModel:
    """A stand-in for the network: every frame gets the fixture's depth (on the device) and focal length,
    so the loop test runs in a second and exercises only the point-cloud path."""

    def __init__(self, depth, f, cuda):
        import torch

        self.depth, self.f = torch.from_numpy(depth).to(cuda), torch.tensor(float(f), device=cuda)

    def infer(self, x, f_px=None):
        return {"depth": self.depth.clone(), "focallength_px": self.f}


def _run_loop(tmp_path, gold, cuda, out, frames=2, **kw):
    import torch
    from PIL import Image

    import generate_depth_maps as G

    src = tmp_path / "frames"
    if not src.exists():
        src.mkdir()
        rgb = np.random.default_rng(3).integers(0, 256, (96, 128, 3), dtype=np.uint8)
        for k in range(frames):
            Image.fromarray(rgb).save(src / f"output_{k:04d}.png")
    model = (_FixtureModel(gold["flat_depth"], gold["flat_f"], cuda), lambda im: torch.as_tensor(np.asarray(im)))
    n = G.batch_generate_depth_maps(str(src), str(out), pattern="output_*.png", model=model, **kw)
    assert n == frames
    return [open(out / f"output_{k:04d}_points.ply", "rb").read() for k in range(frames)]


@pytest.mark.gpu
def test_loop_normalize_ground(tmp_path, gold, cuda):
    """--normalize_ground: levelled PLYs == the reference fixture's adjusted cloud; ground.json holds the
    first frame's fit; a second run reads it and writes byte-identical files."""
    from depth_pro import pointcloud as PC

    out = tmp_path / "pc"
    first = _run_loop(tmp_path, gold, cuda, out, normalize_ground=True)
    saved = json.load(open(out / "ground.json"))
    _close(np.array(saved["normal"] + [saved["d"]] + saved["origin"]), gold["flat_model"], "saved plane")
    stamp = os.stat(out / "ground.json").st_mtime_ns
    pts, cols = PC.read_ply(str(out / "output_0000_points.ply"))
    host = _host_points(gold["flat_depth"], gold["flat_f"])
    assert np.array_equal(pts[:, [0, 2]], host[:, [0, 2]]) and cols.shape == (len(host), 3)
    _close(pts[:, 1], gold["flat_adjusted_20_5"], "levelled PLY")
    assert first[0] == first[1]                                   # the same plane for every frame
    second = _run_loop(tmp_path, gold, cuda, out, normalize_ground=True)
    assert second == first
    assert os.stat(out / "ground.json").st_mtime_ns == stamp      # read, not refitted


@pytest.mark.gpu
def test_loop_without_flag_is_unchanged(tmp_path, gold, cuda):
    """Without --normalize_ground the PLY is the camera-space cloud the loop wrote before."""
    from depth_pro import pointcloud as PC

    out = tmp_path / "plain"
    _run_loop(tmp_path, gold, cuda, out, frames=1, pointcloud=True)
    pts, _ = PC.read_ply(str(out / "output_0000_points.ply"))
    assert np.array_equal(pts, _host_points(gold["flat_depth"], gold["flat_f"]))
    assert not (out / "ground.json").exists()
