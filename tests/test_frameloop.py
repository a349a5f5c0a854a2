"""The generate_depth_maps drop-in: writers pinned to the reference colorize_depth (CPU),
and the pipelined directory loop on the GPU."""

import os
import time

import numpy as np
import pytest

os.environ.setdefault("DEPTH_PRO_SYNTHETIC", "1")  # no checkpoint offline: synthetic weights

import generate_depth_maps as G  # noqa: E402


def test_colorize_matches_reference(golden_dir):
    g = np.load(f"{golden_dir}/golden_frameloop.npz")
    for cmap in ("turbo", "viridis", "jet"):
        assert np.array_equal(G.colorize_depth(g["depth"], cmap=cmap), g[f"color_{cmap}"]), cmap
    d = np.nan_to_num(g["depth"], nan=1.0)
    assert np.array_equal(G.raw_depth_u16(d), g["raw_u16"])


def test_png_writers_roundtrip(tmp_path):
    from PIL import Image

    rgb = (np.arange(48 * 64 * 3) % 251).astype(np.uint8).reshape(48, 64, 3)
    G._write_png(str(tmp_path / "c.png"), rgb)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "c.png")), rgb)
    u16 = (np.arange(48 * 64) * 20).astype(np.uint16).reshape(48, 64)
    G._write_png(str(tmp_path / "r.png"), u16)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "r.png")).astype(np.uint16), u16)


@pytest.mark.gpu
def test_batch_loop_on_gpu(tmp_path, cuda):
    from PIL import Image

    import torch

    src = tmp_path / "frames"
    src.mkdir()
    rng = np.random.default_rng(0)
    for k in range(3):
        Image.fromarray(rng.integers(0, 256, (360, 640, 3), dtype=np.uint8)).save(src / f"output_{k:04d}.png")
    out = tmp_path / "depth"
    n = G.batch_generate_depth_maps(str(src), str(out), pattern="output_*.png")
    assert n == 3
    files = sorted(os.listdir(out))
    assert files == [f"output_{k:04d}_depth.png" for k in range(3)]
    img = np.asarray(Image.open(out / files[0]))
    assert img.shape == (360, 640, 3) and img.dtype == np.uint8
    # the colored PNG is exactly colorize_depth(model.infer(...)) of the same frame
    model, transform = G._model(cuda, False)
    frame = np.asarray(Image.open(src / "output_0000.png"))
    with torch.no_grad():
        depth = model.infer(transform(frame))["depth"].cpu().numpy()
    assert np.array_equal(img, G.colorize_depth(depth))
    n_raw = G.batch_generate_depth_maps(str(src), str(tmp_path / "raw"), pattern="output_*.png", colored=False)
    assert n_raw == 3
    raw = np.asarray(Image.open(tmp_path / "raw" / "output_0001_depth.png"))
    assert raw.shape == (360, 640)


@pytest.mark.gpu
def test_batch_loop_pointcloud_on_gpu(tmp_path, cuda):
    """--pointcloud: one PLY per frame == depth_to_3d(infer depth, infer f_px) with the frame's colours."""
    from PIL import Image

    import torch

    from depth_pro import pointcloud as PC
    from oracle import depth_pro_oracle as O

    src = tmp_path / "frames"
    src.mkdir()
    img = np.random.default_rng(5).integers(0, 256, (270, 480, 3), dtype=np.uint8)
    Image.fromarray(img).save(src / "output_0000.png")
    out = tmp_path / "pc"
    assert G.batch_generate_depth_maps(str(src), str(out), pattern="output_*.png", pointcloud=True) == 1
    pts, cols = PC.read_ply(str(out / "output_0000_points.ply"))
    model, transform = G._model(cuda, False)
    with torch.no_grad():
        pred = model.infer(transform(img))
    depth = pred["depth"].cpu().numpy()
    ref, valid = O.depth_to_3d(depth, float(pred["focallength_px"]), 480, 270)
    assert np.array_equal(pts, ref)
    assert np.array_equal(cols, img[valid])


def test_bad_frame_dropped_once_by_its_writer(tmp_path):
    """a bad frame whose status is already final when the NEXT frame is submitted (the
    GPU finished it before its writer thread looked at it) is reported by its own writer only.
    The loop claims each frame's status (BatchStatus.claim), so the next infer's non-blocking sweep
    of finished frames (DepthPro._check_earlier -> Engine.check_status(block=False)) skips it:
    frames 0 and 2 are written, frame 1 is dropped, and no frame is dropped in its place.  The
    engine's sweep is the real one (Engine._sweep / check_status); the forward is a CPU stub whose
    frames are finished at once."""
    import threading

    import torch
    from PIL import Image

    from depth_pro.engine import BatchStatus, Engine, FrameStatus

    class Done:   # a frame event that has completed; its writer thread is slow to look at it
        def __init__(self, delay):
            self.delay = delay

        def query(self):
            return True

        def synchronize(self):
            if threading.current_thread() is not threading.main_thread():
                time.sleep(self.delay)

    class Model:
        def __init__(self):
            self.eng = Engine.__new__(Engine)
            self.eng._recent, self.eng._unreported = [], []
            self.n, self.last = 0, None

        def infer(self, x, f_px=None):
            self.eng.check_status(block=False)          # as DepthPro.infer before each call
            words = torch.tensor([0, 7 if self.n == 1 else 0], dtype=torch.int32)
            st = FrameStatus(self.n, words, Done(0.5 if self.n == 1 else 0.0))
            self.eng._recent.append(st)
            self.last = BatchStatus([st])
            self.n += 1
            return {"depth": torch.full(x.shape[:2], 2.0), "focallength_px": torch.tensor(1000.0)}

        def last_status(self):
            return self.last

    src = tmp_path / "frames"
    src.mkdir()
    for k in range(3):
        Image.fromarray(np.full((24, 32, 3), 40 * k, np.uint8)).save(src / f"output_{k:04d}.png")
    model = Model()
    n = G.batch_generate_depth_maps(str(src), str(tmp_path / "out"), pattern="output_*.png",
                                    model=(model, lambda im: torch.as_tensor(np.asarray(im))), decode_workers=1,
                                    encode_workers=1)
    assert n == 2
    assert sorted(os.listdir(tmp_path / "out")) == ["output_0000_depth.png", "output_0002_depth.png"]
    assert model.n == 3
    model.eng.check_status(block=True)                  # nothing owed: frame 1 was reported once


# ---- the stage table: option resolution, --resume, the CLI, and every stage in one run -----------------------

_GROUND = {"model": None, "dir": "OUT", "grid": 20, "pct": 5, "rot": None, "resolved": False}
_CLEAN = {"radius": 0.1, "nb": 20}
_CLUSTER = {"eps": 0.2, "min_samples": 5, "height_threshold": 1.3, "max_points": 100000}
_BASE = {"cloud": {}, "ground": _GROUND, "clean": _CLEAN}


def test_resolve_stages_table(tmp_path):
    """Each single flag: the stages that come on and the parameter dicts they get, written out from the `if` blocks
    batch_generate_depth_maps had before the stage table (there: the locals `ground`, `clean`, `cluster`, `shapes`,
    `mesh`, `floor`, None for a stage that is off, and `pointcloud` / `boundary_dir` themselves).  A bad value of a
    stage that is off raises nothing from the loop; one of a stage that is on raises ValueError with the check's message
    (the same on the parent)."""
    want = {
        "pointcloud": {"cloud": {}},
        "normalize_ground": {"cloud": {}, "ground": _GROUND},
        "clean_pointcloud": _BASE,
        "cluster_pointcloud": {**_BASE, "cluster": _CLUSTER},
        "fit_shapes": {**_BASE, "cluster": _CLUSTER, "shapes": {"circularity_threshold": 0.85}},
        "split_l_shapes": {**_BASE, "cluster": _CLUSTER, "shapes": {"circularity_threshold": 0.85, "l_split": True}},
        "mesh_points": {**_BASE, "mesh": {"voxel_size": 0.05, "max_nn": 30}},
        "floor_plan": {**_BASE, "floor": {"resolution": 0.1, "height_threshold": 1.3, "min_area": 0.025}},
    }
    assert G.resolve_stages(output_dir="OUT") == {}
    for flag, stages in want.items():
        got = G.resolve_stages(output_dir="OUT", **{flag: True})
        assert got == stages and list(got) == list(stages), flag
    assert G.resolve_stages(normalize_ground=True)["ground"]["dir"] is None       # a tool asking what a flag turns on
    assert G.resolve_stages(boundary_dir=str(tmp_path)) == {"boundary": {"dir": str(tmp_path), "scores": []}}
    # the values are the options', converted as before; the plane's directory defaults to the output directory
    got = G.resolve_stages(output_dir="OUT", ground_params_dir="GP", grid_size=7, ground_percentile=9, rotation_offset=[1, 2, 3],
                           stray_radius=1, stray_neighbors=3.0, cluster_eps=1, cluster_min_samples=2.0, cluster_height=2,
                           cluster_max_points=0, fit_shapes=True, split_l_shapes=True, circularity_threshold=1,
                           mesh_points=True, voxel_size=1, normals_max_nn=8.0, floor_plan=True, floor_resolution=1,
                           floor_height=float("nan"), floor_min_area=0)
    h = got["floor"].pop("height_threshold")
    assert h != h                                           # NaN: every height
    # repr: 1 is not 1.0 here
    assert repr(got) == repr({"cloud": {}, "ground": {**_GROUND, "dir": "GP", "grid": 7, "pct": 9, "rot": [1, 2, 3]},
                              "clean": {"radius": 1.0, "nb": 3},
                              "cluster": {"eps": 1.0, "min_samples": 2, "height_threshold": 2.0, "max_points": 0},
                              "shapes": {"circularity_threshold": 1.0, "l_split": True},
                              "floor": {"resolution": 1.0, "min_area": 0.0}, "mesh": {"voxel_size": 1.0, "max_nn": 8}})
    bad = {"grid_size": (0, "normalize_ground", "--grid_size must be in"),
           "stray_radius": (-1.0, "clean_pointcloud", "--stray_radius must be finite and > 0"),
           "stray_neighbors": (0, "clean_pointcloud", "--stray_neighbors must be >= 1"),
           "cluster_eps": (0.0, "cluster_pointcloud", "--cluster_eps must be finite and > 0"),
           "cluster_min_samples": (0, "cluster_pointcloud", "--cluster_min_samples must be >= 1"),
           "cluster_max_points": (-1, "cluster_pointcloud", "--cluster_max_points must be >= 0"),
           "circularity_threshold": (float("nan"), "fit_shapes", "--circularity_threshold must not be nan"),
           "voxel_size": (0.0, "mesh_points", "--voxel_size must be finite and > 0"),
           "normals_max_nn": (0, "mesh_points", "--normals_max_nn must be in"),
           "floor_resolution": (float("inf"), "floor_plan", "--floor_resolution must be finite and > 0"),
           "floor_height": (float("inf"), "floor_plan", "--floor_height must be finite"),
           "floor_min_area": (-1.0, "floor_plan", "--floor_min_area must be finite and >= 0")}
    for key, (value, flag, message) in bad.items():
        assert G.batch_generate_depth_maps(str(tmp_path), str(tmp_path / "o"), **{key: value}) == 0      # no frames, no error
        with pytest.raises(ValueError, match=message):
            G.batch_generate_depth_maps(str(tmp_path), str(tmp_path / "o"), **{key: value, flag: True})
    # a stage that another one implies is checked too
    with pytest.raises(ValueError, match="--stray_radius"):
        G.batch_generate_depth_maps(str(tmp_path), str(tmp_path / "o"), floor_plan=True, stray_radius=0.0)
    with pytest.raises(ValueError, match="--boundary_dir must be an existing directory"):
        G.batch_generate_depth_maps(str(tmp_path), str(tmp_path / "o"), boundary_dir=str(tmp_path / "missing"))


_STAGE_FILES = ("_depth.png", "_clean.ply", "_clusters.json", "_shapes.json", "_oriented.ply", "_oriented.json",
                "_floorplan.png", "_floorplan.json")
_EVERY = dict(cleaned=True, clustered=True, shaped=True, oriented=True, floor=True)


def test_plan_frames_every_stage(tmp_path):
    """--resume with every stage on: a frame is done only with all of its stages' files, and `{base}_boundary.json` if it
    has a target; taking any one of them away makes it due again."""
    out, tdir = tmp_path / "out", tmp_path / "targets"
    out.mkdir()
    tdir.mkdir()
    frames = [str(tmp_path / f"f{k}.png") for k in range(2)]
    for k in range(2):
        for s in _STAGE_FILES:
            (out / f"f{k}{s}").write_bytes(b"x")
    (tdir / "f0.npy").write_bytes(b"x")                     # f0 has a target, f1 has none
    (out / "f0_boundary.json").write_bytes(b"x")
    plan = lambda: G.plan_frames(frames, str(out), 1, 0, True, boundary=str(tdir), **_EVERY)      # noqa: E731
    assert plan() == []
    for k in range(2):
        for s in _STAGE_FILES + (("_boundary.json",) if k == 0 else ()):
            os.rename(out / f"f{k}{s}", out / "away")
            assert plan() == [k], (k, s)
            os.rename(out / "away", out / f"f{k}{s}")
    assert plan() == []
    assert G.plan_frames(frames, str(out), 1, 0, False, boundary=str(tdir), **_EVERY) == [0, 1]


def test_cli_passes_every_option(monkeypatch, tmp_path):
    """main() with every stage flag and a non-default value of every numeric option: batch_generate_depth_maps gets exactly
    these keywords and values."""
    import sys

    seen = []
    monkeypatch.setattr(G, "batch_generate_depth_maps", lambda *a, **kw: seen.append((a, kw)) or 0)
    monkeypatch.setattr(G, "_model", lambda *a, **k: pytest.fail("the model was loaded"))
    d = str(tmp_path)
    monkeypatch.setattr(sys, "argv", [
        "generate_depth_maps.py", "--input_dir", d, "--output_dir", d + "/o", "--pattern", "f*.png", "--downscale_factor", "0.5",
        "--half_precision", "--raw", "--pointcloud", "--normalize_ground", "--ground_params_dir", d + "/g", "--rot_x", "1.5",
        "--rot_y", "-2", "--rot_z", "3", "--grid_size", "7", "--ground_percentile", "9", "--clean_pointcloud", "--stray_radius",
        "0.25", "--stray_neighbors", "12", "--cluster_pointcloud", "--cluster_eps", "0.12", "--cluster_min_samples", "6",
        "--cluster_height", "0.5", "--cluster_max_points", "3000", "--fit_shapes", "--split_l_shapes", "--circularity_threshold",
        "0.8", "--mesh_points", "--voxel_size", "0.02", "--normals_max_nn", "16", "--floor_plan", "--floor_resolution", "0.2",
        "--floor_height", "0.75", "--floor_min_area", "0.5", "--boundary_dir", d, "--resume", "--colormap", "jet"])
    G.main()
    assert seen == [((), dict(
        input_dir=d, output_dir=d + "/o", pattern="f*.png", downscale_factor=0.5, half_precision=True, colored=False, cmap="jet",
        pointcloud=True, resume=True, normalize_ground=True, ground_params_dir=d + "/g", grid_size=7, ground_percentile=9,
        rotation_offset=[1.5, -2.0, 3.0], clean_pointcloud=True, stray_radius=0.25, stray_neighbors=12, cluster_pointcloud=True,
        cluster_eps=0.12, cluster_min_samples=6, cluster_height=0.5, cluster_max_points=3000, fit_shapes=True,
        split_l_shapes=True, circularity_threshold=0.8, mesh_points=True, voxel_size=0.02, normals_max_nn=16, floor_plan=True,
        floor_resolution=0.2, floor_height=0.75, floor_min_area=0.5, boundary_dir=d))]
    assert all(type(v) is type(w) for v, w in zip(seen[0][1]["rotation_offset"], [1.5, -2.0, 3.0]))


@pytest.mark.gpu
def test_loop_every_stage(tmp_path, cuda):
    """Shapes with the L-split, mesh points, floor plan and the boundary score in one run: the directory holds exactly the
    files of three runs with one of these branches each (plus the boundary score of the frame with a target), each file
    byte for byte -- but the centroids of {base}_clusters.json, within the cluster table's own bound (test_loop_fit_shapes)."""
    import json

    from test_shapes import GOLDEN, _run_loop

    small = dict(stray_radius=0.25, stray_neighbors=12, cluster_eps=0.12, cluster_min_samples=6, cluster_height=float("nan"),
                 cluster_max_points=3000, ground_params_dir=str(tmp_path / "ground"))
    branches = {"shapes": dict(fit_shapes=True, split_l_shapes=True), "mesh": dict(mesh_points=True), "floor": dict(floor_plan=True)}
    tdir = tmp_path / "targets"
    tdir.mkdir()
    np.save(tdir / "output_0000.npy", np.load(os.path.join(GOLDEN, "golden_ground.npz"))["flat_depth"].astype(np.float32) * 1.5)
    for name, kw in branches.items():
        _run_loop(tmp_path, cuda, tmp_path / name, **kw, **small)
    every = tmp_path / "every"
    _run_loop(tmp_path, cuda, every, fit_shapes=True, split_l_shapes=True, mesh_points=True, floor_plan=True,
              boundary_dir=str(tdir), **small)
    files = {f: tmp_path / name / f for name in branches for f in os.listdir(tmp_path / name)}
    assert {f[len("output_0000"):] for f in files if f.startswith("output_0000")} == {
        "_depth.png", "_clean.ply", "_labels.npy", "_clusters.json", "_shapes.json", "_shapes.txt", "_oriented.ply",
        "_oriented.json", "_floorplan.png", "_floorplan.json"} and len(files) == 20
    assert sorted(os.listdir(every)) == sorted(list(files) + ["output_0000_boundary.json"])
    for f, path in files.items():
        if f.endswith("_clusters.json"):
            a, b = json.load(open(path)), json.load(open(every / f))
            for ca, cb in zip(a["cluster_table"], b["cluster_table"]):
                for axis, (va, vb) in zip("xyz", zip(ca.pop("centroid"), cb.pop("centroid"))):
                    assert abs(va - vb) <= 2 * ca["count"] * 2.0 ** -53 * max(abs(v) for v in ca["bbox"][axis]) + 1e-15
            assert a == b and len(a["cluster_table"]) > 0
            continue
        assert open(path, "rb").read() == open(every / f, "rb").read(), f
    js = json.load(open(every / "output_0000_boundary.json"))
    assert js["kind"] == "depth" and (js["H"], js["W"]) == (96, 128) and 0.0 <= js["score"] <= 1.0
    assert json.load(open(every / "output_0000_shapes.json"))["clusters_listed"] > 0
    src = sorted(str(p) for p in (tmp_path / "frames").glob("*.png"))
    assert G.plan_frames(src, str(every), 1, 0, True, boundary=str(tdir), **_EVERY) == []
    assert G.plan_frames(src, str(tmp_path / "mesh"), 1, 0, True, boundary=str(tdir), **_EVERY) == [0, 1]
