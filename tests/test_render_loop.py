"""The frame loop's `views` stage (--render_view): the loop on two small synthetic frames with a stub model whose depth
is on the device.  With --render_view multi the PNG is the restatement's sheet of the cloud the loop wrote and the JSON
its cameras and counts; without the option the loop writes, byte for byte, what the same code writes with the stage
taken out of the list."""

import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import render_numpy as RN  # noqa: E402

H, W, F_PX = 40, 56, 50.0
SIZE = (96, 54)


class _Model:
    def __init__(self, depths, device):
        import torch

        self.depths = [torch.from_numpy(d).to(device) for d in depths]
        self.calls = 0

    def infer(self, x, f_px=None):
        import torch

        d = self.depths[self.calls % len(self.depths)]
        self.calls += 1
        return {"depth": d.clone(), "focallength_px": torch.tensor(F_PX, device=d.device)}


def _transform(im):
    import torch

    return torch.as_tensor(np.asarray(im))


@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    from PIL import Image

    src = tmp_path_factory.mktemp("view_frames")
    rng = np.random.default_rng(43)
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2)]
    yy, xx = np.mgrid[0:H, 0:W]
    depths = []
    for k in range(2):
        d = (4.0 - 0.03 * yy + 0.3 * rng.random((H, W))).astype(np.float32)
        d[10 + k:24, 20:34 + k] = 1.5                                 # a box in front of the slope
        d[3, 5] = 0.0                                                 # a pixel the back-projection drops
        depths.append(d)
    for k, im in enumerate(images):
        Image.fromarray(im, "RGB").save(src / f"frame_{k:04d}.png")
    return str(src), images, depths


def _loop(G, cuda, frames, out, **options):
    src, _, depths = frames
    return G.batch_generate_depth_maps(src, str(out), pattern="frame_*.png", model=(_Model(depths, cuda), _transform),
                                       decode_workers=1, encode_workers=1, **options)


def _ply_vertices(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    n = int([ln for ln in head.decode().splitlines() if ln.startswith("element vertex")][0].split()[-1])
    rec = np.frombuffer(body, np.uint8).reshape(n, 27)
    return rec[:, :24].copy().view(np.float64).reshape(n, 3), rec[:, 24:].copy()


@pytest.mark.gpu
def test_render_view_multi_writes_the_restatement_of_the_cloud_it_wrote(tmp_path, cuda, frames):
    from PIL import Image

    import generate_depth_maps as G

    assert _loop(G, cuda, frames, tmp_path, pointcloud=True, render_view="multi", render_size="96x54", render_point_size=5) == 2
    assert sorted(os.listdir(tmp_path)) == sorted(f"frame_{k:04d}_{s}" for k in range(2)
                                                   for s in ("depth.png", "points.ply", "view.json", "view.png"))
    for k in range(2):
        xyz, rgb = _ply_vertices(tmp_path / f"frame_{k:04d}_points.ply")
        assert len(xyz) == H * W - 1
        want = RN.render_views(xyz, rgb, RN.SHEET, SIZE, 5, sheet=True)
        im = Image.open(tmp_path / f"frame_{k:04d}_view.png")
        assert im.mode == "RGB" and im.size == (2 * SIZE[0], 2 * SIZE[1]) and np.array_equal(np.asarray(im), want["image"])
        assert 0 < min(want["stats"]["covered_pixels"])
        js = json.load(open(tmp_path / f"frame_{k:04d}_view.json"))
        assert js["parameters"] == {"view": "multi", "size": list(SIZE), "point_size": 5, "min_height": None}
        assert js["views"] == list(RN.SHEET) and js["counts"] == want["stats"]
        assert np.array_equal(np.array(js["cameras"], np.float64).view(np.uint64), want["cameras"].view(np.uint64))
    # --resume: a frame without its picture is done again, the other is not
    os.remove(tmp_path / "frame_0001_view.png")
    assert _loop(G, cuda, frames, tmp_path, pointcloud=True, render_view="multi", render_size="96x54", render_point_size=5,
                 resume=True) == 1


@pytest.mark.gpu
def test_render_view_plan_of_one_frame(tmp_path, cuda, frames):
    from PIL import Image

    import generate_depth_maps as G

    assert _loop(G, cuda, frames, tmp_path, render_view="plan", render_size="96x54", render_min_height=-0.5) == 2   # implies the cloud
    xyz, rgb = _ply_vertices(tmp_path / "frame_0000_points.ply")
    want = RN.render_views(xyz, rgb, ("plan",), SIZE, 7, min_height=-0.5)
    assert np.array_equal(np.asarray(Image.open(tmp_path / "frame_0000_view.png")), want["image"][0])
    js = json.load(open(tmp_path / "frame_0000_view.json"))
    assert js["counts"] == want["stats"] and 0 < want["stats"]["clipped"][0] < len(xyz) and js["cameras"][0][6] == -0.5


@pytest.mark.gpu
def test_without_the_option_the_files_are_those_of_the_loop_without_the_stage(tmp_path, cuda, frames, monkeypatch):
    import generate_depth_maps as G

    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    options = dict(pointcloud=True, anaglyph=True, depth_shadows=True)
    assert _loop(G, cuda, frames, a, **options) == 2
    assert _loop(G, cuda, frames, c, **options, render_view="front", render_size="96x54") == 2
    with monkeypatch.context() as m:
        m.setattr(G, "STAGES", tuple(st for st in G.STAGES if st.name != "views"))
        assert "views" not in [st.name for st in G.STAGES]
        assert _loop(G, cuda, frames, b, **options) == 2
    names = sorted(f"frame_{k:04d}_{s}" for k in range(2) for s in ("anaglyph.png", "depth.png", "points.ply", "shadows.json", "shadows.png"))
    assert sorted(os.listdir(a)) == names and sorted(os.listdir(b)) == names
    assert sorted(os.listdir(c)) == sorted(names + [f"frame_{k:04d}_view.{e}" for k in range(2) for e in ("png", "json")])
    for name in names:
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
        assert (a / name).read_bytes() == (c / name).read_bytes(), name
