"""The frame loop's `shadows` stage (--depth_shadows, --drop_depth_shadows): the loop on two small synthetic frames with
a stub model whose depth is on the device.  The PNG is the restatement's mask and the JSON its counts; with
--pointcloud --drop_depth_shadows the PLY holds exactly the rows of the unmasked pixels, in row-major order; without
the new options the loop writes what a plain run of it writes, byte for byte."""

import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import shadows_numpy as SN  # noqa: E402

H, W, F_PX = 48, 72, 60.0
THR, MIN_REGION = 0.25, 40


class _Model:
    """Stands in for DepthPro: frame k of the sorted list gets depths[k] (the loop runs the frames in order)."""

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

    src = tmp_path_factory.mktemp("shadow_frames")
    rng = np.random.default_rng(41)
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2)]
    depths = [SN.scene(H, W, 50 + k) for k in range(2)]
    depths[1][5, 7] = 0.0                                     # a pixel the back-projection drops by itself
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
    return rec[:, :24].copy().view(np.float64).reshape(n, 3), rec[:, 24:]


@pytest.mark.gpu
def test_depth_shadows_png_and_json_are_the_restatements(tmp_path, cuda, frames):
    from PIL import Image

    import generate_depth_maps as G

    assert _loop(G, cuda, frames, tmp_path, depth_shadows=True, shadow_threshold=THR, shadow_min_region=MIN_REGION) == 2
    assert sorted(os.listdir(tmp_path)) == sorted(f"frame_{k:04d}_{s}" for k in range(2) for s in ("depth.png", "shadows.json", "shadows.png"))
    for k, depth in enumerate(frames[2]):
        want, stats = SN.find_depth_shadows(depth, THR, MIN_REGION)
        assert 0 < want.sum() < want.size
        im = Image.open(tmp_path / f"frame_{k:04d}_shadows.png")
        assert im.mode == "L" and np.array_equal(np.asarray(im), want.astype(np.uint8) * 255)
        js = json.load(open(tmp_path / f"frame_{k:04d}_shadows.json"))
        assert js["parameters"] == {"threshold_factor": THR, "min_region_size": MIN_REGION, "drop": False}
        assert js["counts"] == {n: v for n, v in stats.items() if n != "gmax"} and (js["H"], js["W"]) == (H, W)
        assert np.float32(js["gmax"]) == np.float32(stats["gmax"]) and js["nonfinite"] == 0
    # --resume: a frame without its mask is done again, the other is not
    os.remove(tmp_path / "frame_0001_shadows.png")
    assert _loop(G, cuda, frames, tmp_path, depth_shadows=True, shadow_threshold=THR, shadow_min_region=MIN_REGION, resume=True) == 1


@pytest.mark.gpu
def test_drop_depth_shadows_leaves_exactly_the_unmasked_rows(tmp_path, cuda, frames):
    import generate_depth_maps as G

    _, images, depths = frames
    plain, dropped = tmp_path / "plain", tmp_path / "dropped"
    assert _loop(G, cuda, frames, plain, pointcloud=True) == 2
    assert _loop(G, cuda, frames, dropped, pointcloud=True, drop_depth_shadows=True, shadow_threshold=THR,
                 shadow_min_region=MIN_REGION) == 2
    assert sorted(os.listdir(dropped)) == sorted(f"frame_{k:04d}_{s}" for k in range(2)
                                                  for s in ("depth.png", "points.ply", "shadows.json", "shadows.png"))
    for k, depth in enumerate(depths):
        mask = SN.find_depth_shadows(depth, THR, MIN_REGION)[0]
        valid = depth > 0
        all_xyz, all_rgb = _ply_vertices(plain / f"frame_{k:04d}_points.ply")
        xyz, rgb = _ply_vertices(dropped / f"frame_{k:04d}_points.ply")
        assert len(all_xyz) == int(valid.sum())
        keep = ~mask[valid]                                    # the plain cloud's rows are the valid pixels, row-major
        assert 0 < keep.sum() < len(keep) and len(xyz) == int((valid & ~mask).sum())
        assert np.array_equal(xyz.view(np.uint64), all_xyz[keep].view(np.uint64)) and np.array_equal(rgb, all_rgb[keep])
        assert np.array_equal(rgb, images[k][valid & ~mask])
        assert np.array_equal(xyz[:, 2].astype(np.float32), depth[valid & ~mask])       # z is the depth itself
        assert json.load(open(dropped / f"frame_{k:04d}_shadows.json"))["parameters"]["drop"] is True
        assert (dropped / f"frame_{k:04d}_depth.png").read_bytes() == (plain / f"frame_{k:04d}_depth.png").read_bytes()


@pytest.mark.gpu
def test_without_the_options_the_files_are_those_of_a_plain_run(tmp_path, cuda, frames):
    """The same options with and without the shadows stage beside them: every file both runs write is byte-identical,
    and a run without the new options writes no other file than before."""
    import generate_depth_maps as G

    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    assert _loop(G, cuda, frames, a, pointcloud=True, anaglyph=True) == 2
    assert _loop(G, cuda, frames, b, pointcloud=True, anaglyph=True, depth_shadows=True) == 2
    assert _loop(G, cuda, frames, c) == 2
    names = sorted(f"frame_{k:04d}_{s}" for k in range(2) for s in ("anaglyph.png", "depth.png", "points.ply"))
    assert sorted(os.listdir(a)) == names
    assert sorted(os.listdir(b)) == sorted(names + [f"frame_{k:04d}_shadows.{e}" for k in range(2) for e in ("png", "json")])
    assert sorted(os.listdir(c)) == [f"frame_{k:04d}_depth.png" for k in range(2)]
    for name in names:
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    for k in range(2):
        assert (c / f"frame_{k:04d}_depth.png").read_bytes() == (a / f"frame_{k:04d}_depth.png").read_bytes()
