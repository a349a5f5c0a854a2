"""The frame loop's `anaglyph` and `parallax` stages (--anaglyph, --parallax) and the single-image script
depth_video_effect.py: run through the loop's own stage functions on a stub frame whose depth and image are on the
device, the PNGs decode to the arrays of `depth_pro.effects`; with --floor_polygons also on, the files of the other stages
are byte for byte those of a run without the new options (`{frame}_floorplan_polygons.json` but for its mean height, an
fp64 sum in an unspecified order: tests/test_slices_loop.py); the whole loop takes the phase from the frame's position in
the sorted list; the script's functions run with a stub model."""

import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import effects_numpy as FX  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SKIP = ("cloud", "ground", "clean")


def _run(G, params, frame, base):
    """Queue and write the stages of `params` (in the table's order) for one frame (tests/test_slices_loop.py: _run)."""
    import torch

    on = [st for st in G.STAGES if st.name in params and st.name not in SKIP]
    out = {st.name: st.queue(frame, params[st.name]) for st in on}
    torch.cuda.synchronize()
    for st in on:
        if st.write is not None and out.get(st.name) is not None:
            st.write(base, params, out)
    return out


def _png(path):
    from PIL import Image

    im = Image.open(path)
    assert im.mode == "RGB"
    return np.asarray(im)


class _Model:
    """Stands in for DepthPro: the same device depth map for every frame."""

    def __init__(self, depth):
        self.depth = depth

    def infer(self, x, f_px=None):
        import torch

        return {"depth": self.depth.clone(), "focallength_px": torch.tensor(30.0, device=self.depth.device)}


def _transform(im):
    import torch

    return torch.as_tensor(np.asarray(im))


@pytest.mark.gpu
def test_stages_write_the_api_arrays(tmp_path, cuda, capsys):
    import torch

    import generate_depth_maps as G
    from depth_pro import effects as E

    image, depth = FX.scene(24, 40, 21)
    d = torch.from_numpy(depth).to(cuda)
    params = G.resolve_stages(output_dir=str(tmp_path), anaglyph=True, anaglyph_separation=0.04, parallax="circle",
                              parallax_amplitude=0.08)
    assert list(params) == ["anaglyph", "parallax"]
    frame = {"depth": d, "image": torch.from_numpy(image).pin_memory(), "index": 163, "path": "f.png", "world": 1, "rank": 0}
    _run(G, params, frame, str(tmp_path / "f"))
    assert sorted(os.listdir(tmp_path)) == ["f_anaglyph.png", "f_parallax.png"]
    assert frame["rgb"].is_cuda                                               # uploaded once for both stages
    assert np.array_equal(_png(tmp_path / "f_anaglyph.png"), E.anaglyph(image, d, 0.04)[0].cpu().numpy())
    assert np.array_equal(_png(tmp_path / "f_anaglyph.png"), FX.anaglyph(image, depth, 0.04)[0])
    view = E.view_params("circle", 0.08, 40, 24, 163 % 150, 150)
    assert np.array_equal(_png(tmp_path / "f_parallax.png"), E.warp_views(image, d, [view])[0][0].cpu().numpy())
    assert np.array_equal(_png(tmp_path / "f_parallax.png"), FX.warp_view(image, depth, tuple(view))[0])
    assert "written black" not in capsys.readouterr().out
    holed = depth.copy()
    holed[3, 5:8] = np.nan                                                    # a numpy image this time
    _run(G, params, {"depth": torch.from_numpy(holed).to(cuda), "image": image, "index": 0}, str(tmp_path / "g"))
    text = capsys.readouterr().out
    assert "g_anaglyph.png: 3 pixels" in text and "g_parallax.png: 3 pixels" in text
    assert np.array_equal(_png(tmp_path / "g_anaglyph.png"), FX.anaglyph(image, holed, 0.04)[0])


@pytest.mark.gpu
def test_other_stages_files_do_not_change(tmp_path, cuda):
    import torch

    import generate_depth_maps as G

    xyz = torch.from_numpy(np.load(os.path.join(GOLDEN, "golden_slices.npz"))["room_points"]).to(cuda)
    image, depth = FX.scene(24, 40, 22)
    with_fx = G.resolve_stages(output_dir=str(tmp_path), floor_polygons=True, anaglyph=True, parallax="swing")
    without = G.resolve_stages(output_dir=str(tmp_path), floor_polygons=True)
    assert list(with_fx) == ["cloud", "ground", "clean", "floor", "anaglyph", "parallax", "polygons"]
    assert list(without) == ["cloud", "ground", "clean", "floor", "polygons"]
    for d, params in (("a", with_fx), ("b", without)):
        (tmp_path / d).mkdir()
        frame = {"xyz": xyz, "cols": None, "count": None, "depth": torch.from_numpy(depth).to(cuda), "image": image, "index": 7}
        _run(G, params, frame, str(tmp_path / d / "f"))
    plan_files = ["f_floorplan.json", "f_floorplan.png", "f_floorplan.txt", "f_floorplan_polygons.json"]
    assert sorted(os.listdir(tmp_path / "a")) == sorted(plan_files + ["f_anaglyph.png", "f_parallax.png"])
    assert sorted(os.listdir(tmp_path / "b")) == plan_files
    for name in ("f_floorplan.txt", "f_floorplan.png", "f_floorplan.json"):
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes(), name
    pa, pb = (json.load(open(tmp_path / d / "f_floorplan_polygons.json")) for d in "ab")
    ha, hb = pa.pop("height"), pb.pop("height")
    assert pa == pb and abs(ha - hb) <= 2 * 1.4e-15 * abs(hb)


@pytest.mark.gpu
def test_loop_takes_the_phase_from_the_position_in_the_sorted_list(tmp_path, cuda):
    import torch
    from PIL import Image

    import generate_depth_maps as G
    from depth_pro import effects as E

    image, depth = FX.scene(24, 40, 23)
    src, out, plain = tmp_path / "src", tmp_path / "out", tmp_path / "plain"
    src.mkdir()
    for k in range(3):
        Image.fromarray(image, "RGB").save(src / f"output_{k:04d}.png")
    d = torch.from_numpy(depth).to(cuda)
    kw = dict(pattern="output_*.png", model=(_Model(d), _transform), decode_workers=1, encode_workers=1)
    assert G.batch_generate_depth_maps(str(src), str(out), anaglyph=True, parallax="circle", parallax_amplitude=0.3,
                                       parallax_period=2, **kw) == 3
    assert G.batch_generate_depth_maps(str(src), str(plain), **kw) == 3
    assert sorted(os.listdir(plain)) == [f"output_{k:04d}_depth.png" for k in range(3)]
    assert sorted(os.listdir(out)) == sorted(f"output_{k:04d}_{s}.png" for k in range(3) for s in ("anaglyph", "depth", "parallax"))
    for k in range(3):
        assert (out / f"output_{k:04d}_depth.png").read_bytes() == (plain / f"output_{k:04d}_depth.png").read_bytes()
        want = FX.warp_view(image, depth, FX.view_params("circle", 0.3, 40, 24, k % 2, 2))[0]
        assert np.array_equal(_png(out / f"output_{k:04d}_parallax.png"), want), k
        assert np.array_equal(_png(out / f"output_{k:04d}_anaglyph.png"), FX.anaglyph(image, depth, 0.05)[0]), k
    assert not np.array_equal(_png(out / "output_0000_parallax.png"), _png(out / "output_0001_parallax.png"))
    # --resume: a frame without its parallax file is done again, the others are not
    os.remove(out / "output_0001_parallax.png")
    assert G.batch_generate_depth_maps(str(src), str(out), anaglyph=True, parallax="circle", parallax_amplitude=0.3,
                                       parallax_period=2, resume=True, **kw) == 1
    assert np.array_equal(_png(out / "output_0001_parallax.png"), E.warp_views(
        image, d, [E.view_params("circle", 0.3, 40, 24, 1, 2)])[0][0].cpu().numpy())


@pytest.mark.gpu
def test_single_image_script_with_a_stub_model(tmp_path, cuda):
    import torch
    from PIL import Image

    import depth_video_effect as S

    image, depth = FX.scene(24, 40, 24)
    Image.fromarray(image, "RGB").save(tmp_path / "in.png")
    model = (_Model(torch.from_numpy(depth).to(cuda)), _transform)
    got = S.create_3d_anaglyph(str(tmp_path / "in.png"), str(tmp_path / "ana.png"), separation=0.03, model=model)
    want = FX.anaglyph(image, depth, 0.03)[0]
    assert np.array_equal(got, want) and np.array_equal(_png(tmp_path / "ana.png"), want)
    files = S.create_parallax_effect(str(tmp_path / "in.png"), str(tmp_path / "video.mp4"), duration=1.0, fps=10, amplitude=0.06,
                                     motion_type="swing", model=model)
    assert files == [str(tmp_path / "video_frames" / f"frame_{f:05d}.png") for f in range(10)]        # two chunks of views
    assert sorted(os.listdir(tmp_path / "video_frames")) == [os.path.basename(f) for f in files]
    want = FX.warp_views(image, depth, [FX.view_params("swing", 0.06, 40, 24, f, 10) for f in range(10)])[0]
    for f, path in enumerate(files):
        assert np.array_equal(_png(path), want[f]), f
    with pytest.raises(ValueError, match="scale"):
        S.create_parallax_effect(str(tmp_path / "in.png"), str(tmp_path / "v.mp4"), resolution_scale=0.5, model=model)
    with pytest.raises(ValueError, match="Unknown motion type"):
        S.create_parallax_effect(str(tmp_path / "in.png"), str(tmp_path / "v.mp4"), motion_type="spiral", model=model)
