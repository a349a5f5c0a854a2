"""The frame loop's `planshapes` stage (--plan_shapes): the loop of tests/test_shapes.py (two small frames, a stub model
whose depth is on the device) with the option, with and without --split_l_shapes.  `{frame}_plan.png` is the restatement
(tests/overlay_numpy.py) drawn with the device's records over the plan of the cloud the stage was given; without the
option the loop writes the files it wrote before.

Byte for byte, but for the centroids of `{frame}_clusters.json`: the cluster table accumulates them in an unspecified
order (the ABI 17 contract), so two runs of the same code may differ there, within the bound tests/test_shapes.py uses;
the rest of that file is compared with ==, and every other file, `{frame}_shapes.json` and `.txt` included, by bytes."""

import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import overlay_numpy as ON  # noqa: E402

KW = dict(stray_radius=0.25, stray_neighbors=12, cluster_eps=0.12, cluster_min_samples=6, cluster_max_points=3000,
          circularity_threshold=0.8)
PLAN = dict(plan_shapes=True, plan_size="160x96", plan_point_size=3)


def _spy(monkeypatch):
    import generate_depth_maps as G

    calls, real = [], G.OV.plan_with_shapes

    def plan_with_shapes(*args, **kw):
        res = real(*args, **kw)
        calls.append((args, kw, res))
        return res

    monkeypatch.setattr(G.OV, "plan_with_shapes", plan_with_shapes)
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("split,height", [(False, float("nan")), (True, 0.5)])
def test_plan_shapes_writes_the_restatement_over_the_device_records(tmp_path, cuda, monkeypatch, split, height):
    from PIL import Image

    import test_shapes as TS
    from depth_pro import overlay as OV
    from depth_pro import render as R

    calls = _spy(monkeypatch)
    out = tmp_path / "out"
    options = dict(KW, cluster_height=height, **PLAN, **({"split_l_shapes": True} if split else {}))
    TS._run_loop(tmp_path, cuda, out, **options)                                        # --plan_shapes implies --fit_shapes
    stems = ("clean.ply", "clusters.json", "depth.png", "labels.npy", "plan.json", "plan.png", "shapes.json", "shapes.txt")
    assert sorted(os.listdir(out)) == sorted([f"output_{k:04d}_{s}" for k in range(2) for s in stems] + ["ground.json"])
    assert len(calls) == 2
    for k, (args, kw, res) in enumerate(calls):
        xyz, cols, count, rects, n_rects, shapes, n_clusters = args
        assert kw == dict(size=(160, 96), point_size=3, min_height=None if split is False else 0.5, stroke=3.0, label_scale=2)
        assert tuple(rects.shape[1:]) == (8,) and n_rects.numel() == (2 if split else 1) and tuple(shapes.shape) == (4096, 16)
        got = OV.overlay_summary(res)
        plan = R.render_views(xyz, cols, views="plan", size=kw["size"], point_size=3, count=count, min_height=kw["min_height"])
        base = plan["image"][0].cpu().numpy()
        want, painted = ON.draw(base, got["records"], 3.0, 230, 2)
        im = Image.open(out / f"output_{k:04d}_plan.png")
        assert im.mode == "RGB" and im.size == (160, 96) and np.array_equal(np.asarray(im), want)
        assert got["stats"] == ON.stats_of(got["records"], painted) and got["stats"]["rectangles"] > 0 and (want != base).any()
        js = json.load(open(out / f"output_{k:04d}_plan.json"))
        assert js["parameters"] == {"size": [160, 96], "point_size": 3, "min_height": kw["min_height"], "stroke": 3.0, "alpha": 230,
                                    "label_scale": 2, "split_l_shapes": split}
        assert js["counts"] == got["stats"] and js["plan_counts"] == got["plan_stats"]
        cam = np.array([np.nan if c is None else c for c in js["camera"]])
        assert np.array_equal(cam.view(np.uint64)[[0, 1, 2, 3, 4, 5, 7, 8]], got["camera"].view(np.uint64)[[0, 1, 2, 3, 4, 5, 7, 8]])
        shapes_js = json.load(open(out / f"output_{k:04d}_shapes.json"))
        n_listed = len(shapes_js["rectangles"]) + len(shapes_js["circles"])
        assert len(got["records"]) == n_listed and got["records"][:, 9].tolist() == list(range(1, n_listed + 1))
    # --resume: a frame is skipped only when both new files are there
    os.remove(out / "output_0001_plan.json")
    TS._run_loop(tmp_path, cuda, out, frames=1, resume=True, **options)
    os.remove(out / "output_0000_plan.png")
    TS._run_loop(tmp_path, cuda, out, frames=1, resume=True, **options)
    TS._run_loop(tmp_path, cuda, out, frames=0, resume=True, **options)
    assert len(calls) == 4


def _tables_agree(pa, pb):
    """Two `{frame}_clusters.json`: the centroids within the cluster table's own bound ((count - 1) * 2^-53 * sum |v| of
    the exact sum each, as tests/test_shapes.py takes it), everything else equal."""
    a, b = json.load(open(pa)), json.load(open(pb))
    assert len(a["cluster_table"]) == len(b["cluster_table"])
    for ca, cb in zip(a["cluster_table"], b["cluster_table"]):
        for axis, (va, vb) in zip("xyz", zip(ca.pop("centroid"), cb.pop("centroid"))):
            assert abs(va - vb) <= 2 * ca["count"] * 2.0 ** -53 * max(abs(v) for v in ca["bbox"][axis]) + 1e-15
    assert a == b


@pytest.mark.gpu
def test_without_the_option_the_files_are_those_of_the_loop_without_the_stage(tmp_path, cuda, monkeypatch):
    import generate_depth_maps as G
    import test_shapes as TS

    a, b, c = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    options = dict(KW, cluster_height=float("nan"), fit_shapes=True, split_l_shapes=True)
    TS._run_loop(tmp_path, cuda, a, **options)
    TS._run_loop(tmp_path, cuda, c, ground_params_dir=str(a), **options, **PLAN)
    with monkeypatch.context() as m:                                                    # the option stripped: no such stage at all
        m.setattr(G, "STAGES", tuple(st for st in G.STAGES if st.name != "planshapes"))
        assert "planshapes" not in [st.name for st in G.STAGES]
        TS._run_loop(tmp_path, cuda, b, ground_params_dir=str(a), **options)
    names = sorted(f"output_{k:04d}_{s}" for k in range(2)
                   for s in ("clean.ply", "clusters.json", "depth.png", "labels.npy", "shapes.json", "shapes.txt"))
    assert sorted(set(os.listdir(a)) - {"ground.json"}) == names and sorted(os.listdir(b)) == names
    assert sorted(os.listdir(c)) == sorted(names + [f"output_{k:04d}_plan.{e}" for k in range(2) for e in ("png", "json")])
    for name in names:
        if name.endswith("_clusters.json"):
            _tables_agree(a / name, b / name)
            _tables_agree(a / name, c / name)
            continue
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
        assert (a / name).read_bytes() == (c / name).read_bytes(), name


def test_the_loop_knows_the_option_and_the_library_the_entry_point():
    """What the parent commit lacks: the module, the entry point, the loop's option."""
    import inspect

    import generate_depth_maps as G
    from depth_pro import _lib
    from depth_pro import overlay as OV

    assert hasattr(_lib.load(), "dp_overlay_shapes") and callable(OV.plan_with_shapes)
    assert inspect.signature(G.batch_generate_depth_maps).parameters["plan_shapes"].default is False
    assert "planshapes" in [st.name for st in G.STAGES]
