"""The frame loop's `slices` stage (--floor_slices): run through the loop's own stage functions on the synthetic room of
tests/golden/golden_slices.npz, it writes `{frame}_floorslices.txt` and `{frame}_floorslices.json`, whose closing sizes
and polygon counts are the summary's; and with --floor_polygons also on, `{frame}_floorplan.txt` (and the plan's picture and JSON) is byte for byte
what a run without --floor_slices writes.  `{frame}_floorplan_polygons.json` holds the mean height at full precision, an
fp64 sum in an unspecified order, so two runs of it agree within twice test_outline.py's MEAN_REL
and in everything else exactly."""

import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _run(G, params, xyz, base):
    """Queue and write the stages of `params` (in the table's order) for one frame whose cleaned cloud is `xyz`."""
    import torch

    on = [st for st in G.STAGES if st.name in params and st.name not in ("cloud", "ground", "clean")]
    frame = {"xyz": xyz, "cols": None, "count": None}
    out = {st.name: st.queue(frame, params[st.name]) for st in on}
    torch.cuda.synchronize()
    for st in on:
        if st.write is not None and out.get(st.name) is not None:
            st.write(base, params, out)
    return out


@pytest.mark.gpu
def test_slices_stage_writes_both_files_and_leaves_the_polygons_file_alone(tmp_path, cuda):
    import torch

    import generate_depth_maps as G
    from depth_pro import pointcloud as PC

    xyz = torch.from_numpy(np.load(os.path.join(GOLDEN, "golden_slices.npz"))["room_points"]).to(cuda)
    with_slices = G.resolve_stages(output_dir=str(tmp_path), floor_slices=5, floor_polygons=True)
    without = G.resolve_stages(output_dir=str(tmp_path), floor_polygons=True)
    assert list(with_slices) == ["cloud", "ground", "clean", "floor", "slices", "polygons"] and "slices" not in without
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    out = _run(G, with_slices, xyz, str(tmp_path / "a" / "f"))
    _run(G, without, xyz, str(tmp_path / "b" / "f"))
    assert sorted(os.listdir(tmp_path / "a")) == ["f_floorplan.json", "f_floorplan.png", "f_floorplan.txt",
                                                  "f_floorplan_polygons.json", "f_floorslices.json", "f_floorslices.txt"]
    assert sorted(os.listdir(tmp_path / "b")) == ["f_floorplan.json", "f_floorplan.png", "f_floorplan.txt", "f_floorplan_polygons.json"]
    for name in ("f_floorplan.txt", "f_floorplan.png", "f_floorplan.json"):
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes(), name
    pa, pb = (json.load(open(tmp_path / d / "f_floorplan_polygons.json")) for d in "ab")
    ha, hb = pa.pop("height"), pb.pop("height")
    assert pa == pb and abs(ha - hb) <= 2 * 1.4e-15 * abs(hb)
    assert len((tmp_path / "b" / "f_floorplan.txt").read_text().splitlines()) > 5
    js = json.load(open(tmp_path / "a" / "f_floorslices.json"))
    summary = PC.sliced_floor_plan_summary(out["slices"])
    assert [sl["close_size"] for sl in js["slices"]] == [sl["close_size"] for sl in summary["slices"]] == [3, 5, 3, 5, 5]
    assert [len(sl["polygons"]) for sl in js["slices"]] == [len(sl["polygons"]) for sl in summary["slices"]] == [3, 2, 0, 2, 2]
    assert js == json.loads(json.dumps(summary)) and js["parameters"]["num_slices"] == 5
    lines = (tmp_path / "a" / "f_floorslices.txt").read_text().splitlines()
    assert len(lines) == 5 + 9 and [float(l.split(", ")[0]) for l in lines[5:]] == sorted(float(l.split(", ")[0]) for l in lines[5:])
