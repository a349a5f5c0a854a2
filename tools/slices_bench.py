"""GPU time of the height-sliced floor plan (dp_slice_grids, dp_slice_closing_sizes, dp_slice_morphology and the
per-slice dp_grid_regions + dp_region_outlines + dp_simplify_outlines_with), from stream events.

    python tools/slices_bench.py [--size 3840x2160] [--iters 10] [--repeats 3] [--json out.json]

The synthetic 3840 x 2160 terrain of tools/floorplan_bench.py, levelled and cleaned, at `PC.sliced_floor_plan`'s
defaults (5 slices between 0.1 m and 2.5 m, resolution 0.05 m, padding 0.5 m, min_area 0.1, alpha 0.01).  Per repeat: 2
warm-up calls, then `iters` timed calls between two events on the current stream (tools/outline_bench.py's protocol);
the wrappers' allocations are inside the timed region (torch's caching allocator after the warm-up).  The yardstick is
one `occupancy_grid` over every height on the same cloud in the same process: five separate rasters would cost at
least five of these.
"""

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "ml-depth-pro-video_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    sys.path.insert(0, p)

LAUNCHES_PER_SLICE = 11 + 5 + 3          # dp_grid_regions (a grid of more than 2048 cells), dp_region_outlines, dp_simplify_outlines_with


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160", help="WxH of the terrain frame")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--slices", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    from ground_numpy import terrain

    import torch

    from depth_pro import pointcloud as PC
    from ground_bench import timed

    dev = torch.device("cuda:0")
    depth, f = terrain(h, w, 7)
    xyz, _, _, count = PC.depth_to_points_async(torch.from_numpy(depth).to(dev), f, w, h)
    model = PC.fit_ground_plane(xyz, count)
    xyz, _ = PC.normalize_to_ground(xyz, model, count)
    xyz, _ = PC.ground_adjust(xyz, 20, 5, count)
    xyz, _, count = PC.clean_pointcloud(xyz, None, count)[:3]
    S = args.slices
    plan = PC.sliced_floor_plan(xyz, count, num_slices=S)
    s = PC.sliced_floor_plan_summary(plan)
    p = plan["parameters"]

    def per_slice():
        for sub in plan["slices"]:
            PC.grid_regions(sub["cleaned"], sub["dims"], sub["density"], sub["height"], sub["origin"], p["resolution"])
            PC.region_outlines(sub)
            PC.simplify_outlines_with(sub, p["min_area"], p["alpha"])

    calls = {
        "slice_grids_ms": lambda: PC.slice_grids(xyz, count, num_slices=S),
        "occupancy_grid_every_height_ms": lambda: PC.occupancy_grid(xyz, None, count, None, p["resolution"], p["padding"], 1 << 20),
        "slice_closing_sizes_ms": lambda: PC.slice_closing_sizes(plan["occupied"], plan["dims"]),
        "slice_morphology_ms": lambda: PC.slice_morphology(plan["occupied"], plan["dims"], plan["close_size"], 1, p["open_size"]),
        "per_slice_regions_outlines_simplify_ms": per_slice,
        "sliced_floor_plan_ms": lambda: PC.sliced_floor_plan(xyz, count, num_slices=S),
    }
    res = {"size": args.size, "iters": args.iters, "repeats": args.repeats, "cleaned_points": int(count.item()), "parameters": p,
           "per_slice_launches": S * LAUNCHES_PER_SLICE,
           "slices": [{k: sl[k] for k in ("index", "lo", "hi", "participants", "status", "grid", "set_cells", "components", "close_size")}
                      | {"regions": sl["region_stats"]["regions"], "polygons": len(sl["polygons"])} for sl in s["slices"]]}
    for k in calls:
        res[k] = []
    for _ in range(args.repeats):
        for k, call in calls.items():
            res[k].append(timed(call, args.iters))
    res["slice_grids_over_occupancy_grid"] = min(res["slice_grids_ms"]) / min(res["occupancy_grid_every_height_ms"])
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
