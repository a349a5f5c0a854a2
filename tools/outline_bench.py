"""GPU time of the floor-plan polygons (dp_region_outlines, dp_simplify_outlines), from stream events.

    python tools/outline_bench.py [--size 3840x2160] [--iters 10] [--repeats 3] [--json out.json]

Two plans, each made once by `floor_plan` at the loop's defaults (resolution 0.1 m, padding 0.2 m, closing 7 x 7 twice,
opening 3 x 3): the synthetic 3840 x 2160 terrain of tools/floorplan_bench.py, levelled and cleaned, over every height
(one large region), and "furniture": 40 x 40 boxes of 0.45 m on a 1.5 m lattice at 2 m height (1600 small regions;
the gaps are wider than the 7 x 7 closing bridges).
Per repeat: 2 warm-up calls, then `iters` timed calls between two events on the current stream, for `region_outlines`,
`simplify_outlines` and `grid_regions` (the stage in front, for comparison); the wrappers' allocations are inside the
timed region (torch's caching allocator after the warm-up).
"""

import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "ml-depth-pro-video_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    sys.path.insert(0, p)

RES, PAD = 0.1, 0.2


def furniture(g):
    """1600 boxes of 0.45 m x 0.45 m, 150 points each, on a 1.5 m lattice at a height of about 2 m."""
    cx, cz = np.meshgrid(1.5 * np.arange(40.0), 1.5 * np.arange(40.0))
    xz = np.stack([cx.ravel(), cz.ravel()], axis=1)[:, None, :] + g.uniform(0.0, 0.45, (1600, 150, 2))
    return np.column_stack([xz[..., 0].ravel(), g.uniform(1.8, 2.2, 1600 * 150), xz[..., 1].ravel()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160", help="WxH of the terrain frame")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
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
    clouds = {"terrain": (xyz, count, float("nan")),
              "furniture": (torch.from_numpy(furniture(np.random.default_rng(3))).to(dev), None, 1.3)}
    res = {"size": args.size, "iters": args.iters, "repeats": args.repeats, "resolution": RES, "padding": PAD, "plans": {}}
    for name, (pts, cnt, thr) in clouds.items():
        plan = PC.floor_polygons(PC.floor_plan(pts, None, cnt, height_threshold=thr, resolution=RES, padding=PAD), pts, cnt)
        s = PC.floor_polygons_summary(plan)
        out = {"grid": [int(s["outline_stats"]["height"]), int(s["outline_stats"]["width"])], "outline_stats": s["outline_stats"],
               "polygon_stats": s["polygon_stats"], "height": s["height"],
               "largest_outline": int(plan["outline_columns"][:, 1].max().item()),
               "grid_regions_ms": [], "region_outlines_ms": [], "simplify_outlines_ms": []}
        g = plan
        for _ in range(args.repeats):
            out["grid_regions_ms"].append(timed(lambda: PC.grid_regions(g["cleaned"], g["dims"], g["density"], g["height"],
                                                                        g["origin"], RES), args.iters))
            out["region_outlines_ms"].append(timed(lambda: PC.region_outlines(g), args.iters))
            out["simplify_outlines_ms"].append(timed(lambda: PC.simplify_outlines(g), args.iters))
        res["plans"][name] = out
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
