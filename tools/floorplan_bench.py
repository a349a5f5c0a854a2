"""GPU time of the occupancy floor plan (dp_occupancy_grid, dp_grid_morphology, dp_grid_regions, dp_floorplan_image),
from stream events.

    python tools/floorplan_bench.py [--size 3840x2160] [--iters 10] [--repeats 3] [--json out.json] [--host]

The synthetic 3840 x 2160 terrain of tools/cluster_bench.py, levelled and cleaned, rasterised at the loop's defaults
(resolution 0.1 m, padding 0.2 m, closing 7 x 7 twice, opening 3 x 3) over every height (the terrain has little above
1.3 m; --height sets a threshold).  Per repeat: 2 warm-up calls, then `iters` timed calls between two events on the
current stream, for each of the four stages and for `floor_plan` as a whole; the wrappers' allocations are inside the
timed region (torch's caching allocator after the warm-up).  The raster's time is printed beside the time its 24 bytes
per point take at 8 TB/s.  --host also times, once, the same steps with numpy / scipy.ndimage on the CPU, for
orientation only.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "ml-depth-pro-video_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    sys.path.insert(0, p)

RES, PAD = 0.1, 0.2


def host_times(pts, thr):
    """np.add.at / np.maximum.at raster, scipy.ndimage morphology and labelling on the CPU, once."""
    from scipy import ndimage

    out = {"points": len(pts), "cpus": len(os.sched_getaffinity(0))}
    t = time.time()
    part = pts if np.isnan(thr) else pts[pts[:, 1] >= thr]
    mn = part[:, [0, 2]].min(axis=0) - PAD
    mx = part[:, [0, 2]].max(axis=0) + PAD
    w, h = (int(v) for v in np.ceil((mx - mn) / RES))
    g = ((part[:, [0, 2]] - mn) / RES).astype(np.int64)
    cell = g[:, 1] * w + g[:, 0]
    density = np.bincount(cell, minlength=h * w)
    height = np.full(h * w, -np.inf, np.float32)
    np.maximum.at(height, cell, part[:, 1].astype(np.float32))
    out["raster_numpy_s"] = time.time() - t
    occ = (density > 0).reshape(h, w)
    t = time.time()
    s7, s3 = np.ones((7, 7), bool), np.ones((3, 3), bool)
    for _ in range(2):
        occ = ndimage.binary_erosion(ndimage.binary_dilation(occ, s7, border_value=0), s7, border_value=1)
    occ = ndimage.binary_dilation(ndimage.binary_erosion(occ, s3, border_value=1), s3, border_value=0)
    out["morphology_ndimage_s"] = time.time() - t
    t = time.time()
    lab, n = ndimage.label(occ, structure=s3)
    idx = np.arange(1, n + 1)
    ndimage.sum(occ, lab, idx), ndimage.center_of_mass(occ, lab, idx), ndimage.find_objects(lab)
    out["regions_ndimage_s"] = time.time() - t
    out.update(grid=[h, w], regions=int(n))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160", help="WxH")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--height", type=float, default=float("nan"), help="height threshold (default nan: every height)")
    ap.add_argument("--json", default=None)
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    from ground_numpy import terrain

    depth, f = terrain(h, w, 7)
    import torch

    from depth_pro import pointcloud as PC
    from ground_bench import timed

    dev = torch.device("cuda:0")
    xyz, _, _, count = PC.depth_to_points_async(torch.from_numpy(depth).to(dev), f, w, h)
    model = PC.fit_ground_plane(xyz, count)
    xyz, _ = PC.normalize_to_ground(xyz, model, count)
    xyz, _ = PC.ground_adjust(xyz, 20, 5, count)
    xyz, _, count = PC.clean_pointcloud(xyz, None, count)[:3]
    thr = args.height
    kw = dict(height_threshold=thr, resolution=RES, padding=PAD)
    plan = PC.floor_plan(xyz, None, count, **kw)
    s = PC.floor_plan_summary(plan)
    n = int(count.item())
    res = {"size": args.size, "iters": args.iters, "repeats": args.repeats, "resolution": RES, "padding": PAD,
           "height_threshold": None if thr != thr else thr, "cleaned_points": n, "grid": [s["height"], s["width"]],
           "stats": s["stats"], "region_stats": s["region_stats"], "regions_drawn": len(s["regions"]),
           "raster_bytes": 24 * n, "raster_ms_at_8TBs": 24 * n / 8e12 * 1e3,
           "raster_ms": [], "morphology_ms": [], "regions_ms": [], "image_ms": [], "floor_plan_ms": []}
    g = plan
    for _ in range(args.repeats):
        res["raster_ms"].append(timed(lambda: PC.occupancy_grid(xyz, None, count, thr, RES, PAD), args.iters))
        res["morphology_ms"].append(timed(lambda: PC.grid_morphology(g["occupied"], g["dims"]), args.iters))
        res["regions_ms"].append(timed(lambda: PC.grid_regions(g["cleaned"], g["dims"], g["density"], g["height"], g["origin"],
                                                               RES), args.iters))
        res["image_ms"].append(timed(lambda: PC.floorplan_image(g["labels"], g["dims"], g["table"], g["n_regions"], RES),
                                     args.iters))
        res["floor_plan_ms"].append(timed(lambda: PC.floor_plan(xyz, None, count, **kw), args.iters))
    if args.host:
        res["host"] = host_times(xyz[:n].cpu().numpy(), thr)
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
