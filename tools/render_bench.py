"""GPU time of the point-cloud views (dp_render_cameras, dp_render_points), from stream events.

    python tools/render_bench.py [--size 3840x2160] [--picture 1280x720] [--iters 50] [--repeats 3] [--json out.json]

The synthetic 3840 x 2160 terrain of tools/cluster_bench.py, levelled (not cleaned: every row is live), with random
colours.  Per repeat: 2 warm-up calls, then `iters` timed calls between two events on the current stream.  The stages
are timed through the C entry point on one workspace with the bench-only switches of dp_render_debug_flags (4 / 8 / 16
leave out bounds + cameras / project / resolve, so a stage runs alone on what the full call before it left); `whole`
is `depth_pro.render.render_views` as a user calls it, its allocations included.  `occupancy_grid` on the same cloud
is the yardstick for one scatter pass over every row.  The plain-load filter (1) and the in-wave agreement (2) are
timed on and off on the project stage.  Bytes: what each stage must move at the least.
"""

import argparse
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "ml-depth-pro-video_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160", help="WxH of the frame the cloud comes from")
    ap.add_argument("--picture", default="1280x720", help="WxH of the picture")
    ap.add_argument("--point-size", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    W, H = (int(v) for v in args.picture.split("x"))
    ps = args.point_size
    import torch
    from ground_bench import timed
    from ground_numpy import terrain

    from depth_pro import _lib
    from depth_pro import pointcloud as PC
    from depth_pro import render as R

    depth, f = terrain(h, w, 7)
    dev = torch.device("cuda:0")
    rgb = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(0))
    xyz, _, cols, count = PC.depth_to_points_async(torch.from_numpy(depth).to(dev), f, w, h, rgb=rgb)
    model = PC.fit_ground_plane(xyz, count)
    xyz, _ = PC.normalize_to_ground(xyz, model, count)
    xyz, _ = PC.ground_adjust(xyz, 20, 5, count)
    n = int(count.item())
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    cnt = count.to(torch.int32).reshape(1)
    configs = {"front": (("front",), False), "multi": (R.SHEET, True), "plan": (("plan",), False)}
    res = {"cloud_size": args.size, "rows": n, "picture": args.picture, "point_size": ps, "iters": args.iters, "repeats": args.repeats,
           "occupancy_grid_ms": [timed(lambda: PC.occupancy_grid(xyz, None, count, float("nan"), 0.1, 0.2), args.iters)
                                 for _ in range(args.repeats)], "views": {}}
    for name, (views, sheet) in configs.items():
        rows, plan = R._views(views)
        nv, total = len(rows), len(rows) + (1 if plan else 0)
        flat = [c for r in rows for c in r]
        varr = (ctypes.c_double * max(len(flat), 1))(*flat)
        bg = (ctypes.c_uint8 * 6)(255, 255, 255, *R.PLAN_BACKGROUND)
        image = torch.empty((total, H, W, 3), dtype=torch.uint8, device=dev)
        cams = torch.empty(total, 24, dtype=torch.float64, device=dev)
        stats = torch.empty(24, dtype=torch.float64, device=dev)
        ws = torch.empty(int(lib.dp_render_workspace_size(W, H, ps, total)), dtype=torch.uint8, device=dev)

        def call(flags=0):
            lib.dp_render_debug_flags(flags)
            try:
                _lib.check(lib.dp_render_points(xyz.data_ptr(), cols.data_ptr(), cnt.data_ptr(), xyz.shape[0], varr, nv, 1 if plan else 0,
                                                0.0, W, H, ps, bg, R.TAN_HALF_FOV, 1 if sheet else 0, image.data_ptr(), cams.data_ptr(),
                                                stats.data_ptr(), ws.data_ptr(), ws.numel(), stream), "dp_render_points")
            finally:
                lib.dp_render_debug_flags(0)

        call()
        torch.cuda.synchronize()
        summary = R.stats_dict(stats.cpu().numpy(), total)
        centre = (H + ps - 1) * (W + ps - 1) * 8 * total
        out = {"stats": summary,
               "bytes": {"bounds": 24 * n, "project": 24 * n + centre + 8 * sum(summary["drawn"]),
                         "resolve": centre + 3 * W * H * total + 3 * sum(summary["covered_pixels"])},
               "bounds_cameras_ms": [], "project_ms": [], "resolve_ms": [], "call_ms": [], "whole_ms": [],
               "project_no_filter_ms": [], "project_no_wave_ms": [], "project_neither_ms": []}
        for _ in range(args.repeats):
            out["bounds_cameras_ms"].append(timed(lambda: call(8 | 16), args.iters))
            out["project_ms"].append(timed(lambda: call(4 | 16), args.iters))
            out["resolve_ms"].append(timed(lambda: call(4 | 8), args.iters))
            out["call_ms"].append(timed(call, args.iters))
            out["whole_ms"].append(timed(lambda: R.render_views(xyz, cols, views, (W, H), ps, count=count, sheet=sheet), args.iters))
            out["project_no_filter_ms"].append(timed(lambda: call(4 | 16 | 1), args.iters))
            out["project_no_wave_ms"].append(timed(lambda: call(4 | 16 | 2), args.iters))
            out["project_neither_ms"].append(timed(lambda: call(4 | 16 | 3), args.iters))
        tot = sum(out["bytes"].values())
        out["bytes"]["total"] = tot
        out["TBps_whole_call"] = tot / (min(out["call_ms"]) * 1e-3) / 1e12
        if name == "multi":
            out["four_single_calls_ms"] = [timed(lambda: [R.render_views(xyz, cols, (v,), (W, H), ps, count=count) for v in R.SHEET],
                                                 args.iters) for _ in range(args.repeats)]
        res["views"][name] = out
    line = json.dumps(res)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
