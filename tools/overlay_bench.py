"""GPU time of the shape overlays (dp_overlay_shapes, depth_pro.overlay), from stream events.

    python tools/overlay_bench.py [--size 3840x2160] [--picture 1280x720] [--iters 50] [--repeats 3] [--json out.json]

The cloud is the synthetic 3840 x 2160 terrain of tools/render_bench.py, levelled, with random colours; the shapes are
synthetic lists of 8, 256 and 4096 (three rectangles at random angles to every circle, sides and radii of 0.2 to 1.5 m,
centres spread over the plan).  Per repeat: 2 warm-up calls, then `iters` timed calls between two events on the current
stream; the smallest repeat is quoted.  The stages are timed through the C entry point with the bench-only switches of
dp_overlay_debug_flags: `records` is the call without its draw launch (flags, the two scan kernels, both record kernels
and the counts: six launches), `draw` the call without those (the draw kernel on the records the full call before it
left, and the counts: two launches), `call` the whole entry point; `whole` is `depth_pro.overlay.plan_with_shapes` as a
user calls it, its allocations and the plan included, and `plan` is `render.render_views(views="plan")` alone in the same session.
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


def shape_lists(n, cam, W, H, seed):
    """(rects (n_r, 8), table (n_c, 16)) with n_r + n_c = n, centres on the picture."""
    rng = np.random.default_rng(seed)
    n_c = n // 4
    n_r = n - n_c
    cx, cz, scale = cam[2], cam[3], cam[4]
    u = cx + (rng.random(n) - 0.5) * (W - 1) / scale
    v = cz + (rng.random(n) - 0.5) * (H - 1) / scale
    rects = np.zeros((n_r, 8))
    rects[:, 0], rects[:, 1] = u[:n_r], v[:n_r]
    rects[:, 2:4] = 0.2 + 1.3 * rng.random((n_r, 2))
    rects[:, 4] = 90.0 * rng.random(n_r)
    table = np.zeros((max(n_c, 1), 16))
    table[:n_c, 0] = 2.0
    table[:n_c, 8], table[:n_c, 9], table[:n_c, 10] = u[n_r:], v[n_r:], 0.1 + 0.65 * rng.random(n_c)
    return rects, table[:n_c] if n_c else table[:0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160", help="WxH of the frame the cloud comes from")
    ap.add_argument("--picture", default="1280x720", help="WxH of the picture")
    ap.add_argument("--point-size", type=int, default=7)
    ap.add_argument("--counts", default="8,256,4096")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    W, H = (int(v) for v in args.picture.split("x"))
    import torch
    from ground_bench import timed
    from ground_numpy import terrain

    from depth_pro import _lib
    from depth_pro import overlay as OV
    from depth_pro import pointcloud as PC
    from depth_pro import render as R

    depth, f = terrain(h, w, 7)
    dev = torch.device("cuda:0")
    rgb = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(0))
    xyz, _, cols, count = PC.depth_to_points_async(torch.from_numpy(depth).to(dev), f, w, h, rgb=rgb)
    model = PC.fit_ground_plane(xyz, count)
    xyz, _ = PC.normalize_to_ground(xyz, model, count)
    xyz, _ = PC.ground_adjust(xyz, 20, 5, count)
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    plan = R.render_views(xyz, cols, views="plan", size=(W, H), point_size=args.point_size, count=count)
    cam_dev = plan["cameras"][0].contiguous()
    cam = cam_dev.cpu().numpy()
    pal = (ctypes.c_uint8 * 48)(*OV._rgb(OV.RECT_PALETTE), *OV._rgb(OV.CIRCLE_PALETTE))
    res = {"cloud_size": args.size, "rows": int(count.item()), "picture": args.picture, "point_size": args.point_size,
           "iters": args.iters, "repeats": args.repeats, "stroke": 3.0, "alpha": OV.STROKE_ALPHA, "label_scale": 2,
           "plan_ms": [timed(lambda: R.render_views(xyz, cols, views="plan", size=(W, H), point_size=args.point_size, count=count),
                             args.iters) for _ in range(args.repeats)], "lists": {}}
    for n in (int(v) for v in args.counts.split(",")):
        rects_h, table_h = shape_lists(n, cam, W, H, n)
        rects, table = torch.from_numpy(rects_h).to(dev), torch.from_numpy(table_h).to(dev)
        mr, mc = rects.shape[0], table.shape[0]
        n_r = torch.tensor([mr], dtype=torch.int32, device=dev)
        n_c = torch.tensor([mc], dtype=torch.int32, device=dev)
        image = plan["image"][0].clone()
        records = torch.empty(max(mr + mc, 1), _lib.DP_OVERLAY_RECORD_DOUBLES, dtype=torch.float64, device=dev)
        stats = torch.empty(_lib.DP_OVERLAY_STATS, dtype=torch.float64, device=dev)
        ws = torch.empty(int(lib.dp_overlay_workspace_size(mr, mc)), dtype=torch.uint8, device=dev)

        def call(flags=0):
            lib.dp_overlay_debug_flags(flags)
            try:
                _call()
            finally:
                lib.dp_overlay_debug_flags(0)

        def _call(img=image, pw=W, ph=H):
            _lib.check(lib.dp_overlay_shapes(img.data_ptr(), pw, ph, cam_dev.data_ptr(), rects.data_ptr(), n_r.data_ptr(), mr,
                                             table.data_ptr() if mc else None, n_c.data_ptr(), mc, pal, 3.0, OV.STROKE_ALPHA, 2,
                                             records.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), stream), "dp_overlay_shapes")

        call()
        torch.cuda.synchronize()
        out = {"rectangles": mr, "circles": mc, "stats": OV.stats_dict(stats.cpu().numpy()), "records_ms": [], "draw_ms": [], "call_ms": [], "whole_ms": []}
        for _ in range(args.repeats):
            out["records_ms"].append(timed(lambda: call(2), args.iters))
            out["draw_ms"].append(timed(lambda: call(1), args.iters))
            out["call_ms"].append(timed(call, args.iters))
            out["whole_ms"].append(timed(lambda: OV.plan_with_shapes(xyz, cols, count, rects, n_r, table if mc else None, n_c if mc else None,
                                                                     size=(W, H), point_size=args.point_size), args.iters))
        res["lists"][str(n)] = out
    line = json.dumps(res)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
