"""GPU time of the depth-warped views (dp_anaglyph, dp_warp_views) on one frame, from stream events.

    python tools/effects_bench.py [--sizes 1536x1536,3840x2160] [--iters 200] [--repeats 3] [--json out.json]

A synthetic frame per size (random RGB, a smooth depth with a step edge, amplitude / separation 0.05 as the reference's
defaults).  Per repeat and call: 2 warm-up calls, then `iters` timed calls between two events on the current stream
(tools/ground_bench.py's protocol); outputs are allocated once, the wrappers' small allocations (workspace, counters)
are inside the timed region (torch's caching allocator after the warm-up).  The yardstick is `dp_depth_to_image` in
colour mode on the same depth in the same process: like the new kernels it finds the depth's range in a first pass and
then reads 4 B and writes 3 B per pixel.  Bytes/s are the bytes the algorithm needs (both passes' depth reads, the image
once, every output byte; the gather's taps beyond the image itself are not counted) over the measured time.
"""

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "ml-depth-pro-video_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1536x1536,3840x2160", help="comma-separated WxH")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from depth_pro import effects as E
    from depth_pro import ops
    from ground_bench import timed

    dev = torch.device("cuda:0")
    res = {"iters": args.iters, "repeats": args.repeats, "sizes": {}}
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        rng = np.random.default_rng(0)
        image = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
        yy, xx = np.meshgrid(np.linspace(0, 1, H, dtype=np.float32), np.linspace(0, 1, W, dtype=np.float32), indexing="ij")
        depth = 2.0 + 3.0 * yy + np.sin(9.0 * xx).astype(np.float32) + 4.0 * (xx > 0.6)
        depth = torch.from_numpy(depth.astype(np.float32)).to(dev)
        views = [E.view_params("circle", 0.05, W, H, f, 150) for f in range(3, 3 + 8 * 18, 18)]
        out1 = torch.empty(1, H, W, 3, dtype=torch.uint8, device=dev)
        out8 = torch.empty(8, H, W, 3, dtype=torch.uint8, device=dev)
        col = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
        mm = torch.empty(2, dtype=torch.int32, device=dev)
        px = H * W

        def eight_single():
            for v in range(8):
                E.warp_views(image, depth, views[v:v + 1], out=out8[v:v + 1])

        calls = {       # name: (call, bytes the algorithm needs)
            "depth_to_image_color": (lambda: ops.depth_to_image(depth, True, "turbo", out=col, scratch=mm), px * (4 + 4 + 3)),
            "anaglyph": (lambda: E.anaglyph(image, depth, 0.05, out=col), px * (4 + 4 + 3 + 3)),
            "warp_1_view": (lambda: E.warp_views(image, depth, views[:1], out=out1), px * (4 + 4 + 3 + 3)),
            "warp_8_views_one_launch": (lambda: E.warp_views(image, depth, views, out=out8), px * (4 + 4 + 3 + 3 * 8)),
            "warp_8_single_view_launches": (eight_single, px * (4 + 4 + 3 + 3) * 8),
            "warp_1_zoom_view": (lambda: E.warp_views(image, depth, [E.view_params("zoom", 0.05, W, H, 37, 150)], out=out1), px * (3 + 3)),
        }
        r = {"pixels": px, "ms": {k: [] for k in calls}}
        for _ in range(args.repeats):
            for k, (call, _) in calls.items():
                r["ms"][k].append(timed(call, args.iters))
        r["best_ms"] = {k: min(v) for k, v in r["ms"].items()}
        r["bytes"] = {k: b for k, (_, b) in calls.items()}
        r["gb_per_s"] = {k: calls[k][1] / (r["best_ms"][k] * 1e-3) / 1e9 for k in calls}
        r["ns_per_pixel"] = {k: r["best_ms"][k] * 1e6 / px for k in calls}
        r["one_view_over_yardstick"] = r["best_ms"]["warp_1_view"] / r["best_ms"]["depth_to_image_color"]
        r["eight_in_one_over_eight_single"] = r["best_ms"]["warp_8_views_one_launch"] / r["best_ms"]["warp_8_single_view_launches"]
        _, bad = E.warp_views(image, depth, views, out=out8)
        r["bad"] = int(bad.sum())
        res["sizes"][size] = r
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
