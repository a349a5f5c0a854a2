"""Per-stage GPU time of the ground normalisation at one frame size, from stream events.

    python tools/ground_bench.py [--size 3840x2160] [--iters 10] [--json out.json]

A synthetic terrain depth map (tests/ground_numpy.py `terrain`) is back-projected once; each stage
(trace, distance percentile, normalise, adjust) is then timed alone: 2 warm-up calls, `iters` timed
calls between two events on the current stream.  The workspace allocation of the Python wrappers is
inside the timed region (it comes from torch's caching allocator after the warm-up).
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "ml-depth-pro-video_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

from depth_pro import pointcloud as PC  # noqa: E402


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160", help="WxH")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    from ground_numpy import terrain

    depth, f = terrain(h, w, 7)
    dev = torch.device("cuda:0")
    xyz, _, _, count = PC.depth_to_points_async(torch.from_numpy(depth).to(dev), f, w, h)
    model = PC.fit_ground_plane(xyz, count)
    normed, _ = PC.normalize_to_ground(xyz, model, count)
    lib = PC._lib.load()
    g = 20
    blob = torch.empty(g * 4 + 4 + g, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.dp_ground_workspace_size(xyz.shape[0])), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def trace():
        PC.check(lib.dp_ground_trace(xyz.data_ptr(), count.data_ptr(), xyz.shape[0], g, blob.data_ptr(),
                                     blob.data_ptr() + (g * 4 + 4) * 8, blob.data_ptr() + g * 32, ws.data_ptr(),
                                     ws.numel(), stream), "dp_ground_trace")

    res = {
        "size": args.size, "points": int(count.item()), "iters": args.iters,
        "trace_ms": timed(trace, args.iters),
        "dist_percentile_ms": timed(lambda: PC.distance_percentile(xyz, model["normal"], model["d"], 0.1, count),
                                    args.iters),
        "normalize_ms": timed(lambda: PC.normalize_to_ground(xyz, model, count), args.iters),
        "adjust_ms": timed(lambda: PC.ground_adjust(normed, 20, 5, count), args.iters),
    }
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
