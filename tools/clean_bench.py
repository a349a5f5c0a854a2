"""Per-stage GPU time of the point-cloud cleaning at one frame size, from stream events.

    python tools/clean_bench.py [--size 3840x2160] [--iters 10] [--json out.json] [--host]

A synthetic terrain depth map (tests/ground_numpy.py `terrain`) is back-projected and levelled once;
then the sort alone (64-bit and 63-bit key ranges over all pairs, per pass = total / 8), stray
removal, shadow cleaning (on the stray survivors) and compaction are timed alone: 2 warm-up calls,
`iters` timed calls between two events on the current stream.  The workspace allocation of the
Python wrappers is inside the timed region (torch's caching allocator after the warm-up).
--host also times tests/clean_numpy.py's restatement on the same points, once, for scale only.
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "ml-depth-pro-video_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

from depth_pro import pointcloud as PC  # noqa: E402
from ground_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160", help="WxH")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--host", action="store_true", help="also time the numpy / scipy restatement (minutes at 4K)")
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    from ground_numpy import terrain

    depth, f = terrain(h, w, 7)
    dev = torch.device("cuda:0")
    xyz, _, _, count = PC.depth_to_points_async(torch.from_numpy(depth).to(dev), f, w, h)
    model = PC.fit_ground_plane(xyz, count)
    xyz, _ = PC.normalize_to_ground(xyz, model, count)
    xyz, _ = PC.ground_adjust(xyz, 20, 5, count)
    n = xyz.shape[0]
    cols = torch.randint(0, 256, (n, 3), dtype=torch.uint8, device=dev)
    keys = torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), dtype=torch.int64, device=dev)
    vals = torch.arange(n, dtype=torch.int32, device=dev)
    keep1, st1 = PC.stray_mask(xyz, count)
    p1, c1, n1 = PC.compact_points(xyz, cols, keep1, count)
    _, st2 = PC.shadow_mask(p1, n1)
    sort64 = timed(lambda: PC.sort_pairs(keys, vals), args.iters)       # includes the two clones (20 bytes / pair)
    sort63 = timed(lambda: PC.sort_pairs(keys, vals, None, 0, 63), args.iters)
    clone = timed(lambda: (keys.clone(), vals.clone()), args.iters)
    res = {
        "size": args.size, "points": int(count.item()), "iters": args.iters,
        "sort_64bit_ms": sort64, "sort_63bit_ms": sort63, "sort_input_clone_ms": clone,
        "sort_pass_ms": (sort64 - clone) / 8,
        "sort_pass_GBps": 24 * n / ((sort64 - clone) / 8 * 1e-3) / 1e9,
        "stray_ms": timed(lambda: PC.stray_mask(xyz, count), args.iters),
        "shadows_ms": timed(lambda: PC.shadow_mask(p1, n1), args.iters),
        "compact_ms": timed(lambda: PC.compact_points(xyz, cols, keep1, count), args.iters),
        "clean_pointcloud_ms": timed(lambda: PC.clean_pointcloud(xyz, cols, count), args.iters),
        "stray_stats": st1.cpu().tolist(), "shadow_stats": st2.cpu().tolist(),
    }
    if args.host:
        import clean_numpy as C

        pts = xyz[:int(count.item())].cpu().numpy()
        t = time.time()
        C.clean(pts)
        res["host_restatement_s"] = time.time() - t
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
