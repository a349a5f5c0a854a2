"""GPU time of the rectangle list and the L-shape split (dp_shape_rectangles, dp_lshape_split) beside the
shape fit's, from stream events.

    python tools/lshape_bench.py [--size 3840x2160] [--iters 10] [--repeats 3] [--json out.json]

The synthetic 3840 x 2160 terrain of tools/cluster_bench.py, levelled, with the walls of eight 6 x 5 m rooms
(200 000 rows each, a 2.9 x 2.3 m block inside each: large enough that a room's empty share is under 0.6 and
the room splits into its wall ring and the block) added to the cloud, at the loop's defaults (y >= 1.3 m, at
most 100 000 participants) but for the circularity threshold: 0.99, because at 0.85 the reference's decision
calls the outline of a 6 x 5 room a circle and the list would hold nothing to split.  Per repeat: 2 warm-up
calls, then `iters` timed calls between two events on the current stream, for fit_shapes, rectangle_list and
split_l_shapes each (the wrappers' allocations are inside the timed region: torch's caching allocator after
the warm-up).
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "ml-depth-pro-video_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    sys.path.insert(0, p)

from depth_pro import pointcloud as PC  # noqa: E402
from ground_bench import timed  # noqa: E402


def rooms(g, n_rooms=8, w=6.0, h=5.0, per_room=200000):
    """(N, 3) wall and block points of n_rooms rooms in a row, 9 m apart, 12 m in front of the camera: enough rows
    that the cluster stage's even thinning to 100 000 participants leaves the walls dense."""
    out = []
    for k in range(n_rooms):
        nw = per_room * 3 // 4
        t = g.uniform(0, 2 * (w + h), nw)
        wall = np.where((t < w)[:, None], np.c_[t, np.zeros(nw)],
                        np.where((t < w + h)[:, None], np.c_[np.full(nw, w), t - w],
                                 np.where((t < 2 * w + h)[:, None], np.c_[t - w - h, np.full(nw, h)],
                                          np.c_[np.zeros(nw), t - 2 * w - h])))
        block = np.c_[g.uniform(1.55, 4.45, per_room - nw), g.uniform(1.35, 3.65, per_room - nw)]
        xz = np.r_[wall, block] + g.uniform(-0.01, 0.01, (per_room, 2)) + [9.0 * (k - n_rooms / 2), 12.0]
        out.append(np.c_[xz[:, 0], g.uniform(1.35, 2.0, per_room), xz[:, 1]])
    pts = np.concatenate(out)
    return pts[g.permutation(len(pts))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160", help="WxH")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    from ground_numpy import terrain

    dev = torch.device("cuda:0")
    depth, f = terrain(h, w, 7)
    xyz, _, _, count = PC.depth_to_points_async(torch.from_numpy(depth).to(dev), f, w, h)
    model = PC.fit_ground_plane(xyz, count)
    xyz, _ = PC.normalize_to_ground(xyz, model, count)
    xyz, _ = PC.ground_adjust(xyz, 20, 5, count)
    n = int(count.item())
    extra = torch.from_numpy(rooms(np.random.default_rng(0))).to(dev)
    xyz = torch.cat([xyz[:n], extra]).contiguous()
    kw = dict(height_threshold=1.3, max_points=100000)
    labels, ncl, stats = PC.dbscan_labels(xyz, None, **kw)
    table, order, offsets = PC.cluster_table(xyz, labels, ncl)
    shapes = PC.fit_shapes(xyz, order, offsets, ncl, circularity_threshold=0.99)[0]
    rects, n_rects = PC.rectangle_list(shapes, ncl)
    out, n_out, info = PC.split_l_shapes(xyz, labels, rects, n_rects)
    nr = int(n_rects.item())
    st = info[:nr, 0].cpu().numpy().astype(int)
    inf = info[:nr].cpu().numpy()
    res = {"size": args.size, "iters": args.iters, "repeats": args.repeats, "points": int(xyz.shape[0]),
           "participants": int(stats[2].item()), "clusters": int(ncl.item()), "rectangles": nr,
           "rows_out": n_out.cpu().tolist(), "status_counts": np.bincount(st, minlength=10).tolist(),
           "candidates": int((st != 1).sum()), "grid_cells": int((inf[:, 2] * inf[:, 3])[(st != 1) & (st != 3) & (st != 9)].sum()),
           "shapes_ms": [], "rectangle_list_ms": [], "split_l_shapes_ms": []}
    for _ in range(args.repeats):
        res["shapes_ms"].append(timed(lambda: PC.fit_shapes(xyz, order, offsets, ncl, circularity_threshold=0.99), args.iters))
        res["rectangle_list_ms"].append(timed(lambda: PC.rectangle_list(shapes, ncl), args.iters))
        res["split_l_shapes_ms"].append(timed(lambda: PC.split_l_shapes(xyz, labels, rects, n_rects), args.iters))
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
