"""GPU time of the point-cloud clustering (dp_cluster_dbscan, dp_cluster_table), from stream events.

    python tools/cluster_bench.py [--size 3840x2160] [--iters 10] [--json out.json] [--runs 2,3,1] [--sklearn]

Three runs, each 2 warm-up calls then `iters` timed calls between two events on the current stream
(the workspace allocation of the Python wrappers is inside the timed region: torch's caching
allocator after the warm-up):
  1  the levelled synthetic terrain of tools/clean_bench.py, every point (max_points 0, no height test);
  2  the same terrain at the loop's defaults (y >= 1.3 m, at most 100 000 points);
  3  1 M coincident points (the dense-cell rule: must not cost more than ten times run 1 per point).
The labels and the table are timed separately.  The times are per call, not per stage: a split by
sort / core flags / union / numbering / border needs a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python tools/cluster_bench.py), the kernels are named after the
stages.  --sklearn also times sklearn's DBSCAN on run 2's participants, once, where it is installed.
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


def one(name, xyz, count, iters, **kw):
    t0 = time.time()
    labels, ncl, stats = PC.dbscan_labels(xyz, count, **kw)
    st = stats.cpu().tolist()
    first = time.time() - t0
    print(f"[{name}] first call {first:.3f} s, stats {st}", flush=True)
    db = timed(lambda: PC.dbscan_labels(xyz, count, **kw), iters)
    tb = timed(lambda: PC.cluster_table(xyz, labels, ncl, count), iters)
    n = st[0] + st[1]
    res = {"points": int(n), "stats": dict(zip(PC.CLUSTER_STATS, st)), "first_call_s": first, "dbscan_ms": db,
           "table_ms": tb, "dbscan_ns_per_point": db * 1e6 / max(n, 1), "table_ns_per_point": tb * 1e6 / max(n, 1)}
    print(f"[{name}] {json.dumps(res)}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160", help="WxH")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    ap.add_argument("--runs", default="2,3,1")
    ap.add_argument("--sklearn", action="store_true")
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    from ground_numpy import terrain

    dev = torch.device("cuda:0")
    depth, f = terrain(h, w, 7)
    xyz, _, _, count = PC.depth_to_points_async(torch.from_numpy(depth).to(dev), f, w, h)
    model = PC.fit_ground_plane(xyz, count)
    xyz, _ = PC.normalize_to_ground(xyz, model, count)
    xyz, _ = PC.ground_adjust(xyz, 20, 5, count)
    res = {"size": args.size, "iters": args.iters}

    def dump():
        if args.json:
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as fh:
                json.dump(res, fh, indent=1)

    for r in args.runs.split(","):
        if r == "1":
            res["run1_terrain_all"] = one("run1", xyz, count, args.iters, height_threshold=None, max_points=0)
        elif r == "2":
            res["run2_terrain_defaults"] = one("run2", xyz, count, args.iters, height_threshold=1.3, max_points=100000)
        elif r == "3":
            same = torch.tensor([[1.0, 2.0, 3.0]], dtype=torch.float64, device=dev).repeat(1000000, 1)
            res["run3_coincident_1M"] = one("run3", same, None, args.iters, height_threshold=None, max_points=0)
        dump()
    if "run1_terrain_all" in res and "run3_coincident_1M" in res:
        res["dense_ratio_per_point"] = res["run3_coincident_1M"]["dbscan_ns_per_point"] / \
            res["run1_terrain_all"]["dbscan_ns_per_point"]
    if args.sklearn:
        from sklearn.cluster import DBSCAN

        sys.path.insert(0, os.path.join(REPO, "tests"))
        import cluster_numpy as N

        pts = xyz[:int(count.item())].cpu().numpy()
        rows = N.participants(pts, 1.3, 100000)
        t = time.time()
        DBSCAN(eps=0.2, min_samples=5).fit(pts[rows][:, [0, 2]])
        res["sklearn_run2_s"] = time.time() - t
        res["sklearn_run2_points"] = len(rows)
    print(json.dumps(res))
    dump()


if __name__ == "__main__":
    main()
