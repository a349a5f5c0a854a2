"""GPU time of the shape fit (dp_cluster_shapes) beside the cluster stage's, from stream events.

    python tools/shapes_bench.py [--size 3840x2160] [--iters 10] [--repeats 3] [--json out.json] [--host]

The synthetic 3840 x 2160 terrain of tools/cluster_bench.py, levelled, at the loop's defaults (y >= 1.3 m,
at most 100 000 points).  Per repeat: 2 warm-up calls, then `iters` timed calls between two events on the
current stream, for dbscan_labels, cluster_table and fit_shapes each (the wrappers' allocations are inside
the timed region: torch's caching allocator after the warm-up).  A second scene puts the 100 000 points
into ONE cluster (a disc), the hull's and the circle's worst case.  --host also times, once, the numpy
restatement (tests/shapes_numpy.py) and the reference's own calls (scipy ConvexHull + leastsq) on the
same clusters, where scipy is installed.
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "ml-depth-pro-video_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    sys.path.insert(0, p)

from depth_pro import pointcloud as PC  # noqa: E402
from ground_bench import timed  # noqa: E402


def stage_times(name, xyz, count, iters, repeats, **kw):
    labels, ncl, stats = PC.dbscan_labels(xyz, count, **kw)
    table, order, offsets = PC.cluster_table(xyz, labels, ncl, count)
    shapes = PC.fit_shapes(xyz, order, offsets, ncl, count)[0]
    k = int(ncl.item())
    sh = shapes[:min(k, 4096)].cpu().numpy()
    res = {"clusters": k, "participants": int(stats[2].item()), "largest_cluster": int(sh[:, 1].max()) if k else 0,
           "kinds": [int((sh[:, 0] == v).sum()) for v in (0, 1, 2)], "errors": int(sh[:, 15].sum()),
           "dbscan_ms": [], "table_ms": [], "shapes_ms": []}
    for _ in range(repeats):
        res["dbscan_ms"].append(timed(lambda: PC.dbscan_labels(xyz, count, **kw), iters))
        res["table_ms"].append(timed(lambda: PC.cluster_table(xyz, labels, ncl, count), iters))
        res["shapes_ms"].append(timed(lambda: PC.fit_shapes(xyz, order, offsets, ncl, count), iters))
    print(f"[{name}] {json.dumps(res)}", flush=True)
    return res, labels


def host_times(pts, labels):
    import shapes_numpy as S

    t = time.time()
    S.fit_shapes(pts, labels)
    out = {"restatement_s": time.time() - t}
    try:
        from scipy import optimize
        from scipy.spatial import ConvexHull
    except ImportError:
        return out
    t = time.time()
    for c in range(int(labels.max()) + 1):
        uv = np.c_[-pts[labels == c, 0], pts[labels == c, 2]]
        if len(uv) < 5:
            continue
        try:
            ConvexHull(uv)
        except Exception:
            pass

        def f_2(ctr):
            Ri = np.sqrt((uv[:, 0] - ctr[0]) ** 2 + (uv[:, 1] - ctr[1]) ** 2)
            return Ri - Ri.mean()
        optimize.leastsq(f_2, (uv[:, 0].mean(), uv[:, 1].mean()))
    out["scipy_hull_leastsq_s"] = time.time() - t
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="3840x2160", help="WxH")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    w, h = (int(v) for v in args.size.split("x"))
    from ground_numpy import terrain

    dev = torch.device("cuda:0")
    depth, f = terrain(h, w, 7)
    xyz, _, _, count = PC.depth_to_points_async(torch.from_numpy(depth).to(dev), f, w, h)
    model = PC.fit_ground_plane(xyz, count)
    xyz, _ = PC.normalize_to_ground(xyz, model, count)
    xyz, _ = PC.ground_adjust(xyz, 20, 5, count)
    res = {"size": args.size, "iters": args.iters, "repeats": args.repeats}
    res["terrain_defaults"], labels = stage_times("terrain", xyz, count, args.iters, args.repeats, height_threshold=1.3,
                                                  max_points=100000)
    if args.host:
        n = int(count.item())
        res["terrain_defaults"]["host"] = host_times(xyz[:n].cpu().numpy(), labels[:n].cpu().numpy())
    g = np.random.default_rng(0)
    t, r = g.uniform(0, 2 * np.pi, 100000), 3.0 * np.sqrt(g.uniform(0, 1, 100000))
    disc = torch.from_numpy(np.c_[r * np.cos(t), np.full(100000, 2.0), 10 + r * np.sin(t)]).to(dev)
    res["one_cluster_100k"], _ = stage_times("disc", disc, None, args.iters, args.repeats, height_threshold=1.3,
                                             max_points=100000)
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
