"""GPU time of the triangle-mesh stage (dp_knn_exact, dp_mesh_fan, dp_mesh_clean_triangles), from stream events.

    python tools/mesh_bench.py [--size 3840x2160] [--iters 10] [--repeats 3] [--json out.json] [--host]

The synthetic 3840 x 2160 terrain of tools/cluster_bench.py, levelled, cleaned and down-sampled as tools/normals_bench.py
does (voxel 0.05 m), at the loop's defaults (6 neighbours, search grid of 2 * voxel).  Per repeat: 2 warm-up calls, then
`iters` timed calls between two events on the current stream, for knn_exact at k = 6 and at k = 20, the fan, the
triangle clean-up (on the fan of the k = 6 lists), the mean neighbour distance at k = 20 and simple_mesh whole (voxel
grid included); the wrappers' allocations are inside the timed region (torch's caching allocator after the warm-up).
For orientation, not as a speed-up: knn_search (radius 0.1 m, at most 30) on the same voxels, and with --host
scipy's cKDTree.query(k = 7) on the CPU, once.  Also reports the triangles before and after the clean-up and the
largest ring.
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

VOXEL, NEIGHBORS = 0.05, 6


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

    depth, f = terrain(h, w, 7)
    res = {"size": args.size, "iters": args.iters, "repeats": args.repeats, "voxel_size": VOXEL, "neighbors": NEIGHBORS,
           "cell_edge": 2 * VOXEL}
    import torch

    from depth_pro import pointcloud as PC
    from ground_bench import timed

    dev = torch.device("cuda:0")
    xyz, _, _, count = PC.depth_to_points_async(torch.from_numpy(depth).to(dev), f, w, h)
    model = PC.fit_ground_plane(xyz, count)
    xyz, _ = PC.normalize_to_ground(xyz, model, count)
    xyz, _ = PC.ground_adjust(xyz, 20, 5, count)
    xyz, _, count = PC.clean_pointcloud(xyz, None, count)[:3]
    down, _, _, _, n_out, _ = PC.voxel_downsample(xyz, None, count, VOXEL)
    n = int(n_out.item())
    down = down[:n].contiguous()                # the voxels alone: the fan's buffer then has n * 5 slots
    nbr, cnt, d2, kst = PC.knn_exact(down, None, NEIGHBORS, 2 * VOXEL)
    kst20 = PC.knn_exact(down, None, 20, 2 * VOXEL)[3]
    tri = PC.fan_triangles(nbr, cnt)
    _, n_tri, tst = PC.clean_triangles(tri, n)
    mean = PC.mean_neighbor_distance(down, None, 20, 2 * VOXEL)
    res.update({"cleaned_points": int(count.item()), "voxels": n,
                "knn_stats_k6": dict(zip(PC.KNN_EXACT_STATS, kst.cpu().tolist())),
                "knn_stats_k20": dict(zip(PC.KNN_EXACT_STATS, kst20.cpu().tolist())),
                "triangle_stats": dict(zip(PC.TRIANGLE_STATS, tst.cpu().tolist())),
                "triangles_before": int(tri.shape[0]), "triangles_after": int(n_tri.item()),
                "mean_neighbor_distance_k20": float(mean.item()),
                "knn_exact_k6_ms": [], "knn_exact_k20_ms": [], "fan_ms": [], "clean_ms": [], "mean_distance_k20_ms": [],
                "simple_mesh_ms": [], "knn_search_r0.1_nn30_ms": []})
    for _ in range(args.repeats):
        res["knn_exact_k6_ms"].append(timed(lambda: PC.knn_exact(down, None, NEIGHBORS, 2 * VOXEL), args.iters))
        res["knn_exact_k20_ms"].append(timed(lambda: PC.knn_exact(down, None, 20, 2 * VOXEL), args.iters))
        res["fan_ms"].append(timed(lambda: PC.fan_triangles(nbr, cnt), args.iters))
        res["clean_ms"].append(timed(lambda: PC.clean_triangles(tri, n), args.iters))
        res["mean_distance_k20_ms"].append(timed(lambda: PC.mean_neighbor_distance(down, None, 20, 2 * VOXEL), args.iters))
        res["simple_mesh_ms"].append(timed(lambda: PC.simple_mesh(xyz, None, count, VOXEL, NEIGHBORS), args.iters))
        res["knn_search_r0.1_nn30_ms"].append(timed(lambda: PC.knn_search(down, None, 2 * VOXEL, 30), args.iters))
    if args.host:
        from scipy.spatial import cKDTree

        pts = down.cpu().numpy()
        t = time.time()
        cKDTree(pts).query(pts, k=NEIGHBORS + 1, workers=-1)
        res["host"] = {"ckdtree_query_k7_s": time.time() - t, "cpus": len(os.sched_getaffinity(0))}
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
