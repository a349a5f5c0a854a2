"""GPU time of the oriented-mesh-points stage (dp_voxel_downsample, dp_knn_search, dp_estimate_normals), from
stream events.

    python tools/normals_bench.py [--size 3840x2160] [--iters 10] [--repeats 3] [--json out.json] [--host]

The synthetic 3840 x 2160 terrain of tools/cluster_bench.py, levelled and cleaned, at the loop's defaults (voxel
0.05 m, radius 0.1 m, at most 30 neighbours).  Per repeat: 2 warm-up calls, then `iters` timed calls between two
events on the current stream, for voxel_downsample (on the cleaned cloud), knn_search and the normals (on the
down-sampled cloud) each; the wrappers' allocations are inside the timed region (torch's caching allocator
after the warm-up).  --host also times, once, the same three steps with numpy and scipy's cKDTree on the CPU
(np.unique voxel grid, cKDTree.query(k, distance_upper_bound), batched numpy.linalg.eigh), for orientation only.
Also reports the largest Rayleigh excess and direction error of the device normals against
eigh on the fixtures' cloud A (tests/golden/golden_normals.npz).
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

VOXEL, MAX_NN = 0.05, 30


def host_times(pts):
    """np.unique voxel grid + cKDTree hybrid search + batched eigh on the CPU, once."""
    from scipy.spatial import cKDTree

    out = {"points": len(pts), "cpus": len(os.sched_getaffinity(0))}
    t = time.time()
    idx = np.floor((pts - (pts.min(axis=0) - VOXEL / 2)) / VOXEL).astype(np.int64)
    key = (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    down = np.stack([np.bincount(inv, weights=pts[:, a]) for a in range(3)], axis=1) / cnt[:, None]
    out["voxel_numpy_s"] = time.time() - t
    out["voxels"] = len(down)
    t = time.time()
    d, i = cKDTree(down).query(down, k=MAX_NN, distance_upper_bound=2 * VOXEL, workers=-1)
    out["ckdtree_query_s"] = time.time() - t
    t = time.time()
    ok = np.isfinite(d)
    m = ok.sum(axis=1)
    nb = np.where(ok[:, :, None], down[np.where(ok, i, 0)], 0.0)
    mean = nb.sum(axis=1) / m[:, None]
    c = np.where(ok[:, :, None], nb - mean[:, None, :], 0.0)
    C = np.einsum("nki,nkj->nij", c, c) / m[:, None, None]
    w, v = np.linalg.eigh(C)
    nrm = v[:, :, 0]
    nrm = np.where(((nrm * -down).sum(axis=1) < 0)[:, None], -nrm, nrm)
    out["normals_numpy_s"] = time.time() - t
    return out


def fixture_accuracy(dev):
    """Largest Rayleigh excess / l2 and |sin| * gap of the device normals on cloud A against numpy.linalg.eigh."""
    import torch

    import normals_numpy as N
    from depth_pro import pointcloud as PC

    gold = np.load(os.path.join(REPO, "tests", "golden", "golden_normals.npz"))
    out = {}
    for name, pts in (("A", gold["A_points"]), ("A_down", N.voxel_downsample(gold["A_points"], None, None, VOXEL)["points"])):
        t = torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
        nbr, cnt, _ = PC.knn_search(t, None, 0.1, MAX_NN)
        nrm = PC.normals_from_neighbors(t, nbr, cnt, None, (0, 0, 0), False)[0].cpu().numpy()
        nbr, cnt = nbr.cpu().numpy(), cnt.cpu().numpy()
        C = N.covariance(pts, nbr, cnt)[1]
        w, v = np.linalg.eigh(C)
        rows = cnt >= 3
        excess = np.einsum("ni,nij,nj->n", nrm[rows], C[rows], nrm[rows]) - w[rows, 0]
        gap = (w[rows, 1] - w[rows, 0]) / w[rows, 2]
        sin = np.linalg.norm(np.cross(nrm[rows], v[rows][:, :, 0]), axis=1)
        out[name] = {"rows": int(rows.sum()), "rayleigh_excess_over_l2": float(np.max(excess / w[rows, 2])),
                     "sin_times_gap": float(np.max(sin * gap)), "sin": float(sin.max()),
                     "length_error": float(np.abs(np.sqrt((nrm[rows] ** 2).sum(axis=1)) - 1).max())}
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

    depth, f = terrain(h, w, 7)
    res = {"size": args.size, "iters": args.iters, "repeats": args.repeats, "voxel_size": VOXEL, "radius": 2 * VOXEL,
           "max_nn": MAX_NN}
    import torch

    from depth_pro import pointcloud as PC
    from ground_bench import timed

    dev = torch.device("cuda:0")
    xyz, _, _, count = PC.depth_to_points_async(torch.from_numpy(depth).to(dev), f, w, h)
    model = PC.fit_ground_plane(xyz, count)
    xyz, _ = PC.normalize_to_ground(xyz, model, count)
    xyz, _ = PC.ground_adjust(xyz, 20, 5, count)
    xyz, _, count = PC.clean_pointcloud(xyz, None, count)[:3]
    down, _, _, _, n_out, vst = PC.voxel_downsample(xyz, None, count, VOXEL)
    nbr, cnt, kst = PC.knn_search(down, n_out, 2 * VOXEL, MAX_NN)
    _, nst = PC.normals_from_neighbors(down, nbr, cnt, n_out)
    res.update({"cleaned_points": int(count.item()), "voxels": int(n_out.item()),
                "voxel_stats": dict(zip(PC.VOXEL_STATS, vst.cpu().tolist())),
                "knn_stats": dict(zip(PC.KNN_STATS, kst.cpu().tolist())),
                "normal_stats": dict(zip(PC.NORMAL_STATS, nst.cpu().tolist())),
                "voxel_ms": [], "knn_ms": [], "normals_ms": []})
    for _ in range(args.repeats):
        res["voxel_ms"].append(timed(lambda: PC.voxel_downsample(xyz, None, count, VOXEL), args.iters))
        res["knn_ms"].append(timed(lambda: PC.knn_search(down, n_out, 2 * VOXEL, MAX_NN), args.iters))
        res["normals_ms"].append(timed(lambda: PC.normals_from_neighbors(down, nbr, cnt, n_out), args.iters))
    res["fixture_accuracy"] = fixture_accuracy(dev)
    if args.host:
        res["host"] = host_times(xyz[:int(count.item())].cpu().numpy())
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
