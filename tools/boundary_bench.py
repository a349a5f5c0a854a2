"""GPU time of the boundary metric's counts (dp_boundary_counts, both kinds) from stream events.

    python tools/boundary_bench.py [--sizes 1536x1536,3840x2160] [--iters 10] [--repeats 3] [--json out.json] [--host]

The synthetic scene of tests/boundary_numpy.py at full size (WxH), the ten default thresholds.  Per repeat: 2 warm-up
calls, then `iters` timed calls between two events on the current stream; the wrapper's allocations (counts, workspace)
are inside the timed region (torch's caching allocator after the warm-up).  Beside each time: the bytes the call must
read at the least (both float32 images for the depth kind, the float32 prediction and the byte mask for the mask kind)
and the time they take at 8 TB/s.  The counts are checked against the numpy restatement once per size (--host also
times that restatement, once, for orientation only).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1536x1536,3840x2160", help="comma-separated WxH")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    import torch

    import boundary_numpy as B
    from depth_pro import _lib
    from depth_pro.eval import boundary_metrics as M
    from ground_bench import timed

    dev = torch.device("cuda:0")
    th, _ = M.get_thresholds_and_weights(1.05, 1.25, 10)
    th32 = th.astype(np.float32).astype(np.float64)
    out = {"iters": args.iters, "repeats": args.repeats, "thresholds": len(th), "sizes": {}}
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        pred, tgt, alpha = B.scene(h, w, 3)
        mask = alpha > 0.1
        p, t, m = (torch.from_numpy(a).to(dev) for a in (pred, tgt, mask.astype(np.uint8)))
        res = {"workspace_bytes": int(_lib.load().dp_boundary_workspace_size(h, w, len(th))),
               "depth_bytes": 8 * h * w, "depth_ms_at_8TBs": 8 * h * w / 8e12 * 1e3,
               "mask_bytes": 5 * h * w, "mask_ms_at_8TBs": 5 * h * w / 8e12 * 1e3, "depth_ms": [], "mask_ms": [], "f1_ms": []}
        for _ in range(args.repeats):
            res["depth_ms"].append(timed(lambda: M.boundary_counts(p, t, th, M.DP_BOUNDARY_DEPTH), args.iters))
            res["mask_ms"].append(timed(lambda: M.boundary_counts(p, m, th32, M.DP_BOUNDARY_MASK), args.iters))
            res["f1_ms"].append(timed(lambda: M.SI_boundary_F1(p, t), args.iters))        # with the read-back and the score
        got_d = M.boundary_counts(p, t, th, M.DP_BOUNDARY_DEPTH).view(torch.int64).cpu().numpy()
        got_m = M.boundary_counts(p, m, th32, M.DP_BOUNDARY_MASK).view(torch.int64).cpu().numpy()
        res["f1"], res["recall"] = float(M.SI_boundary_F1(p, t)), float(M.SI_boundary_Recall(p, torch.from_numpy(alpha).to(dev)))
        res["pred_edges_plain"], res["pred_edges_thinned"] = int(got_d[:, :, 2].sum()), int(got_m[:, :, 2].sum())
        t0 = time.time()
        want_d = B.counts(B.invert_depth(pred), B.invert_depth(tgt), th, "depth", "f64")
        t1 = time.time()
        want_m = B.counts(B.invert_depth(pred), mask, th, "mask", "f32")
        t2 = time.time()
        res["counts_equal_restatement"] = bool(np.array_equal(got_d, want_d.astype(np.int64)) and np.array_equal(got_m, want_m.astype(np.int64)))
        if args.host:
            res["host"] = {"cpus": len(os.sched_getaffinity(0)), "depth_numpy_s": t1 - t0, "mask_numpy_s": t2 - t1}
        out["sizes"][size] = res
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)
    if not all(r["counts_equal_restatement"] for r in out["sizes"].values()):
        sys.exit("counts differ from the restatement")


if __name__ == "__main__":
    main()
