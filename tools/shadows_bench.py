"""GPU time of the depth-shadow stages (csrc/dp_shadows.hip) on one frame, from stream events.

    python tools/shadows_bench.py [--sizes 1536x1536,3840x2160] [--iters 100] [--repeats 3] [--json out.json]

Two depths per size: the synthetic scene of the tests (boxes on a ramp, tests/shadows_numpy.py: a few large components)
and a noise depth (uniform 0.5 ... 50: hundreds of thousands of components, the labeller's worst case).  Per repeat and
call: 2 warm-up calls, then `iters` timed calls between two events on the current stream (tools/ground_bench.py's
protocol); the wrappers' allocations (workspace, outputs, stats) are inside the timed region (torch's caching allocator
after the warm-up).  Whole calls and stages: `gradient` (dp_depth_gradient), `edges` (dp_depth_edges: gradient +
threshold), `regions` (dp_region_filter on ~edge), `chain` (dp_depth_shadows), `chain_drop` (with the NaN-masked depth),
`fill` (dp_fill_ground_shadows).  Beside them `dp_depth_to_image` in colour mode on the same depth, the one-pass
yardstick, and `dp_grid_regions` (8-connected, numbered, with a region table) on a crop of the same free mask of at most
2048 x 2048, with `regions` on the same crop.  Bytes are those a stage must move (its inputs once, its outputs once:
gradient 4 + 4 B per pixel, edges 4 + 1, regions 1 + 1, chain 4 + 1, chain_drop 4 + 1 + 4, fill 4 + 1 + 4), not those
it does move; TB/s is that over the measured time.
"""

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "ml-depth-pro-video_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    sys.path.insert(0, p)

MUST_MOVE = {"gradient": 8, "edges": 5, "regions": 2, "chain": 5, "chain_drop": 9, "fill": 9, "depth_to_image_color": 11}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1536x1536,3840x2160", help="comma-separated WxH")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import shadows_numpy as SN
    from depth_pro import ops
    from depth_pro import pointcloud as PC
    from depth_pro import shadows as SH
    from ground_bench import timed

    dev = torch.device("cuda:0")
    res = {"iters": args.iters, "repeats": args.repeats, "must_move_bytes_per_pixel": MUST_MOVE, "sizes": {}}
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        px = H * W
        depths = {"scene": SN.scene(H, W, 7, noise=0.02),
                  "noise": np.random.default_rng(1).uniform(0.5, 50.0, (H, W)).astype(np.float32)}
        res["sizes"][size] = {"pixels": px}
        for kind, host in depths.items():
            thr = 0.05 if kind == "scene" else 0.2
            depth = torch.from_numpy(host).to(dev)
            edge, _ = SH.edge_mask(depth, thr)
            free = (edge == 0).to(torch.uint8)
            shadow = SH.find_depth_shadows(depth, thr, 100)
            col = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)
            mm = torch.empty(2, dtype=torch.int32, device=dev)
            plane = {"normal": [0.0, -0.8, 0.6], "d": 1.45}
            ch, cw = min(H, 2048), min(W, 2048)
            crop = free[:ch, :cw].contiguous()
            mc = 1 << 22
            grid = torch.zeros(mc, dtype=torch.uint8, device=dev)
            grid[:ch * cw] = crop.reshape(-1)
            dims = torch.tensor([ch, cw], dtype=torch.int32, device=dev)
            density = torch.zeros(mc, dtype=torch.int32, device=dev)
            height = torch.zeros(mc, dtype=torch.float32, device=dev)
            origin = torch.zeros(2, dtype=torch.float64, device=dev)
            calls = {
                "depth_to_image_color": (lambda: ops.depth_to_image(depth, True, "turbo", out=col, scratch=mm), px),
                "gradient": (lambda: SH.gradient_magnitude(depth), px),
                "edges": (lambda: SH.edge_mask(depth, thr), px),
                "regions": (lambda: SH.small_region_mask(free, 100), px),
                "chain": (lambda: SH.find_depth_shadows(depth, thr, 100), px),
                "chain_drop": (lambda: SH.find_depth_shadows(depth, thr, 100, drop=True), px),
                "fill": (lambda: SH.fill_ground_shadows(depth, shadow["mask"], plane), px),
                "regions_crop": (lambda: SH.small_region_mask(crop, 100), ch * cw),
                "grid_regions_crop": (lambda: PC.grid_regions(grid, dims, density, height, origin), ch * cw),
            }
            r = {"ms": {k: [] for k in calls}}
            for _ in range(args.repeats):
                for k, (call, _) in calls.items():
                    r["ms"][k].append(timed(call, args.iters))
            r["best_us"] = {k: 1e3 * min(v) for k, v in r["ms"].items()}
            r["tb_per_s"] = {k: MUST_MOVE[k] * calls[k][1] / (r["best_us"][k] * 1e-6) / 1e12 for k in calls if k in MUST_MOVE}
            r["stage_us"] = {"gradient": r["best_us"]["gradient"], "threshold": r["best_us"]["edges"] - r["best_us"]["gradient"],
                             "regions": r["best_us"]["regions"]}
            r["crop"] = [ch, cw]
            r["grid_regions_over_regions_on_crop"] = r["best_us"]["grid_regions_crop"] / r["best_us"]["regions_crop"]
            r["chain_over_yardstick"] = r["best_us"]["chain"] / r["best_us"]["depth_to_image_color"]
            r["stats"] = SH.shadows_summary(shadow)["stats"]
            res["sizes"][size][kind] = r
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
