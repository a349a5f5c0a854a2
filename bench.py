#!/usr/bin/env python3
"""Depth Pro frames/sec at 1536x1536 on 1..8 MI355X (one process per GPU).

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N ...

A plain run sets up, warms up, times the K steps and prints the result line.  `--dump-outputs DIR`
also writes what the last timed step returned as DIR/<name>.npy.  `--full` adds the legs that take
runs of their own: per-kernel / roofline figures, depth parity vs the reference, the CPU baseline.

A step = every rank runs `DepthPro.infer(transform(frame))` on one synthetic 1536x1536
uint8 frame that is already resident in HBM (transform: u8 -> normalised fp32 on the GPU;
infer: copy into the engine input -> hipGraph forward -> depth epilogue -> frame status), and
(N > 1) the depth maps are gathered to rank 0 over RCCL.
Weights: synthetic seed-0 set (no checkpoint offline), packed once on rank 0
and RCCL-broadcast.  Prints ONE JSON line on rank 0.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "ml-depth-pro-video_amd"))

FLOP_PER_FRAME = 19.247e12      # 2 x (9,018.2 conv/linear + 605.5 attention) GMAC
PEAK_BF16_TFLOPS = 2500.0       # MI355X dense bf16/f16 MFMA (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0


TILE_NAMES = {1: "128x128", 2: "256x64", 3: "256x32", 4: "256x256", 5: "256x128", 8: "8phase-256x256",
              12: "streamK-256x256", 13: "320x256", 14: "512x128", 17: "dual-256x128",
              18: "persistent-8phase-256x256", 19: "8phase-320x256",
              20: "patch-conv3x3-256x256"}
TILE_KERNEL = {1: "gemm_kernel<{K}, 128, 128", 4: "gemm_big_kernel<{K}, 256, 256", 5: "gemm_big_kernel<{K}, 256, 128",
               8: "gemm_8ph_kernel<{K}", 12: "gemm_sk_kernel<{K}", 13: "gemm_big_kernel<{K}, 320, 256",
               14: "gemm_big_kernel<{K}, 512, 128", 17: "gemm_big_kernel<{K}, 256, 128, 32, 3",
               18: "gemm_p8ph_kernel<{K}", 19: "gemm_8ph320_kernel<{K}",
               20: "gemm_cv3_kernel<{K}"}


def tile_kernel(tile: int, dtype: torch.dtype) -> str:
    """Kernel-name prefix (as rocprofv3 prints it) of the GEMM engine `tile` for operand type `dtype`."""
    t = TILE_KERNEL.get(tile)
    return t.format(K="KBF16" if dtype == torch.bfloat16 else "KF16") if t else ""


# The PMC traffic summary the bench line cites (tools/pmc_traffic.py over separate FETCH_SIZE /
# WRITE_SIZE passes of the tree being benched); named explicitly, updated with each profiled tree.
PMC_TRAFFIC = "profiles/r06_pmc_traffic.json"


def pmc_traffic(kernel: str, workgroups: int):
    """HBM bytes per launch of `kernel` at `workgroups` from PMC_TRAFFIC (FETCH_SIZE doubled per
    the gfx950 correction), or None when that summary has no such launch."""
    path = os.path.join(REPO, PMC_TRAFFIC)
    try:
        data = json.load(open(path))
    except (OSError, ValueError):
        return None
    for k in data.get("kernels", []):
        if k["workgroups"] == workgroups and k["kernel"].startswith(kernel):
            return {"bytes_per_launch": round(k["read_bytes_per_launch"] + k["write_bytes_per_launch"]),
                    "source": PMC_TRAFFIC}
    return None


# The rocprofv3 --kernel-trace --stats summary of this tree's bench run (tools/gpu_check.sh prof,
# copied from gpurun_out/): the dominant kernel's average duration there (every launch of it in that run:
# graph replays, where it overlaps other streams, and the instrumented frames) is reported beside the live
# HIP-event figure, so the line's roofline fraction can be checked against the committed profile.
PROF_STATS = "profiles/r06_kernel_stats.csv"


def rocprof_avg_us(kernel: str):
    """(average us, calls) of the kernels whose name starts with `kernel` in PROF_STATS, or None."""
    import csv
    path = os.path.join(REPO, PROF_STATS)
    try:
        rows = list(csv.DictReader(open(path)))
    except OSError:
        return None
    def bare(name):   # "void (anonymous namespace)::gemm_p8ph_kernel<...>(dpg::GemmP)" -> "gemm_p8ph_kernel<...>..."
        return name.replace("void ", "", 1).replace("(anonymous namespace)::", "")
    hit = [r for r in rows if bare(r["Name"]).startswith(kernel)]
    if not hit:
        return None
    calls = sum(int(r["Calls"]) for r in hit)
    ns = sum(float(r["TotalDurationNs"]) for r in hit)
    return ns / calls / 1e3, calls


def frame(seed: int) -> np.ndarray:
    return np.random.default_rng(seed=seed).integers(0, 256, (1536, 1536, 3), dtype=np.uint8)


def depth_parity(depth: torch.Tensor, canonical: torch.Tensor, fov: torch.Tensor) -> dict:
    """The "+ depth L1 vs reference" half of the metric, on synthetic frame 0 / seed-0 weights.

    Reference = tests/golden/golden_forward_frame0.npz (the reference's own DepthPro.forward on
    the same frame and weights, tests/golden/make_golden.py): canonical inverse depth every 8th
    pixel + fov_deg.  Its depth follows the reference infer epilogue (depth_pro.py:282-298):
    f_px = 0.5 W / tan(0.5 rad(fov)); depth = 1 / clamp(canonical * W / f_px, 1e-4, 1e4).
    Metric: relative L1 = mean|x - x_ref| / mean|x_ref| over the 192 x 192 grid.
    """
    path = os.path.join(REPO, "tests", "golden", "golden_forward_frame0.npz")
    if not os.path.exists(path):
        return None
    g = np.load(path)
    c_ref = g["canonical_sub8"].astype(np.float64)
    fov_ref = float(g["fov_deg"][0])
    W = 1536.0
    f_ref = 0.5 * W / np.tan(0.5 * np.deg2rad(fov_ref))
    d_ref = 1.0 / np.clip(c_ref * (W / f_ref), 1e-4, 1e4)
    d = depth[::8, ::8].double().cpu().numpy()
    c = canonical.reshape(1536, 1536)[::8, ::8].double().cpu().numpy()
    rel = lambda a, b: float(np.abs(a - b).mean() / np.abs(b).mean())  # noqa: E731
    return {"depth_rel_l1": round(rel(d, d_ref), 7), "canonical_rel_l1": round(rel(c, c_ref), 7),
            "fov_rel_err": round(abs(float(fov.reshape(-1)[0]) - fov_ref) / fov_ref, 7),
            "target": 1e-3, "frame": "synthetic frame 0 (1536x1536), graph replay, every 8th pixel",
            "reference": "tests/golden/golden_forward_frame0.npz"}


DUMP_BUDGET = 64 << 20          # bytes of .npy data per --dump-outputs directory


def dump_outputs(path: str, pred: dict, gathered=None) -> None:
    """--dump-outputs: what the last timed step returned to its caller, as <path>/<name>.npy (float32).

    `pred` is that step's `DepthPro.infer` result on this rank (depth map + focal length); `gathered`
    (N > 1) the depth maps rank 0 received for that step, in rank order.  When the gathered maps
    would not fit DUMP_BUDGET beside the rest, a fixed seeded sample of their pixels (the same
    pixels of every map, from default_rng(0)) is written with its flat indices."""
    os.makedirs(path, exist_ok=True)
    arrays = {name: t.detach().float().cpu().numpy() for name, t in pred.items()}
    if gathered is not None:
        maps = np.stack([t.detach().float().cpu().numpy() for t in gathered])
        room = DUMP_BUDGET - sum(a.nbytes for a in arrays.values())
        per_map = maps[0].size
        keep = room // (maps.shape[0] * 4 + 8)         # float32 per map + one int64 index
        if keep < per_map:
            idx = np.sort(np.random.default_rng(seed=0).choice(per_map, size=keep, replace=False))
            arrays["depth_gathered_index"] = idx.astype(np.float64)
            maps = maps.reshape(maps.shape[0], -1)[:, idx]
        arrays["depth_gathered"] = maps
    assert sum(a.nbytes for a in arrays.values()) <= DUMP_BUDGET
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline() -> dict:
    """The fp32 CPU oracle (a port of the reference path) on one synthetic frame.

    Bounded sample (~20 s on 16 host threads, BASELINE.md "CPU baseline"): one untimed
    warm-up of a ViT block at the patch-encoder shape (thread pool + allocator), then one
    timed frame through the oracle's `infer`.  One frame, not a median of three: a frame takes
    ~20 s, and the baseline leg is bounded to 10-30 s of CPU work so that the default bench
    finishes within minutes; the box-to-box spread is reported in DESIGN.md instead.
    """
    from depth_pro.weights import synthetic_state_dict
    from oracle import depth_pro_oracle as O

    threads = min(len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS", "16") or 16))
    torch.set_num_threads(threads)
    sd = synthetic_state_dict(0)
    x = O.transform(frame(0))
    with torch.no_grad():
        O.vit_block(sd, "encoder.patch_encoder.blocks.0.", torch.zeros(1, 577, 1024))
    t0 = time.time()
    with torch.no_grad():
        O.infer(sd, x)
    dt = time.time() - t0
    return {"value": 1.0 / dt, "unit": "frames/sec", "cores": threads, "kind": "port",
            "cpu_model": cpu_model(),
            "sample": f"1 synthetic 1536x1536 frame through oracle/depth_pro_oracle.infer (fp32 torch CPU, "
                      f"after a 1-block warm-up), {dt:.1f} s"}


def refuse(msg: str, code: int) -> None:
    """Exit non-zero WITHOUT a bench line: a number from such a run would be meaningless."""
    print(json.dumps({"error": msg, "value": None}), flush=True)
    print(f"bench.py: {msg}", file=sys.stderr, flush=True)
    sys.exit(code)


def launch_ranks(n: int) -> None:
    """`python bench.py --gpus N` (N > 1) outside a torch.distributed launcher: start the N ranks
    here, one process per GPU (torch.distributed.run, rendezvous on 127.0.0.1), before this process
    makes any GPU call, and exit with the launcher's status.  Fails (non-zero) when fewer than N
    devices are visible, so the line can never report fewer GPUs than requested."""
    import socket
    import subprocess

    ndev = torch.cuda.device_count()       # counts devices without initialising HIP
    if ndev < n:
        refuse(f"--gpus {n} requested but only {ndev} GPU(s) are visible", 2)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", f"--master-port={port}", os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd))


def timed_steps(infer_one, steps: int, warmup: int, world: int, dev: torch.device, sync=None,
                on_gathered=None) -> dict:
    """The measured loop of every rank (also driven over gloo by tests/test_bench_cli.py with a
    stub model): `warmup` untimed steps, then exactly `steps` timed ones between a barrier +
    device synchronisation on both sides; the elapsed time is the MAX over ranks (all_reduce).

    Step n: `infer_one(n) -> (depth, status)` runs this rank's next frame (frame k -> rank
    k mod world); for world > 1 its depth map is gathered to rank 0 asynchronously (RCCL's own
    stream) while the next frame computes -- double-buffered: a depth tensor stays referenced until
    its gather's wait(), which step n + 2 (or the drain) issues.  On rank 0,
    `on_gathered(n, bufs)` sees step n's gathered maps (rank order) after that wait.
    Returns {"elapsed": s (max over ranks), "statuses": [...], "frames_total": steps * world}."""
    from depth_pro import distributed as D

    sync = sync or torch.cuda.synchronize
    pending = [None, None]
    statuses = []          # status of every infer call of this rank (checked after the timed loop)
    counter = [0]

    def retire(j):
        d, bufs, work, n = pending[j]
        work.wait()
        if on_gathered is not None and bufs is not None:
            on_gathered(n, bufs)
        pending[j] = None

    def step(i):
        if pending[i & 1] is not None:
            retire(i & 1)
        n = counter[0]
        counter[0] += 1
        d, st = infer_one(n)
        statuses.append(st)
        if world > 1:
            bufs, work = D.gather_frames(d, dst=0, async_op=True)
            pending[i & 1] = (d, bufs, work, n)

    def drain(i0):
        for j in (i0 & 1, (i0 + 1) & 1):     # oldest first: rank 0 sees the steps in order
            if pending[j] is not None:
                retire(j)

    for i in range(warmup):
        step(i)
    drain(warmup)
    sync()
    if world > 1:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for i in range(steps):
        step(i)
    drain(steps)
    sync()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()
    return {"elapsed": elapsed, "statuses": statuses, "frames_total": steps * world}


# environment switches and their product defaults: a bench line is only printed for the defaults
AB_KNOBS = {"DP_ABLATE": "0", "DP_GEMM_DEBUG": "0"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", choices=["bf16", "fp16", "mixed"], default="mixed",
                    help="compute precision: bf16 / fp16 everywhere, or mixed = bf16 ViTs + f16 maps, "
                         "decoder and heads (depth_pro.depth_pro.PRECISION_MODES)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline leg")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last one returned (rank 0) as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs beside the headline figure: per-kernel / roofline timing, depth "
                         "parity vs the reference, and (1 GPU, unless --no-cpu-baseline) the CPU baseline")
    ap.add_argument("--pool", type=int, default=4, help="distinct resident frames per rank")
    ap.add_argument("--ab", action="store_true",
                    help="A/B timing run (tools/ab_env.sh): allows the AB_KNOBS switches off their defaults and reports "
                         "'ab_fps' instead of a bench 'value'")
    args = ap.parse_args()

    # a run whose results are wrong by construction (ablations) or whose schedule is not the product's
    # (debug switches) prints no value
    forced = [v for v, dflt in AB_KNOBS.items() if os.environ.get(v, dflt) not in ("", dflt)]
    if forced and not args.ab:
        refuse(f"{', '.join(forced)} set: ablation / debug / schedule switches off their defaults make the "
               f"frame invalid or not the product's (use --ab)", 3)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        launch_ranks(args.gpus)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        refuse(f"--gpus {args.gpus} but the launcher started {world} rank(s)", 2)
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)
    os.environ["DEPTH_PRO_COMPUTE_DTYPE"] = args.dtype

    import depth_pro
    from depth_pro import distributed as D
    from depth_pro import _lib, ops
    from depth_pro.depth_pro import DepthPro, DepthProConfig, Transform, _compute_dtype
    from depth_pro.engine import pack_weights
    from depth_pro.weights import synthetic_state_dict

    t_setup = time.time()
    code = _compute_dtype(torch.float32)
    if world > 1:
        packed = None
        if rank == 0:
            packed = pack_weights(synthetic_state_dict(0), dev, code)
        packed = D.broadcast_packed(packed, dev, src=0)
    else:
        packed = pack_weights(synthetic_state_dict(0), dev, code)
    # the drop-in API object (depth_pro.DepthPro), on the packed weight set (rank 0's, broadcast)
    model = DepthPro.from_packed(packed, dev, code)
    transform = Transform(dev, torch.float32)
    eng = model.engine()
    if not args.no_graph:
        eng.capture_graph()
    torch.cuda.synchronize()
    t_setup = time.time() - t_setup

    # resident inputs: this rank's first `pool` frames of the stream (frame k -> rank k mod N), u8 in HBM
    frames = [torch.from_numpy(frame(k)).to(dev) for k in D.shard_frames(args.pool * world, rank, world)]

    def infer_one(n):
        # the user's call: transform (u8 -> normalised fp32 on the GPU) + DepthPro.infer (copy into
        # the engine input, graph replay of the forward, depth / focal-length epilogue, status)
        with torch.no_grad():
            pred = model.infer(transform(frames[n % len(frames)]))
        last["pred"] = pred
        return pred["depth"], model.last_status()

    def keep_gathered(n, bufs):
        last["gathered"] = bufs          # step n's depth maps at rank 0; the final call is the last timed step's

    last = {}
    dump = args.dump_outputs and rank == 0
    run = timed_steps(infer_one, args.steps, args.warmup, world, dev,
                      on_gathered=keep_gathered if dump and world > 1 else None)
    elapsed, statuses = run["elapsed"], run["statuses"]
    frames_total = run["frames_total"]
    fps = frames_total / elapsed
    ms_per_step = 1000.0 * elapsed / args.steps
    fps_per_gpu = fps / world

    # every benched frame healthy: no timed-out stream-K hand-off, depth / focal length all finite
    bad = [st for st in statuses if st.error() is not None]
    if bad and not args.ab:
        refuse(f"rank {rank}: {len(bad)} of {len(statuses)} benched infer calls invalid "
               f"(first: {bad[0].error()})", 5)

    if dump:
        dump_outputs(args.dump_outputs, last["pred"], last.get("gathered"))

    # --full: the legs beside the headline figure (rank 0), each a run of its own after the timed steps
    full = args.full and rank == 0

    # per-kernel leg (rank 0): instrumented eager frames with HIP events on the launching stream
    # around every launch, grouped by (kernel kind, shape).  `groups`: a SERIAL frame (every launch on
    # one stream, alone on the chip -- as in a rocprofv3 kernel trace, which serialises the graph's
    # streams): its intervals are disjoint, so the per-kind table sums to the serial kernel time of a
    # frame, and the dominant kernel's average is comparable with the committed rocprof summary.
    # `groups_cc`: the product's concurrent stream layout (side encoders / decoder chains beside the
    # main stream), where an interval also holds the time a launch waited for CUs other streams held:
    # reported for the dominant kernel only, as its in-frame figure.
    groups, groups_cc = {}, {}
    serial_frame_ms = None
    if full:
        ops.normalize_u8(frames[0], eng.x0)
        for _ in range(2):
            eng.forward()                   # warm (no graph)
        for serial, grp in ((True, groups), (False, groups_cc)):
            eng.serial_side = serial
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ops.profile_begin()
            e0.record()
            eng.forward()
            e1.record()
            rec = ops.profile_end()
            if serial:
                serial_frame_ms = e0.elapsed_time(e1)
            for kind, flops, shape, kdt, ms in rec:
                k = grp.setdefault((kind, shape, kdt), {"launches": 0, "ms": 0.0, "flop": 0.0})
                k["launches"] += 1
                k["ms"] += ms
                k["flop"] += flops
        eng.serial_side = False

    parity = None
    if full:
        # frame 0 through the API (graph replay) against the reference's output
        x = transform(frames[0])
        with torch.no_grad():
            c, fov = model.forward(x.unsqueeze(0))
            depth = model.infer(x)["depth"]
        torch.cuda.synchronize()
        parity = depth_parity(depth, c, fov)
        if not args.ab:
            model.last_status().check()
        if parity is None:
            refuse("tests/golden/golden_forward_frame0.npz missing: depth L1 vs reference not measurable", 4)
        if not args.ab and not parity["depth_rel_l1"] < parity["target"]:
            refuse(f"depth rel-L1 {parity['depth_rel_l1']} >= {parity['target']} vs the reference", 4)

    if full:
        achieved = fps_per_gpu * FLOP_PER_FRAME / 1e12
        kern = {}
        for (kind, shape, _), g in groups.items():
            k = kern.setdefault(kind, {"launches": 0, "ms": 0.0, "flop": 0.0})
            for f in ("launches", "ms", "flop"):
                k[f] += g[f]
        for k in kern.values():
            k["tflops"] = k["flop"] / (k["ms"] * 1e-3) / 1e12 if k["ms"] > 0 else None
            k["avg_us"] = 1000.0 * k["ms"] / k["launches"]
        dom_key = max(groups, key=lambda key: groups[key]["ms"])
        dom = groups[dom_key]
        dom_avg_us = 1000.0 * dom["ms"] / dom["launches"]
        dom_flop = dom["flop"] / dom["launches"]
        dom_tf = dom_flop / (dom_avg_us * 1e-6) / 1e12
        dom_info = {"kind": dom_key[0], "shape": list(dom_key[1]), "dtype": str(dom_key[2]).replace("torch.", ""),
                    "launches_per_frame": dom["launches"],
                    "avg_us": round(dom_avg_us, 2), "flop_per_launch": dom_flop,
                    "timing": "HIP events around each launch in a serial eager frame (alone on the chip)",
                    "share_of_frame_kernel_time": round(dom["ms"] / sum(g["ms"] for g in groups.values()), 3)}
        cc = groups_cc.get(dom_key)
        if cc:
            dom_info["in_frame_concurrent_avg_us"] = round(1000.0 * cc["ms"] / cc["launches"], 2)
        traffic = None
        if dom_key[0].startswith("gemm"):
            M, N, K = dom_key[1]
            kdt = dom_key[2]
            A = torch.empty(8, dtype=kdt, device=dev)
            tile, wgs = ops.gemm(A, A, A, M=M, N=N, K=K, plan_only=True, workspace=eng.ws_main)
            kname = tile_kernel(tile, kdt)
            meta = ops.PROF_GEMM_META.get(dom_key)
            if tile == _lib.DP_TILE_P8PH_256x256 and meta is not None:
                # the persistent engine runs the folded-LN qkv and fc1 and the decoder's deconvs: its
                # instantiation is <K_, RELU, ACT, HG, DCV, LNC> (dp_gemm_impl.h, launch_part_8ph)
                b = lambda v: "true" if v else "false"  # noqa: E731
                kname += f", false, {meta['act']}, false, {b(meta['deconv'])}, {b(meta['ln_consumer'])}>"
            dom_info["engine"] = {"tile": TILE_NAMES.get(tile, tile), "workgroups": wgs, "kernel": kname}
            traffic = pmc_traffic(kname, wgs) if kname else None
            if traffic is not None:
                dom_info["traffic_source"] = traffic.pop("source")
            rp = rocprof_avg_us(kname) if kname else None
            if rp is not None:
                # same kernel in the committed rocprofv3 summary (every launch of it in that bench run)
                dom_info["rocprof"] = {"source": PROF_STATS, "avg_us": round(rp[0], 2), "calls": rp[1],
                                       "frac": round(dom_flop / (rp[0] * 1e-6) / 1e12 / PEAK_BF16_TFLOPS, 4)}

    if rank == 0:
        out = {
            "metric": "frames/sec at 1536x1536 (1/2/4/8 MI355X) + depth L1 vs reference",
            "value": round(fps, 3),
            "unit": "frames/sec",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": {"bf16": "bf16", "fp16": "f16", "mixed": "bf16+f16"}[args.dtype],
            "data": "synthetic (uint8 1536x1536 frames from numpy default_rng(k); synthetic seed-0 weights, "
                    "full Depth Pro architecture, 951,991,330 params)",
            "config": {"workload": ("BASELINE config 2/3: one 1536x1536 frame per GPU per step through "
                                    "DepthPro.infer (patch+image+FOV ViT-L, decoder, heads), hipGraph replay"),
                       "global_batch": world, "frame": [1536, 1536], "parallelism": f"frame-dp{world}",
                       "graph": not args.no_graph,
                       "precision": {"bf16": "bf16 everywhere", "fp16": "f16 everywhere",
                                     "mixed": "bf16 MFMA operands in the three ViT-L encoders, f16 in the "
                                              "encoder maps / decoder / heads (fp32 accumulate; the patch "
                                              "encoder's residual stream held split as a 16-bit hi part + an "
                                              "int8 lo part, ~16 significant bits, the side encoders' in "
                                              "fp32): the default, chosen to meet depth L1 < 1e-3"
                                     }[args.dtype]},
            "setup_s": round(t_setup, 1),
        }
    if full:
        out.update({
            # dominant kernel: algorithmic FLOP per launch / its average HIP-event duration
            "roofline": {"bound": "mfma", "achieved": round(dom_tf, 1), "peak": PEAK_BF16_TFLOPS,
                         "unit": "TFLOP/s", "frac": round(dom_tf / PEAK_BF16_TFLOPS, 4),
                         "traffic": traffic["bytes_per_launch"] if traffic else None,
                         "dominant_kernel": dom_info,
                         "frame": {"achieved": round(achieved, 1), "frac": round(achieved / PEAK_BF16_TFLOPS, 4),
                                   "basis": "fps_per_gpu x 19.247 TFLOP/frame (SURVEY 8d)"}},
            # per-kind launch times of one SERIAL eager frame (disjoint intervals: they sum to
            # serial_frame_kernel_ms; the graph-replayed step overlaps streams, so it is shorter)
            "kernels": {k: {kk: (round(vv, 3) if isinstance(vv, float) else vv) for kk, vv in v.items()}
                        for k, v in kern.items()},
            "kernels_basis": {"frame": "serial eager (every launch on one stream)",
                              "serial_frame_ms": round(serial_frame_ms, 3),
                              "serial_frame_kernel_ms": round(sum(k["ms"] for k in kern.values()), 3)},
            "parity": parity,
        })
    if rank == 0:
        if args.ab:        # A/B timing run: not a bench result
            out["metric"] = "A/B timing run (DP_GEMM_DEBUG / DP_ABLATE allowed): not a bench result"
            out["ab_fps"], out["value"] = out["value"], None
            out["ab_env"] = {v: os.environ.get(v, "") for v in AB_KNOBS}
        elif full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline()
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
