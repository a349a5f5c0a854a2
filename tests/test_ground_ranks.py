"""The ground plane's way through a 2-rank process group (gloo, CPU): `generate_depth_maps._ground_plane`.

Rank 0 alone reads `ground.json`; every rank takes part in exactly one broadcast per run, also when
there is no plane to share, and remembers the outcome (a second collective that rank 0 never joins
would hang the group)."""

import json
import multiprocessing as mp
import os
import socket

import numpy as np
import torch.distributed as dist

MODEL = {"normal": [0.01, 0.99, 0.05], "d": 1.25, "origin": [0.0, -1.2626262626262625, 0.0]}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, gdir, rot, q):
    import generate_depth_maps as G

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ground = {"model": None, "dir": gdir, "grid": 20, "pct": 5, "rot": rot, "resolved": False, "world": world,
                  "rank": rank}
        first = G._ground_plane(ground, None, None, None)     # a rank without a frame at hand
        calls = []
        real = dist.broadcast
        dist.broadcast = lambda *a, **k: calls.append(1) or real(*a, **k)
        second = G._ground_plane(ground, None, None, None)    # remembered: no further collective
        dist.broadcast = real
        dist.barrier()
        vec = None if first is None else np.concatenate([first["normal"], [first["d"]], first["origin"]]).tolist()
        q.put((rank, vec, second is first, len(calls)))
    finally:
        dist.destroy_process_group()


def _run(gdir, rot):
    port, ctx = _free_port(), mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, gdir, rot, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    return {m[0]: m[1:] for m in (q.get(timeout=5) for _ in range(2))}


def test_plane_from_ground_json_reaches_every_rank(tmp_path):
    with open(tmp_path / "ground.json", "w") as f:
        json.dump(MODEL, f, indent=4)
    res = _run(str(tmp_path), [0.0, 0.0, 0.0])
    want = MODEL["normal"] + [MODEL["d"]] + MODEL["origin"]
    for rank in (0, 1):
        vec, same, calls = res[rank]
        assert vec == want and same and calls == 0
    # a rotation offset is applied on every rank alike, after the broadcast
    rot = _run(str(tmp_path), [2.0, 0.0, -1.0])
    assert rot[0][0] == rot[1][0] and rot[0][0] != want


def test_no_plane_is_shared_once_and_remembered(tmp_path):
    res = _run(str(tmp_path), None)          # no ground.json, no frame to fit: "no plane" for both ranks
    for rank in (0, 1):
        vec, same, calls = res[rank]
        assert vec is None and same and calls == 0
