#!/usr/bin/env python3
"""The GEMM planner's recorded plan table (host only: no GPU, no torch device).

Generates a deterministic list of dp_gemm_args and records what dp_gemm_plan answers for each:
(rc, tile, grid).  tests/golden/gemm_plan_table.npz holds the answers of the library the table was
last recorded from; tests/test_gemm_plan_table.py holds the current library to them row for row, so
a change to the planner shows exactly which launches it re-routes.

The list: the frame's launches (the shapes of tests/test_abi.py::test_gemm_plan_tile_choice, the
CASES of tests/test_gemm_contract.py, the RC_CASES of tests/test_ln_fold_contract.py) and
perturbations around each (M +- one tile and at the 600-tile / 2 x CU thresholds, N, K, the map
side, c_dtype, accumulate, relu_a, act, R1, ldc % 8 != 0, M * in_c on both sides of 2^30).  Every problem
is planned under every tile hint 0..23 with and without a workspace; every launch again under each
planner-read debug bit (the perturbations under DP_TILE_AUTO only there).  A perturbation changes one
field and what that field drags along (ldc == N follows N, lda / ldb == K follow K, a conv's in_c
follows K, M and the out side follow the map side).  The planner never dereferences an operand
pointer: every non-null one is the dummy address 256.

    python tools/gemm_plan_table.py --check          # compare the built library with the table
    python tools/gemm_plan_table.py --write          # re-record (after re-routing a launch on purpose)
    python tools/gemm_plan_table.py --time 5         # seconds per pass over the whole list (through ctypes)
    python tools/gemm_plan_table.py --dump FILE      # the list for tools/gemm_plan_time.cpp (the planner alone)
DP_MI355X_LIB selects another build of the library (how the table was first recorded at the parent
of the planner refactor: profiles/gemm_plan_refactor/README.md).
"""
import argparse
import ctypes
import hashlib
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "tests"), os.path.join(REPO, "ml-depth-pro-video_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
from depth_pro import _lib, ops  # noqa: E402
from depth_pro._lib import GemmArgs  # noqa: E402

TABLE = os.path.join(REPO, "tests", "golden", "gemm_plan_table.npz")
N_TILES = 24
NUM_CUS = 256              # MI355X; dp_gemm_plan's fallback without a device is the same
PTR = 256                  # every non-null pointer (never dereferenced by the planner)
DEBUG_BITS = (32, 1024, 2048, 4096, 8192, 16384, 1 << 15, 1 << 16, 1 << 20, 1 << 22, 1 << 23, 1 << 25)
SIDES = (48, 96, 192, 384, 768, 200)       # 200: not a multiple of 16
RC_CODE = {0: 0, 1000: 1, 1001: 2, 1002: 3, 1003: 4}     # the int8 `rc` column
RC_NAME = ["ok", "DP_ERR_ARG", "DP_ERR_SHAPE", "DP_ERR_ALIGN", "DP_ERR_DTYPE"]
TILE_NAME = {v: k[len("DP_TILE_"):] for k, v in vars(_lib).items() if k.startswith("DP_TILE_")}
AUTO_TILES = ("256x32", "256x64", "128x128", "BIG_256x128", "BIG_256x256", "BIG_320x256", "BIG_512x128",
              "8PH_256x256", "STREAMK_256x256", "PBIG_320x256", "PBIG_256x256", "P8PH_256x256", "8PH_320x256",
              "CV3_256x256", "CV3_192x256", "CV3_384x128")
_POINTERS = [f for f, t in GemmArgs._fields_ if t is ctypes.c_void_p]


def _copy(a, **kw):
    b = GemmArgs.from_buffer_copy(bytes(a))
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _normalized(a):
    """`a` with the dummy address in every non-null pointer, DP_TILE_AUTO and no workspace."""
    b = _copy(a, tile=0, workspace=None, workspace_bytes=0)
    for f in _POINTERS:
        if getattr(b, f):
            setattr(b, f, PTR)
    return b


# ---------------------------------------------------------------------------------- the launches
def _dense(M, N, K, **kw):
    return _copy(GemmArgs(), **dict(dict(M=M, N=N, K=K, A=PTR, B=PTR, C=PTR, lda=K, ldb=K, ldc=N), **kw))


def _conv(S, cin, N=256, K=None, **kw):
    return _dense(S * S, N, 9 * cin if K is None else K, a_mode=_lib.DP_A_CONV, in_h=S, in_w=S, in_c=cin, k_h=3, k_w=3,
                  stride=1, pad=1, out_h=S, out_w=S, **kw)


def _deconv(S, cin, cout, **kw):
    return _dense(S * S, 4 * cout, cin, store_mode=_lib.DP_STORE_DECONV2X2, dc_h=S, dc_w=S, dc_cout=cout, ldc=cout,
                  dtype=_lib.DP_F16, c_dtype=_lib.DP_F16, bias=PTR, **kw)


def frame_shapes():
    """(label, args) of tests/test_abi.py::test_gemm_plan_tile_choice, and the composed head's compact form."""
    big_m = (1 << 21) + 5
    hps = dict(N=128, head_corr=PTR, store_mode=_lib.DP_STORE_HEAD_PS, head_w=PTR, c_dtype=_lib.DP_F32)
    return [
        ("vit qkv", _dense(20195, 3072, 1024)), ("vit proj", _dense(20195, 1024, 1024)),
        ("vit fc1", _dense(20195, 4096, 1024)), ("side qkv", _dense(577, 3072, 1024)),
        ("head.0 dense", _dense(768 * 768, 128, 2304)), ("A past 2^31, N 1024", _dense(big_m, 1024, 1024)),
        ("A past 2^31, N 4096", _dense(big_m, 4096, 1024)), ("A below 2^31", _dense(big_m - 8, 1024, 1024)),
        ("conv 48^2 x 1024", _conv(48, 1024)), ("conv 96^2 x 1024", _conv(96, 1024)),
        ("conv 192^2 x 512", _conv(192, 512)), ("conv 48^2 x 256", _conv(48, 256)),
        ("conv 768^2 x 256", _conv(768, 256)), ("conv 384^2 x 256", _conv(384, 256)),
        ("head.0 composed", _conv(768, 256, N=128, head_corr=PTR)),
        ("head pixel-shuffle", _conv(768, 128, **hps)), ("head pixel-shuffle compact", _conv(768, 128, K=4 * 128, **hps)),
        ("deconv 384^2", _deconv(384, 256, 256)), ("deconv 192^2", _deconv(192, 256, 256)),
        ("deconv 96^2 x 512", _deconv(96, 512, 512)), ("deconv 96^2", _deconv(96, 256, 256)),
        ("deconv 48^2", _deconv(48, 256, 256)), ("deconv 384^2 relu", _deconv(384, 256, 256, act=_lib.DP_ACT_RELU)),
    ]


def launches():
    import test_gemm_contract as gc
    import test_ln_fold_contract as lc

    out = [("frame: " + n, a) for n, a in frame_shapes()]
    cpu = torch.device("cpu")
    for ci, c in enumerate(gc.CASES):
        P = gc.problem(ci, torch.bfloat16)
        A, B, kw = gc.gemm_kwargs(P, cpu)
        out.append(("contract: " + c["name"], _normalized(ops._gemm_args(A, B, gc.prefill(P), **kw))))
    for c in lc.RC_CASES:
        out.append(("ln: " + c["name"], _normalized(lc.ln_args(c, 0))))
    return out


# ------------------------------------------------------------------------------ the perturbations
def perturbations(a):
    """(label, args): one-field changes around the launch `a`."""
    out = []

    def put(label, **kw):
        out.append((label, _copy(a, **kw)))

    conv, deconv = a.a_mode == _lib.DP_A_CONV, a.store_mode == _lib.DP_STORE_DECONV2X2
    nt = max(1, a.N // 256)
    for lab, M in (("M - 256", a.M - 256), ("M + 256", a.M + 256),
                   ("599 tiles", (-(-600 // nt)) * 256 - 256), ("600 tiles", (-(-600 // nt)) * 256),
                   ("2 CUs of tiles - 1", (-(-2 * NUM_CUS // nt)) * 256 - 256), ("2 CUs of tiles", (-(-2 * NUM_CUS // nt)) * 256)):
        if M > 0:
            put(lab, M=M)
    for N in (32, 64, 128, 136, 256, 1024):
        put(f"N = {N}", N=N, **(dict(ldc=N) if a.ldc == a.N else {}))
    for K in (64, 128, 256, 1024, 2304, 4608):
        kw = dict(K=K)
        if conv and a.k_h * a.k_w > 0 and K % (a.k_h * a.k_w) == 0:
            kw.update(in_c=K // (a.k_h * a.k_w))
        for ld in ("lda", "ldb"):
            if getattr(a, ld) == a.K:
                kw[ld] = K
        put(f"K = {K}", **kw)

    def side(S, label, **kw):
        if conv and a.out_h > 0 and a.out_w > 0 and a.stride > 0:
            o = (S + 2 * a.pad - a.k_h) // a.stride + 1
            put(label, in_h=S, in_w=S, out_h=o, out_w=o, M=max(1, a.M // (a.out_h * a.out_w)) * o * o, **kw)
        elif deconv and a.dc_h > 0 and a.dc_w > 0:
            put(label, dc_h=S, dc_w=S, M=max(1, a.M // (a.dc_h * a.dc_w)) * S * S, **kw)

    for S in SIDES:
        side(S, f"side {S}")
    put("c_dtype", c_dtype=a.dtype if a.c_dtype == _lib.DP_F32 else _lib.DP_F32)
    put("accumulate", accumulate=0 if a.accumulate else 1)
    put("relu_a", relu_a=0 if a.relu_a else 1)
    for act, lab in ((_lib.DP_ACT_NONE, "none"), (_lib.DP_ACT_RELU, "relu"), (_lib.DP_ACT_GELU, "gelu")):
        if act != a.act:
            put(f"act {lab}", act=act)
    if a.R1:
        put("no R1", R1=None)
    else:
        put("R1", R1=PTR, ldr1=a.N)
    put("ldc + 4", ldc=a.ldc + 4)
    # M * in_c on both sides of 2^30 (batch * S^2 * in_c == 2^30 exactly, and one 16-pixel step below)
    if conv and a.in_c > 0 and a.in_c & (a.in_c - 1) == 0 and a.in_c <= 1 << 20 and a.out_h > 0 and a.out_w > 0:
        e = 30 - (a.in_c.bit_length() - 1)
        S = 1 << (e // 2)
        for s, lab in ((S - 16, "M in_c below 2^30"), (S, "M in_c = 2^30")):
            o = (s + 2 * a.pad - a.k_h) // a.stride + 1 if a.stride > 0 else s
            put(lab, in_h=s, in_w=s, out_h=o, out_w=o, M=(1 + e % 2) * o * o)
    return out


class Rows:
    """The generated list: `problems` [(label, args)], and per row the problem, workspace, hint and debug bit."""

    def __init__(self):
        base = launches()
        self.problems, is_launch = [], []
        for name, a in base:
            self.problems.append((name, a))
            is_launch.append(True)
            for lab, b in perturbations(a):
                self.problems.append((f"{name} / {lab}", b))
                is_launch.append(False)
        # (debug bit, problem, hints): every problem under every hint; the debug bits on the launches under
        # every hint and on the perturbations under DP_TILE_AUTO
        self.blocks = [(0, pi, N_TILES) for pi in range(len(self.problems))]
        for bit in DEBUG_BITS:
            self.blocks += [(bit, pi, N_TILES if is_launch[pi] else 1) for pi in range(len(self.problems))]
        n = 2 * sum(h for _, _, h in self.blocks)
        self.problem, self.ws = np.empty(n, np.int32), np.empty(n, np.int8)
        self.hint, self.dbg = np.empty(n, np.int8), np.empty(n, np.int32)
        r = 0
        for bit, pi, nh in self.blocks:
            for ws in (0, 1):
                self.problem[r:r + nh], self.ws[r:r + nh], self.dbg[r:r + nh] = pi, ws, bit
                self.hint[r:r + nh] = np.arange(nh)
                r += nh

    def digest(self):
        h = hashlib.sha256()
        for _, a in self.problems:
            h.update(bytes(a))
        for arr in (self.problem, self.ws, self.hint, self.dbg):
            h.update(arr.tobytes())
        return h.hexdigest()

    def plan(self, lib):
        """(rc, tile, grid) of every row from `lib`, and the seconds spent in the planning loop."""
        n = len(self.problem)
        rc, tile, grid = np.empty(n, np.int8), np.full(n, -1, np.int8), np.full(n, -1, np.int32)
        ws_bytes = int(lib.dp_gemm_workspace_size())
        t, g = ctypes.c_int32(), ctypes.c_int32()
        tp, gp, fn = ctypes.byref(t), ctypes.byref(g), lib.dp_gemm_plan
        work = [_copy(a) for _, a in self.problems]
        r, cur, spent = 0, None, 0.0
        try:
            for bit, pi, nh in self.blocks:
                if bit != cur:
                    lib.dp_gemm_debug_flags(bit)
                    cur = bit
                a = work[pi]
                ap = ctypes.byref(a)
                t0 = time.perf_counter()
                for ws in (0, 1):
                    a.workspace, a.workspace_bytes = (PTR, ws_bytes) if ws else (None, 0)
                    for h in range(nh):
                        a.tile = h
                        c = fn(ap, tp, gp)
                        rc[r] = RC_CODE[c]
                        if c == 0:
                            tile[r], grid[r] = t.value, g.value
                        r += 1
                spent += time.perf_counter() - t0
        finally:
            lib.dp_gemm_debug_flags(0)
        return rc, tile, grid, spent

    def dump(self, path, ws_bytes):
        """The list as a flat file for tools/gemm_plan_time.cpp: int64 header (problems, struct bytes, blocks,
        workspace bytes), the dp_gemm_args structs, then (debug bit, problem, hints) int32 triples."""
        with open(path, "wb") as fh:
            fh.write(np.array([len(self.problems), ctypes.sizeof(GemmArgs), len(self.blocks), ws_bytes], np.int64).tobytes())
            for _, a in self.problems:
                fh.write(bytes(a))
            fh.write(np.array(self.blocks, np.int32).tobytes())

    def describe(self, r):
        name, a = self.problems[self.problem[r]]
        kind = "conv" if a.a_mode == _lib.DP_A_CONV else "dense"
        return (f"{name} [{kind} M {a.M} N {a.N} K {a.K}], hint {TILE_NAME[int(self.hint[r])]}, "
                f"{'workspace' if self.ws[r] else 'no workspace'}, debug {int(self.dbg[r])}")


def outcome(rc, tile, grid):
    return RC_NAME[rc] if rc else f"{TILE_NAME[int(tile)]} x {int(grid)} workgroups"


def coverage_gaps(rows, rc, tile):
    """What the table does not exercise: (auto results, error codes, hints) that never occur."""
    auto = (rows.hint == 0) & (rc == 0)
    got = {TILE_NAME[int(t)] for t in np.unique(tile[auto])}
    return ([t for t in AUTO_TILES if t not in got],
            [RC_NAME[c] for c in (1, 2, 3, 4) if not (rc == c).any()],
            [TILE_NAME[h] for h in range(1, N_TILES) if not ((rows.hint == h) & (rc == 0)).any()])


def differences(rows, table, rc, tile, grid, limit=20):
    """The first `limit` rows whose outcome differs from the table, in words."""
    bad = np.flatnonzero((table["rc"] != rc) | (table["tile"] != tile) | (table["grid"] != grid))
    lines = [f"{rows.describe(r)}: {outcome(table['rc'][r], table['tile'][r], table['grid'][r])} -> "
             f"{outcome(rc[r], tile[r], grid[r])}" for r in bad[:limit]]
    return len(bad), lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", action="store_true", help="record the built library's answers into the table")
    ap.add_argument("--check", action="store_true", help="compare the built library with the table")
    ap.add_argument("--time", type=int, default=0, metavar="REPS", help="time REPS passes over the list")
    ap.add_argument("--dump", metavar="FILE", help="write the list for tools/gemm_plan_time.cpp (a native timing loop)")
    ap.add_argument("--table", default=TABLE)
    args = ap.parse_args()
    lib = _lib.load()
    rows = Rows()
    rc, tile, grid, _ = rows.plan(lib)
    print(f"{len(rows.problems)} problems, {len(rc)} rows, list {rows.digest()[:16]}, library {_lib.LIB_PATH}")
    gaps = coverage_gaps(rows, rc, tile)
    print(f"not covered: auto results {gaps[0]}, codes {gaps[1]}, hints {gaps[2]}")
    if args.dump:
        rows.dump(args.dump, int(lib.dp_gemm_workspace_size()))
    if args.write:
        if any(gaps):
            sys.exit("the list does not cover the planner: extend the generator")
        np.savez_compressed(args.table, rc=rc, tile=tile, grid=grid, digest=np.array(rows.digest()))
        print(f"wrote {args.table}: {os.path.getsize(args.table)} bytes")
    if args.check:
        table = np.load(args.table)
        if str(table["digest"]) != rows.digest():
            sys.exit("the generated list is not the one the table was recorded for")
        n, lines = differences(rows, table, rc, tile, grid)
        print("\n".join(lines))
        print(f"{n} of {len(rc)} rows differ")
        if n:
            sys.exit(1)
    for _ in range(args.time):
        print(f"pass: {rows.plan(lib)[3]:.4f} s")


if __name__ == "__main__":
    main()
