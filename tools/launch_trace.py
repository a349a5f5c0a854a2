#!/usr/bin/env python3
"""Every libdp_mi355x.so call of ONE eager `Engine.forward()`, one line per call, in a form that
two trees can be compared by: the check for a host-schedule refactor ("the same launches with the
same arguments in the same order on the same streams").

    python tools/launch_trace.py OUT.txt [--no-fov]          (synthetic weights, no graph capture)

A line holds the entry name, every scalar argument, every field of every `GemmArgs` of dp_gemm /
dp_gemm_grouped and the stream as the name of the engine stream it equals.  A device pointer is
written as `name+byte offset` of the engine tensor that contains it (`P[key]`, `vp.x`, `dec[96].c`,
...; the largest one where views overlap), `null`, or `tmp<k>` (k by first appearance within the
call) for memory the engine does not hold.  Precision and ablations come from the environment
(DEPTH_PRO_COMPUTE_DTYPE, DP_ABLATE).  It touches only `Engine`'s public attributes and
`depth_pro._lib`, so one copy runs on any two commits; compare the files with cmp.
"""
import argparse
import bisect
import ctypes
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "ml-depth-pro-video_amd"))


def tensors(obj, path, out, depth=0):
    """(name, tensor) of every tensor reachable from `obj`: dict values, list items, and the
    attributes of the engine module's own objects."""
    if isinstance(obj, torch.Tensor):
        out.append((path, obj))
    elif isinstance(obj, dict):
        for k, v in obj.items():
            tensors(v, f"{path}[{k}]", out, depth + 1)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            tensors(v, f"{path}[{i}]", out, depth + 1)
    elif depth < 3 and type(obj).__module__ == "depth_pro.engine":
        for k, v in vars(obj).items():
            if not k.startswith("_"):
                tensors(v, f"{path}.{k}" if path else k, out, depth + 1)


class Names:
    def __init__(self, eng):
        found = []
        tensors(eng, "", found)
        # the largest tensor first, then by name: a view never hides the buffer it lies in
        spans = sorted(((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), n) for n, t in found
                        if t.is_cuda and t.numel()), key=lambda s: (s[0] - s[1], s[2]))
        self.spans = []
        for lo, hi, n in spans:      # keep the spans that no earlier (larger) one covers
            if not any(a <= lo and hi <= b for a, b, _ in self.spans):
                self.spans.append((lo, hi, n))
        self.spans.sort()
        self.starts = [s[0] for s in self.spans]
        main = torch.cuda.current_stream(eng.dev).cuda_stream
        self.streams = {main: "main"}
        for n in ("side", "dec_a", "dec_b", "dec_c"):
            self.streams.setdefault(getattr(eng, n).cuda_stream, n)

    def ptr(self, p, tmp):
        if not p:
            return "null"
        i = bisect.bisect_right(self.starts, p) - 1     # (the spans left are separate allocations)
        if i >= 0 and p < self.spans[i][1]:
            return f"{self.spans[i][2]}+{p - self.spans[i][0]}"
        return tmp.setdefault(p, f"tmp{len(tmp)}")

    def stream(self, s):
        return "stream=" + self.streams.get(s or 0, "other")


def fmt_args(names, fn, args):
    tmp, out = {}, []
    types = fn.argtypes
    for j, (a, ty) in enumerate(zip(args, types)):
        if ty is ctypes.c_void_p and j == len(args) - 1:
            out.append(names.stream(a))
        elif isinstance(a, ctypes.Array) and a._type_ is ctypes.c_void_p:      # a host table of pointers
            out.append("[" + " ".join(names.ptr(p, tmp) for p in a) + "]")
        elif isinstance(a, ctypes.Array) or hasattr(a, "_obj"):               # GemmArgs: an array / byref(one)
            for g in (a if isinstance(a, ctypes.Array) else [a._obj]):
                fields = []
                for f, fty in g._fields_:
                    v = getattr(g, f)
                    fields.append(f"{f}={names.ptr(v, tmp) if fty is ctypes.c_void_p else repr(v)}")
                out.append("{" + " ".join(fields) + "}")
        elif ty is ctypes.c_void_p:
            out.append(names.ptr(a, tmp))
        else:
            out.append(repr(a))
    return " ".join(out)


class Traced:
    """Stands in for the loaded library: every dp_* call is written down, then made."""

    def __init__(self, lib, names, lines):
        self.__dict__.update(lib=lib, names=names, lines=lines)

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("dp_"):
            return fn

        def call(*args):
            self.lines.append(f"{name} {fmt_args(self.names, fn, args)}")
            return fn(*args)
        return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--no-fov", action="store_true", help="an engine without the FOV encoder (one side ViT)")
    args = ap.parse_args()
    from depth_pro import _lib, ops
    from depth_pro.depth_pro import _compute_dtype
    from depth_pro.engine import Engine, pack_weights
    from depth_pro.weights import synthetic_state_dict

    dev = torch.device("cuda:0")
    code = _compute_dtype(torch.float32)
    eng = Engine(pack_weights(synthetic_state_dict(0), dev, code), dev, code, use_fov=not args.no_fov)
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (1536, 1536, 3), dtype=np.uint8)).to(dev)
    ops.normalize_u8(img, eng.x0)
    lines = []
    lib = _lib.load()
    _lib._lib = Traced(lib, Names(eng), lines)
    try:
        eng.forward()
    finally:
        _lib._lib = lib
    torch.cuda.synchronize()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"{args.out}: {len(lines)} calls")


if __name__ == "__main__":
    main()
