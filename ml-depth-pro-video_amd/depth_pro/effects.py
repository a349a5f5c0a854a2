"""Depth-warped views of a frame: the parallax frames and the red-cyan anaglyph of the reference's
`OLD_SCRIPTS/depth_video_effect.py` (its `3D_EFFECTS_README.md`), on the GPU (csrc/dp_effects.hip).

`view_params` is the host side of a parallax frame: the reference's phase `t = 2 pi frame / total_frames` and its
`np.cos` / `np.sin` displacement, in numpy as the reference computes them (the device does no transcendental).
`warp_views` / `parallax_views` make any number of views of one image from one read of its depth; `anaglyph` is the
fused left / right pass.  Every function queues on the current stream and synchronises nothing, like
`depth_pro.pointcloud`; the `bad` counts stay on the device (int64: the pixels written black because their map
coordinate was not finite -- NaN / inf depth, or a constant depth map; see include/dp_mi355x.h, "Depth-warped views").

Stated differences from the reference: the views are not transposed (the reference passes
`map_x.T, map_y.T` to `cv2.remap`), arrays are RGB and are written as RGB (the reference hands RGB to `cv2.imwrite`),
and non-finite depth is defined (finite min / max, black and counted).
"""

from __future__ import annotations

import ctypes
from typing import Iterable, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import DP_WARP_MAX_VIEWS, DP_WARP_SHIFT, DP_WARP_SHIFT_F32, DP_WARP_ZOOM, check

MOTIONS = ("circle", "zoom", "swing")


class View(NamedTuple):
    """One view descriptor of dp_warp_views: {kind, a, b}."""
    kind: int
    a: float
    b: float


def view_params(motion: str, amplitude: float, W: int, H: int, frame: int, total_frames: int) -> View:
    """The descriptor of frame `frame` of a `total_frames` parallax cycle (reference :69-97), computed as the
    reference does: Python / numpy float64, `np.cos` and `np.sin` of `t = 2 * np.pi * frame / total_frames`."""
    t = 2 * np.pi * frame / total_frames
    if motion == "circle":
        return View(DP_WARP_SHIFT, float(amplitude * W * np.cos(t)), float(amplitude * H * np.sin(t)))
    if motion == "zoom":
        zoom_factor = 1.0 + amplitude * np.sin(t)
        return View(DP_WARP_ZOOM, float(1 - zoom_factor), 0.0)
    if motion == "swing":
        return View(DP_WARP_SHIFT, float(amplitude * W * np.sin(t)), 0.0)
    raise ValueError(f"Unknown motion type: {motion}")


def anaglyph_views(separation: float, W: int) -> Tuple[View, View]:
    """The anaglyph's (left, right) views as dp_warp_views descriptors (reference :152-161)."""
    dx = separation * W
    return View(DP_WARP_SHIFT_F32, dx, 0.0), View(DP_WARP_SHIFT_F32, -dx, 0.0)


def _inputs(image: torch.Tensor, depth: torch.Tensor):
    if depth.device.type != "cuda":
        raise _lib.DPError("the depth-warped views run on the ROCm device (csrc/dp_effects.hip)")
    d = depth.detach()
    if d.dtype != torch.float32 or d.dim() != 2:
        raise ValueError(f"depth must be float32 (H, W), got {d.dtype} {tuple(d.shape)}")
    d = d.contiguous()
    H, W = d.shape
    img = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image))
    if img.dtype != torch.uint8 or tuple(img.shape) != (H, W, 3):
        raise ValueError(f"image must be uint8 (H, W, 3) = {(H, W, 3)}, got {img.dtype} {tuple(img.shape)}")
    img = img.to(d.device, non_blocking=True).contiguous()
    lib = _lib.load()
    ws = torch.empty(int(lib.dp_effects_workspace_size()), dtype=torch.uint8, device=d.device)
    return lib, img, d, H, W, ws, torch.cuda.current_stream(d.device).cuda_stream


def warp_views(image: torch.Tensor, depth: torch.Tensor, views: Sequence[Sequence[float]],
               out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """dp_warp_views: `views` ({kind, a, b} each) of `image` (uint8 (H, W, 3); a host array is uploaded) by `depth`
    (float32 (H, W), device).  Returns (uint8 (V, H, W, 3), bad int64 (V,)), both on the device; more than 32 views
    go in several launches (each reads the depth once for its views)."""
    views = [tuple(float(c) for c in v) for v in views]
    if not views or any(len(v) != 3 for v in views):
        raise ValueError("views: a non-empty sequence of (kind, a, b)")
    lib, img, d, H, W, ws, stream = _inputs(image, depth)
    V = len(views)
    if out is None:
        out = torch.empty(V, H, W, 3, dtype=torch.uint8, device=d.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (V, H, W, 3) or not out.is_contiguous() or out.device != d.device:
        raise ValueError(f"out must be a contiguous uint8 {(V, H, W, 3)} tensor on the depth's device")
    bad = torch.empty(V, dtype=torch.int64, device=d.device)
    for v0 in range(0, V, DP_WARP_MAX_VIEWS):
        chunk = views[v0:v0 + DP_WARP_MAX_VIEWS]
        desc = (ctypes.c_double * (3 * len(chunk)))(*[c for v in chunk for c in v])
        check(lib.dp_warp_views(img.data_ptr(), d.data_ptr(), H, W, desc, len(chunk), out[v0].data_ptr(),
                                bad[v0:].data_ptr(), ws.data_ptr(), ws.numel(), stream), "dp_warp_views")
    return out, bad


def parallax_views(image: torch.Tensor, depth: torch.Tensor, motion: str = "circle", amplitude: float = 0.05,
                   total_frames: int = 150, frames: Optional[Iterable[int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The frames `frames` (default: all `total_frames`, the reference's 5 s x 30 fps) of the reference's parallax
    video of one image, as (uint8 (len(frames), H, W, 3), bad int64)."""
    if int(total_frames) < 1:
        raise ValueError(f"total_frames must be >= 1 (got {total_frames})")
    H, W = depth.shape[-2:]
    frames = range(int(total_frames)) if frames is None else list(frames)
    return warp_views(image, depth, [view_params(motion, amplitude, W, H, f, total_frames) for f in frames])


def anaglyph(image: torch.Tensor, depth: torch.Tensor, separation: float = 0.05,
             out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """dp_anaglyph: the reference's red-cyan anaglyph (:113-183) in one pass -- red from the left view, green and
    blue from the right.  Returns (uint8 (H, W, 3), bad int64 scalar), both on the device."""
    lib, img, d, H, W, ws, stream = _inputs(image, depth)
    if out is None:
        out = torch.empty(H, W, 3, dtype=torch.uint8, device=d.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (H, W, 3) or not out.is_contiguous() or out.device != d.device:
        raise ValueError(f"out must be a contiguous uint8 {(H, W, 3)} tensor on the depth's device")
    bad = torch.empty(1, dtype=torch.int64, device=d.device)
    check(lib.dp_anaglyph(img.data_ptr(), d.data_ptr(), H, W, float(separation * W), out.data_ptr(), bad.data_ptr(),
                          ws.data_ptr(), ws.numel(), stream), "dp_anaglyph")
    return out, bad.reshape(())
