"""Depth shadows in image space: `find_depth_shadows` and the ground fill of `remove_depth_shadows` of the reference's
`OLD_SCRIPTS/mesh_from_depth.py`, on the GPU (csrc/dp_shadows.hip).

At an object's silhouette a depth map has no true value; the pixels between foreground and background back-project to a
sheet of points behind the object.  `find_depth_shadows` marks them as the reference does: a Sobel gradient (scipy's
arithmetic, bit for bit), normalised by its maximum, thresholded, then the 4-connected free regions of fewer than
`min_region_size` pixels are added to the edge pixels.  Every function queues on the current stream and synchronises
nothing, like `depth_pro.effects`; `stats` stays on the device (fp64, `STATS` names its entries) and
`shadows_summary` is the one read-back.

Stated differences from the reference: its Canny assistance (`image is not None`) is not built;
non-finite depth is defined (counted in `stats`, and such a frame has no edges: every pixel is free); `drop=True`,
which hands `dp_depth_to_points` a depth with the shadow pixels set to NaN, is this project's own use of the mask (the
reference fills the shadow pixels and never drops them); of the fill only the ground-plane interpolation is built, not
RANSAC `detect_ground_plane`, `optimize_ground_plane`, the x-aligned plane's depth search or the cKDTree nearest-valid
fill (reached only by shadow pixels with depth <= 0, counted as `shadow_nonpositive`).
"""

from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import DP_SHADOW_STATS, check

# the entries of `stats`, in the order of DP_SHADOW_STAT_* (include/dp_mi355x.h)
STATS = ("edge", "shadow", "components", "kept", "largest", "gmax", "nonfinite", "error", "shadow_nonpositive")
assert len(STATS) == DP_SHADOW_STATS


def _setup(x: torch.Tensor, dtype: torch.dtype, what: str):
    if x.device.type != "cuda":
        raise _lib.DPError("the depth-shadow stages run on the ROCm device (csrc/dp_shadows.hip)")
    x = x.detach()
    if x.dtype == torch.bool and dtype == torch.uint8:
        x = x.to(torch.uint8)
    if x.dtype != dtype or x.dim() != 2:
        raise ValueError(f"{what} must be {dtype} (H, W), got {x.dtype} {tuple(x.shape)}")
    x = x.contiguous()
    H, W = x.shape
    if H < 1 or W < 1 or H * W >= 2 ** 31:
        raise ValueError(f"{what}: H and W must be >= 1 and H * W < 2^31 (got {(H, W)})")
    lib = _lib.load()
    ws = torch.empty(int(lib.dp_shadows_workspace_size(H, W)), dtype=torch.uint8, device=x.device)
    stats = torch.empty(DP_SHADOW_STATS, dtype=torch.float64, device=x.device)
    return lib, x, H, W, ws, stats, torch.cuda.current_stream(x.device).cuda_stream


def gradient_magnitude(depth: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """dp_depth_gradient: (gradient float32 (H, W), its maximum float32 scalar, stats), all on the device --
    np.sqrt(sobel(d, 1)**2 + sobel(d, 0)**2) with scipy.ndimage.sobel, bit for bit."""
    lib, d, H, W, ws, stats, stream = _setup(depth, torch.float32, "depth")
    g = torch.empty_like(d)
    gmax = torch.empty(1, dtype=torch.float32, device=d.device)
    check(lib.dp_depth_gradient(d.data_ptr(), H, W, g.data_ptr(), gmax.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(),
                                stream), "dp_depth_gradient")
    return g, gmax.reshape(()), stats


def edge_mask(depth: torch.Tensor, threshold_factor: float = 0.2) -> Tuple[torch.Tensor, torch.Tensor]:
    """dp_depth_edges: (edge uint8 (H, W), stats) -- (gmax > 0 ? g / gmax : g) > float32(threshold_factor)."""
    lib, d, H, W, ws, stats, stream = _setup(depth, torch.float32, "depth")
    edge = torch.empty(H, W, dtype=torch.uint8, device=d.device)
    check(lib.dp_depth_edges(d.data_ptr(), H, W, float(threshold_factor), edge.data_ptr(), stats.data_ptr(), ws.data_ptr(),
                             ws.numel(), stream), "dp_depth_edges")
    return edge, stats


def small_region_mask(free: torch.Tensor, min_region_size: int = 100) -> Tuple[torch.Tensor, torch.Tensor]:
    """dp_region_filter: (mask uint8 (H, W), stats) for any free mask (uint8 or bool, non-zero = free) -- 1 where the
    pixel is not free or its 4-connected free component has fewer than min_region_size pixels."""
    lib, f, H, W, ws, stats, stream = _setup(free, torch.uint8, "free")
    mask = torch.empty(H, W, dtype=torch.uint8, device=f.device)
    check(lib.dp_region_filter(f.data_ptr(), H, W, int(min_region_size), mask.data_ptr(), stats.data_ptr(), ws.data_ptr(),
                               ws.numel(), stream), "dp_region_filter")
    return mask, stats


def find_depth_shadows(depth: torch.Tensor, threshold_factor: float = 0.2, min_region_size: int = 100,
                       drop: bool = False) -> Dict[str, torch.Tensor]:
    """dp_depth_shadows, with the reference's name and defaults: {"mask": uint8 (H, W), 1 = shadow; "stats": fp64
    (len(STATS),); with drop=True also "depth": the depth with the shadow pixels set to NaN}, all on the device."""
    lib, d, H, W, ws, stats, stream = _setup(depth, torch.float32, "depth")
    mask = torch.empty(H, W, dtype=torch.uint8, device=d.device)
    dropped = torch.empty_like(d) if drop else None
    check(lib.dp_depth_shadows(d.data_ptr(), H, W, float(threshold_factor), int(min_region_size), mask.data_ptr(),
                               dropped.data_ptr() if drop else None, stats.data_ptr(), ws.data_ptr(), ws.numel(), stream),
          "dp_depth_shadows")
    out = {"mask": mask, "stats": stats}
    if drop:
        out["depth"] = dropped
    return out


def fill_ground_shadows(depth: torch.Tensor, shadow: torch.Tensor, ground_model: dict, ground_rows: float = 0.7,
                        filled: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """dp_fill_ground_shadows: the depth with the shadow pixels of the rows >= int(ground_rows * H) replaced by the
    depth of the plane `ground_model` ({"normal": 3 floats, "d": float}: n . p + d = 0 in the frame the reference's
    formula assumes -- camera axes, y down, unit normal, with its own cx = W / 2, cy = H / 2, f = max(W, H); not
    converted here), rounded to float32; every other pixel copied.  Returns (depth float32 (H, W), filled int64 scalar).
    An x-aligned normal (|n2| <= 1e-6 < |n0|: the reference's 100-step depth search) raises ValueError."""
    normal = [float(c) for c in np.asarray(ground_model["normal"], np.float64).reshape(3)]
    plane = normal + [float(ground_model["d"])]
    if not all(np.isfinite(plane)) or not np.isfinite(float(ground_rows)):
        raise ValueError(f"ground_model and ground_rows must be finite (got {plane}, {ground_rows})")
    if not abs(normal[2]) > 1e-6 and abs(normal[0]) > 1e-6:
        raise ValueError("fill_ground_shadows: an x-aligned ground normal (the reference's depth search) is not built")
    if depth.device.type != "cuda":
        raise _lib.DPError("the depth-shadow stages run on the ROCm device (csrc/dp_shadows.hip)")
    d = depth.detach()
    if d.dtype != torch.float32 or d.dim() != 2:
        raise ValueError(f"depth must be float32 (H, W), got {d.dtype} {tuple(d.shape)}")
    d = d.contiguous()
    H, W = d.shape
    s = shadow.detach()
    s = s.to(torch.uint8) if s.dtype == torch.bool else s
    if s.dtype != torch.uint8 or tuple(s.shape) != (H, W) or s.device != d.device:
        raise ValueError(f"shadow must be uint8 or bool {(H, W)} on the depth's device, got {s.dtype} {tuple(s.shape)}")
    s = s.contiguous()
    out = torch.empty_like(d)
    if filled is None:
        filled = torch.empty(1, dtype=torch.int64, device=d.device)
    check(_lib.load().dp_fill_ground_shadows(d.data_ptr(), s.data_ptr(), H, W, (ctypes.c_double * 4)(*plane), float(ground_rows),
                                             out.data_ptr(), filled.data_ptr(), torch.cuda.current_stream(d.device).cuda_stream),
          "dp_fill_ground_shadows")
    return out, filled.reshape(())


def stats_dict(stats) -> dict:
    """A host `stats` vector as {name: value}: the counts as int, gmax as float."""
    v = np.asarray(stats, np.float64).reshape(-1)
    return {k: (float(v[i]) if k == "gmax" else int(v[i])) for i, k in enumerate(STATS)}


def shadows_summary(result: dict) -> dict:
    """The one read-back of a `find_depth_shadows` result: {"mask": uint8 (H, W) numpy, "stats": {name: value}, and
    "depth" when the result has one}."""
    out = {"mask": result["mask"].cpu().numpy(), "stats": stats_dict(result["stats"].cpu().numpy())}
    if "depth" in result:
        out["depth"] = result["depth"].cpu().numpy()
    return out
