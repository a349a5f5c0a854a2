"""Shape overlays on the plan view, on the GPU (csrc/dp_overlay.hip): the last step of pointcloud_pipeline.py's
`in_memory_pointcloud_visualization` (:172-230), which strokes the fitted rectangles and circles on the top-down plan of
the cloud and writes each one's number on it.

The picture is defined by the rule of DESIGN.md section 23 (the numbered list of include/dp_mi355x.h, restated in
tests/overlay_numpy.py), not by matplotlib's rasteriser.  Strokes and labels are drawn from the tables that are on the
device already (`pointcloud.rectangle_list` / `split_l_shapes` rows, the circles of the `fit_shapes` table) with the
camera record of the plan picture they are drawn on; every function queues on the current stream and synchronises
nothing, and `overlay_summary` is the one read-back.

Stated differences from the reference: hard-edged strokes, not anti-aliased ones; 5 x 7 bitmap digits, not a TrueType
face; a plain label box, not a rounded one; the stroke's width is in pixels, not in points; no 'jet' colour bar (the
plan shows the cloud's own colours); no random thinning of the points.
"""

from __future__ import annotations

import ctypes
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import render
from ._lib import DP_OVERLAY_MAX_LABEL_SCALE, DP_OVERLAY_RECORD_DOUBLES, DP_OVERLAY_STATS, DP_RENDER_CAMERA_DOUBLES, check

# the reference's two colour tables (pointcloud_pipeline.py:176-179)
RECT_PALETTE = ("#4285F4", "#34A853", "#FBBC05", "#EA4335", "#8E44AD", "#16A085", "#D35400", "#7F8C8D")
CIRCLE_PALETTE = ("#3498DB", "#2ECC71", "#F1C40F", "#E74C3C", "#9B59B6", "#1ABC9C", "#E67E22", "#95A5A6")
STROKE_ALPHA = 230                                  # the reference's 0.9
STATS = ("rectangles", "circles", "skipped", "offscreen", "labels_dropped", "pixels_painted", "error", "spare")
RECORD_COLUMNS = ("kind", "flags", "x", "y", "a", "b", "cos", "sin", "colour", "number", "stroke_x0", "stroke_y0", "stroke_x1",
                  "stroke_y1", "label_x0", "label_y0", "label_x1", "label_y1", "digits", "spare")
assert len(STATS) == DP_OVERLAY_STATS and len(RECORD_COLUMNS) == DP_OVERLAY_RECORD_DOUBLES
_OVERLAY = "shape overlays run on the ROCm device (csrc/dp_overlay.hip)"


def _rgb(hexes) -> list:
    if len(hexes) != 8:
        raise ValueError("a palette has 8 colours")
    return [int(h[k:k + 2], 16) for h in hexes for k in (1, 3, 5)]


def _list(rows, n, width: int, dev, what: str):
    """(tensor or None, device int32 count or None, capacity) of one of the two lists."""
    if rows is None:
        return None, None, 0
    if not torch.is_tensor(rows) or rows.device != dev:
        raise _lib.DPError(f"{what} must be on the picture's device")
    if rows.dtype != torch.float64 or rows.dim() != 2 or rows.shape[1] != width:
        raise ValueError(f"{what} must be an (R, {width}) float64 tensor")
    rows = rows.detach().contiguous()
    if n is not None:
        n = (n.detach().to(device=dev, dtype=torch.int32) if torch.is_tensor(n) else torch.tensor([int(n)], dtype=torch.int32, device=dev))
        n = n.reshape(-1)[:1].contiguous()
    return rows, n, rows.shape[0]


def draw_shapes(image: torch.Tensor, camera: torch.Tensor, rects: Optional[torch.Tensor] = None, n_rects=None,
                shapes: Optional[torch.Tensor] = None, n_clusters=None, stroke: float = 3.0, alpha: int = STROKE_ALPHA,
                label_scale: int = 2, inplace: bool = False, rect_palette=RECT_PALETTE, circle_palette=CIRCLE_PALETTE
                ) -> Dict[str, torch.Tensor]:
    """dp_overlay_shapes: the rectangles `rects` ((R, 8) fp64 rows of `rectangle_list` / `split_l_shapes`, the first
    `n_rects` of them) and the circles of `shapes` (the (K, 16) fp64 table of `fit_shapes`, rows below `n_clusters` with
    kind 2) stroked and numbered on `image` (uint8 (H, W, 3) on the device), seen through `camera`, the plan record
    (24 fp64, on the device) of the `render_views` call that made the picture.  A count is a device int32, an int, or
    None for every row.  `stroke` is the line's width in pixels, `alpha` its opacity (0..255), `label_scale` the size
    of a font pixel (0: no labels).  Returns {"image": the picture (a copy unless inplace=True), "records": fp64
    (R + K, 20), the first rectangles + circles rows written, "stats": fp64 (8,) in `STATS` order}, on the device."""
    if not torch.is_tensor(image) or image.device.type != "cuda":
        raise _lib.DPError(_OVERLAY)
    if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
        raise ValueError("image must be an (H, W, 3) uint8 tensor")
    dev = image.device
    H, W = int(image.shape[0]), int(image.shape[1])
    if W < 1 or H < 1 or W * H >= 2 ** 31:
        raise ValueError(f"image: W and H must be >= 1 and W * H < 2^31 (got {(W, H)})")
    if not torch.is_tensor(camera) or camera.device != dev or camera.dtype != torch.float64 or camera.numel() != DP_RENDER_CAMERA_DOUBLES:
        raise ValueError(f"camera must be {DP_RENDER_CAMERA_DOUBLES} float64 values on the picture's device")
    if not (np.isfinite(float(stroke)) and float(stroke) > 0):
        raise ValueError(f"stroke must be finite and > 0 (got {stroke})")
    if not 0 <= int(alpha) <= 255:
        raise ValueError(f"alpha must be in [0, 255] (got {alpha})")
    if not 0 <= int(label_scale) <= DP_OVERLAY_MAX_LABEL_SCALE:
        raise ValueError(f"label_scale must be in [0, {DP_OVERLAY_MAX_LABEL_SCALE}] (got {label_scale})")
    if inplace and not image.is_contiguous():
        raise ValueError("inplace=True needs a contiguous image")
    img = image if inplace else image.detach().clone(memory_format=torch.contiguous_format)
    cam = camera.detach().contiguous()
    rects, n_rects, mr = _list(rects, n_rects, 8, dev, "rects")
    shapes, n_clusters, mc = _list(shapes, n_clusters, 16, dev, "shapes")
    lib = _lib.load()
    pal = (ctypes.c_uint8 * 48)(*_rgb(rect_palette), *_rgb(circle_palette))
    records = torch.empty(max(mr + mc, 1), DP_OVERLAY_RECORD_DOUBLES, dtype=torch.float64, device=dev)
    stats = torch.empty(DP_OVERLAY_STATS, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.dp_overlay_workspace_size(mr, mc)), dtype=torch.uint8, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    check(lib.dp_overlay_shapes(img.data_ptr(), W, H, cam.data_ptr(), ptr(rects), ptr(n_rects), mr, ptr(shapes), ptr(n_clusters), mc,
                                pal, float(stroke), int(alpha), int(label_scale), records.data_ptr(), stats.data_ptr(), ws.data_ptr(),
                                ws.numel(), torch.cuda.current_stream(dev).cuda_stream), "dp_overlay_shapes")
    return {"image": img, "records": records[:mr + mc], "stats": stats}


def plan_with_shapes(points: torch.Tensor, colors: Optional[torch.Tensor], count, rects: Optional[torch.Tensor], n_rects,
                     shapes: Optional[torch.Tensor], n_clusters, size: Tuple[int, int] = (1280, 720), point_size: int = 7,
                     min_height: Optional[float] = None, stroke: float = 3.0, alpha: int = STROKE_ALPHA, label_scale: int = 2
                     ) -> Dict[str, torch.Tensor]:
    """The reference's picture: `render.render_views(views="plan")` of the cloud (the rows with y >= `min_height`, the
    highest on top), then `draw_shapes` on it with that call's camera record; nothing leaves the device in between.
    Returns {"image": uint8 (H, W, 3), "camera": fp64 (24,), "records", "stats": the overlay's, "plan_stats": the
    plan's fp64 (DP_RENDER_STATS,)}."""
    plan = render.render_views(points, colors, views=render.PLAN, size=size, point_size=point_size, count=count, min_height=min_height)
    res = draw_shapes(plan["image"][0], plan["cameras"][0], rects, n_rects, shapes, n_clusters, stroke, alpha, label_scale, inplace=True)
    return {**res, "camera": plan["cameras"][0], "plan_stats": plan["stats"]}


def stats_dict(stats) -> dict:
    """A host `stats` vector as {name: int}."""
    v = np.asarray(stats, np.float64).reshape(-1)
    return {k: int(v[i]) for i, k in enumerate(STATS)}


def overlay_summary(result: dict) -> dict:
    """The one read-back of a `draw_shapes` / `plan_with_shapes` result: {"image": numpy uint8, "records": numpy fp64,
    the rows written, "stats": {name: int}} (and "camera", "plan_stats" {name: int} where the result has them)."""
    stats = stats_dict(result["stats"].cpu().numpy())
    n = stats["rectangles"] + stats["circles"] + stats["skipped"] + stats["offscreen"]
    out = {"image": result["image"].cpu().numpy(), "records": result["records"][:n].cpu().numpy(), "stats": stats}
    if "camera" in result:
        out["camera"] = result["camera"].cpu().numpy()
        out["plan_stats"] = render.stats_dict(result["plan_stats"].cpu().numpy(), 1)
    return out
