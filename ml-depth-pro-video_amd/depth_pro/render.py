"""Pictures of a point cloud on the GPU (csrc/dp_render.hip): z-buffered square splats from the reference's four view
presets (`render_point_cloud_to_image` of img_to_normalized_pointcloud.py, `visualize_pointcloud` of
pointcloud_cleaner.py: front, top, side, isometric, their 2 x 2 `multi_view` sheet) and the top-down `plan` picture of
pointcloud_pipeline.py's `in_memory_pointcloud_visualization`.

The picture is defined by the rule of DESIGN.md section 22 (restated in tests/render_numpy.py), not by Open3D's
rasteriser: a perspective camera after Open3D's ViewControl, a `point_size` x `point_size` square per point, the nearest
point per pixel with the lower row winning equal depths.  Every function queues on the current stream and synchronises
nothing; `stats` stays on the device (fp64) and `render_summary` is the one read-back.

Stated differences from the reference: the `top` preset's front is [0, 1, 0], not the reference's [0, -1, 0].  With
Open3D's eye = lookat + front * distance the reference's value puts the eye under a cloud whose y points up (every cloud
of the reference and of this project), looking up at the underside of the floor, although its comment says "Looking
down"; here `top` looks down, so the highest point hides the one below it.  The other three presets are the reference's
(its isometric view, front [1, -1, -1], looks from below as the reference's does).  No lighting (it changes nothing for
points without normals); no text labels on the sheet; the plan view has no alpha blending, no random thinning to 50 000
points, it shows every point with the highest on top (the shape overlays and number labels of that picture are
`depth_pro.overlay`); mesh rendering (`visualize_mesh`) is not built.
"""

from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import DP_RENDER_CAMERA_DOUBLES, DP_RENDER_MAX_SIZE, DP_RENDER_MAX_VIEWS, DP_RENDER_STAT_VIEWS, DP_RENDER_STATS, check

# (front, up, zoom): the reference's table, but for the sign of `top`'s front
VIEW_PRESETS = {
    "front": ((0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 0.4),
    "top": ((0.0, 1.0, 0.0), (0.0, 0.0, -1.0), 0.4),         # the eye above the cloud: the reference has [0, -1, 0], see below
    "side": ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.4),
    "isometric": ((1.0, -1.0, -1.0), (0.0, 1.0, 0.0), 0.35),
}
SHEET = ("front", "top", "isometric", "side")       # the multi-view sheet: top-left, top-right, bottom-left, bottom-right
PLAN = "plan"
PLAN_BACKGROUND = (240, 240, 240)                   # the main pipeline's #f0f0f0
TAN_HALF_FOV = math.tan(math.radians(30.0))         # Open3D's 60 degree field of view
GLOBAL_STATS = ("live", "nonfinite", "degenerate", "error")
VIEW_STATS = ("drawn", "clipped", "outside", "covered_pixels")
assert len(GLOBAL_STATS) == DP_RENDER_STAT_VIEWS and DP_RENDER_STAT_VIEWS + len(VIEW_STATS) * (DP_RENDER_MAX_VIEWS + 1) == DP_RENDER_STATS
_RENDER = "point-cloud views run on the ROCm device (csrc/dp_render.hip)"


def _views(views) -> Tuple[list, bool]:
    """(the perspective views as 7 doubles each, is the plan asked for); a view is a preset's name, "plan", or
    (front, up, zoom)."""
    if isinstance(views, str):
        views = (views,)
    rows, plan = [], False
    for v in views:
        if isinstance(v, str):
            if v == PLAN:
                plan = True
                continue
            if v not in VIEW_PRESETS:
                raise ValueError(f"unknown view {v!r}: one of {', '.join(VIEW_PRESETS)}, {PLAN}, or (front, up, zoom)")
            v = VIEW_PRESETS[v]
        front, up, zoom = v
        rows.append([float(c) for c in front] + [float(c) for c in up] + [float(zoom)])
        if len(rows[-1]) != 7:
            raise ValueError("a view is (front (3), up (3), zoom)")
    if not rows and not plan:
        raise ValueError("no view")
    return rows, plan


def _setup(points: torch.Tensor, count, views, size, min_height):
    if points.device.type != "cuda":
        raise _lib.DPError(_RENDER)
    if points.dtype != torch.float64 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points must be an (N, 3) float64 tensor")
    W, H = (int(v) for v in size)
    pts = points.detach().contiguous()
    n = pts.shape[0]
    if n >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 points")
    dev = pts.device
    if n == 0:                                       # an empty cloud still has a picture: one row that is not live
        pts, count = torch.zeros(1, 3, dtype=torch.float64, device=dev), 0
    if count is not None:
        count = (count.detach().to(device=dev, dtype=torch.int32) if torch.is_tensor(count)
                 else torch.tensor([int(count)], dtype=torch.int32, device=dev)).reshape(1)
    rows, plan = _views(views)
    flat = [c for r in rows for c in r]
    varr = (ctypes.c_double * max(len(flat), 1))(*flat)
    plan_mode = 0 if not plan else (1 if min_height is None else 2)
    mh = 0.0 if min_height is None else float(min_height)
    return _lib.load(), pts, count, varr, len(rows), plan_mode, mh, W, H, torch.cuda.current_stream(dev).cuda_stream


def cameras(points: torch.Tensor, views, size: Tuple[int, int], count=None, min_height: Optional[float] = None
            ) -> Tuple[torch.Tensor, torch.Tensor]:
    """dp_render_cameras: the bounds of the live finite rows and the camera record of every view, on the device:
    (cameras fp64 (V, 24), stats fp64 (DP_RENDER_STATS,)) -- the perspective views in the order given, the plan last."""
    lib, pts, cnt, varr, nv, plan, mh, W, H, stream = _setup(points, count, views, size, min_height)
    total = nv + (1 if plan else 0)
    cams = torch.empty(total, DP_RENDER_CAMERA_DOUBLES, dtype=torch.float64, device=pts.device)
    stats = torch.empty(DP_RENDER_STATS, dtype=torch.float64, device=pts.device)
    ws = torch.empty(256, dtype=torch.uint8, device=pts.device)
    check(lib.dp_render_cameras(pts.data_ptr(), None if cnt is None else cnt.data_ptr(), pts.shape[0], varr, nv, plan, mh, W, H,
                                TAN_HALF_FOV, cams.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), stream),
          "dp_render_cameras")
    return cams, stats


def render_views(points: torch.Tensor, colors: Optional[torch.Tensor] = None, views: Sequence = ("front",),
                 size: Tuple[int, int] = (1280, 720), point_size: int = 7, background: Tuple[int, int, int] = (255, 255, 255),
                 count=None, sheet: bool = False, min_height: Optional[float] = None) -> Dict[str, torch.Tensor]:
    """dp_render_points: {"image": uint8 (V, H, W, 3), "cameras": fp64 (V, 24), "stats": fp64 (DP_RENDER_STATS,)}, all on
    the device.  `views`: preset names, (front, up, zoom) tuples (at most 4) and / or "plan" (always the last picture;
    its background is `PLAN_BACKGROUND`, `min_height` shows only the rows with y >= it).  `size` is (W, H);
    `point_size` is odd, 1 .. 15.  sheet=True takes exactly four perspective views and returns one (2H, 2W, 3)
    picture, `SHEET` being the reference's arrangement.  `colors`: uint8 (N, 3) or None (grey)."""
    lib, pts, cnt, varr, nv, plan, mh, W, H, stream = _setup(points, count, views, size, min_height)
    if W < 1 or H < 1 or W * H >= 2 ** 31:
        raise ValueError(f"size: W and H must be >= 1 and W * H < 2^31 (got {(W, H)})")
    ps = int(point_size)
    if not (1 <= ps <= DP_RENDER_MAX_SIZE and ps % 2 == 1):
        raise ValueError(f"point_size must be odd and in [1, {DP_RENDER_MAX_SIZE}] (got {point_size})")
    if nv > DP_RENDER_MAX_VIEWS:
        raise ValueError(f"at most {DP_RENDER_MAX_VIEWS} perspective views in one call (got {nv})")
    if sheet and (nv != DP_RENDER_MAX_VIEWS or plan):
        raise ValueError("sheet=True takes exactly four perspective views and no plan")
    dev, n = pts.device, pts.shape[0]
    cols = None
    if colors is not None and points.shape[0] > 0:
        cols = colors.detach().contiguous()
        if cols.dtype != torch.uint8 or tuple(cols.shape) != (n, 3) or cols.device != dev:
            raise ValueError("colors must be an (N, 3) uint8 tensor on the points' device")
    total = nv + (1 if plan else 0)
    bg = (ctypes.c_uint8 * 6)(*[int(c) for c in background], *PLAN_BACKGROUND)
    image = torch.empty((2 * H, 2 * W, 3) if sheet else (total, H, W, 3), dtype=torch.uint8, device=dev)
    cams = torch.empty(total, DP_RENDER_CAMERA_DOUBLES, dtype=torch.float64, device=dev)
    stats = torch.empty(DP_RENDER_STATS, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.dp_render_workspace_size(W, H, ps, total)), dtype=torch.uint8, device=dev)
    check(lib.dp_render_points(pts.data_ptr(), None if cols is None else cols.data_ptr(), None if cnt is None else cnt.data_ptr(), n,
                               varr, nv, plan, mh, W, H, ps, bg, TAN_HALF_FOV, 1 if sheet else 0, image.data_ptr(), cams.data_ptr(),
                               stats.data_ptr(), ws.data_ptr(), ws.numel(), stream), "dp_render_points")
    return {"image": image, "cameras": cams, "stats": stats}


def stats_dict(stats, n_views: int) -> dict:
    """A host `stats` vector as {name: int}; the per-view entries are lists over the call's views."""
    v = np.asarray(stats, np.float64).reshape(-1)
    out = {k: int(v[i]) for i, k in enumerate(GLOBAL_STATS)}
    for j, k in enumerate(VIEW_STATS):
        out[k] = [int(v[DP_RENDER_STAT_VIEWS + len(VIEW_STATS) * i + j]) for i in range(n_views)]
    return out


def render_summary(result: dict) -> dict:
    """The one read-back of a `render_views` result: {"image": numpy uint8, "cameras": numpy fp64, "stats": {name: int}}."""
    cams = result["cameras"].cpu().numpy()
    return {"image": result["image"].cpu().numpy(), "cameras": cams, "stats": stats_dict(result["stats"].cpu().numpy(), len(cams))}
