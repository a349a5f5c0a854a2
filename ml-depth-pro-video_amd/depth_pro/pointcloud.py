"""Point-cloud write-out of a depth frame (BASELINE config 5).

Reference: `depth_to_3d` (img_to_normalized_pointcloud.py:819-856) followed by the
Open3D PLY write (`o3d.io.write_point_cloud`, :1318).  The back-projection and the
row-major compaction of the valid pixels run in `dp_depth_to_points` (HIP, fp64 as
numpy computes it); the PLY writer is this package's own (no Open3D): binary
little-endian, `double x y z` + `uchar red green blue`, the vertex layout Open3D writes.

Ground normalisation (the rest of the reference's first 3-D stage, same file): `fit_ground_plane`
(`grid_based_ground_plane_fit`, :601-816), `normalize_to_ground` (`normalize_point_cloud_to_ground`,
:880-981), `ground_adjust` (`grid_based_ground_adjustment`, :983-1118), the `ground.json` helpers
(:225-312) and `apply_rotation_to_plane` (:314-373).  All per-point work and every percentile run
in csrc/dp_ground.hip (segmented radix selection, fp64); the host only sees the <= 32 trace points.
Not built: `optimize_ground_plane` (scipy) and the 50 000-point random pre-sample in front of it.

Cleaning (the reference pipeline's next step, `pointcloud_cleaner.py:142-309`): `remove_stray_points`,
`clean_shadows` and `clean_pointcloud` (one after the other), on the stable device radix sort
`sort_pairs` and an order-preserving compaction -- csrc/dp_clean.hip, no Open3D, no host read-back.

Clustering (the per-point part of the floor-plan step, `simple_pointcloud_viewer.py:332-412`):
`dbscan_labels` (sklearn's DBSCAN labels over (x, z), exactly), `cluster_table`, `cluster_pointcloud`
and the host-side `cluster_summary` -- csrc/dp_cluster.hip, no sklearn, no host read-back.
`fit_shapes` / `cluster_shapes` fit each cluster's convex hull, minimum-area rectangle and circle and take
the reference's circle-or-rectangle decision (csrc/dp_shapes.hip, no scipy, no OpenCV); `shape_summary` and
`export_shape_text` are their host-side writers.

Oriented mesh points (the start of the reference's meshing step, `pointcloud_to_mesh.py:313-395`):
`voxel_downsample`, `knn_search`, `estimate_normals` and `oriented_points` (all three with the reference's
values) -- csrc/dp_normals.hip, no Open3D, no host read-back; `write_ply_normals` / `read_ply_normals` are the
PLY writer and reader for a cloud with normals.

Triangle mesh (the reference's `--mesh_method simple`, `pointcloud_to_mesh.py:397-465`): `knn_exact` (the k nearest
other rows, exactly), `fan_triangles`, `clean_triangles`, `triangulate`, `simple_mesh` and `mean_neighbor_distance`
(the deterministic `get_average_point_distance`) -- csrc/dp_mesh.hip, no Open3D, no host read-back;
`mesh_ply_records_async`, `write_mesh_ply` and `read_mesh_ply` are the PLY writer and reader for a mesh.
Not built: Poisson and ball-pivoting reconstruction, `remove_duplicated_vertices`, `remove_non_manifold_edges`.

Occupancy floor plan (the reference's `cleaned_pointcloud_to_floorplan.py` up to its contour tracing):
`occupancy_grid`, `grid_morphology`, `grid_regions`, `floorplan_image` and `floor_plan` (all four with the
reference's height-threshold values) -- csrc/dp_floorplan.hip, no OpenCV, no host read-back;
`floor_plan_summary` makes the one read-back.

Floor-plan polygons (the rest of that file: `findContours`, `approximate_contour`, `save_floorplan_data`):
`region_outlines`, `simplify_outlines`, `floor_mean_height` and `floor_polygons` on a `floor_plan` result --
csrc/dp_outline.hip, no OpenCV, no shapely, no host read-back; `floor_polygons_summary` makes the one read-back
and `export_floorplan_text` writes the reference's `{base}_floorplan.txt`.

Depth shadows in image space (`find_depth_shadows` and the ground fill of `remove_depth_shadows`,
`OLD_SCRIPTS/mesh_from_depth.py`) live in `depth_pro.shadows` (csrc/dp_shadows.hip): they work on the depth map, ahead
of `dp_depth_to_points`, which drops the pixels they set to NaN.
"""

from __future__ import annotations

import ctypes
import json
import os
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import check


def depth_to_3d(depth_in: torch.Tensor, focallength_px: Union[float, torch.Tensor], width: int, height: int,
                rgb: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Same arguments and point order as the reference `depth_to_3d`, on the GPU.

    depth_in: (height, width) fp32 device tensor (`model.infer(...)["depth"]`);
    focallength_px: a float, or the device scalar `infer` returns (read on the device);
    rgb: optional (height, width, 3) uint8 device tensor -> colours of the valid points.
    Returns (points (N, 3) fp64, valid_mask (height, width) bool, colors (N, 3) uint8 or None).
    Reads the point count back (one synchronisation); `depth_to_points_async` does not.
    """
    xyz, valid, cols, count = depth_to_points_async(depth_in, focallength_px, width, height, rgb)
    n = int(count.item())
    return xyz[:n], valid, (None if cols is None else cols[:n])


def depth_to_points_async(depth_in: torch.Tensor, focallength_px: Union[float, torch.Tensor], width: int,
                          height: int, rgb: Optional[torch.Tensor] = None):
    """`depth_to_3d` without the read-back: (points buffer (H*W, 3) fp64, valid mask, colours buffer
    or None, device int32 point count).  The first `count` rows of the buffers are the result;
    nothing is synchronised, so a frame loop can queue it behind `infer` and read it later."""
    if depth_in.device.type != "cuda":
        raise _lib.DPError("depth_to_3d runs on the ROCm device (dp_depth_to_points)")
    d = depth_in.detach().to(torch.float32).contiguous()
    if tuple(d.shape) != (height, width):
        raise ValueError(f"depth shape {tuple(d.shape)} != (height, width) = {(height, width)}")
    dev = d.device
    rows = torch.empty(height + 1, dtype=torch.int32, device=dev)
    xyz = torch.empty(height * width, 3, dtype=torch.float64, device=dev)
    cols = None
    if rgb is not None:
        rgb = rgb.contiguous()
        if rgb.dtype != torch.uint8 or tuple(rgb.shape) != (height, width, 3):
            raise ValueError("rgb must be uint8 (height, width, 3)")
        cols = torch.empty(height * width, 3, dtype=torch.uint8, device=dev)
    if torch.is_tensor(focallength_px):
        f_dev = focallength_px.detach().to(device=dev, dtype=torch.float32).reshape(1).contiguous()
        use_given, f_host, f_ptr = 0, 0.0, f_dev.data_ptr()
    else:
        f_dev, use_given, f_host, f_ptr = None, 1, float(focallength_px), None
    stream = torch.cuda.current_stream(dev).cuda_stream
    check(_lib.load().dp_depth_to_points(d.data_ptr(), height, width, f_ptr, f_host, use_given,
                                         None if rgb is None else rgb.data_ptr(), rows.data_ptr(), xyz.data_ptr(),
                                         None if cols is None else cols.data_ptr(), stream), "dp_depth_to_points")
    valid = (d == d) & (d > 0)
    return xyz, valid, cols, rows[height]


PLY_RECORD = 27   # bytes per vertex: double x, y, z + uchar red, green, blue


def ply_records_async(xyz: torch.Tensor, cols: torch.Tensor) -> torch.Tensor:
    """The PLY vertex records of `depth_to_points_async`'s buffers, interleaved on the device
    ((H*W, 27) uint8: the 24 bytes of x, y, z then r, g, b -- the layout `write_ply` writes), so
    that the frame loop's writer only writes bytes.  Queued on the current stream, no sync."""
    n = xyz.shape[0]
    rec = torch.empty(n, PLY_RECORD, dtype=torch.uint8, device=xyz.device)
    rec[:, :24].copy_(xyz.view(torch.uint8).view(n, 24))
    rec[:, 24:].copy_(cols.view(n, 3))
    return rec


def _ply_header(n: int, colored: bool) -> bytes:
    props = ["property double x", "property double y", "property double z"]
    if colored:
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    return ("\n".join(["ply", "format binary_little_endian 1.0", f"element vertex {n}", *props, "end_header"])
            + "\n").encode("ascii")


def write_ply_records(path: str, records: np.ndarray) -> str:
    """`write_ply` for vertex records already in file layout ((n, 27) uint8, `ply_records_async`)."""
    rec = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, PLY_RECORD)
    if not path.endswith(".ply"):
        path = path + ".ply"
    with open(path, "wb") as f:
        f.write(_ply_header(rec.shape[0], True))
        f.write(memoryview(rec).cast("B"))
    return path


def write_ply(path: str, points: np.ndarray, colors: Optional[np.ndarray] = None) -> str:
    """Binary little-endian PLY: double x, y, z (+ uchar red, green, blue)."""
    pts = np.ascontiguousarray(np.asarray(points, dtype="<f8").reshape(-1, 3))
    n = pts.shape[0]
    if colors is not None:
        col = np.ascontiguousarray(np.asarray(colors, dtype=np.uint8).reshape(-1, 3))
        if col.shape[0] != n:
            raise ValueError("points and colors differ in length")
        body = np.empty(n, dtype=[("p", "<f8", 3), ("c", "u1", 3)])   # the 27-byte vertex records
        body["p"], body["c"] = pts, col
    else:
        body = pts
    if not path.endswith(".ply"):
        path = path + ".ply"
    with open(path, "wb") as f:
        f.write(_ply_header(n, colors is not None))
        # straight from the array's buffer: no bytes copy of the ~224 MB body (4K frame) made with
        # the GIL held, which serialised the loop's writer threads
        f.write(memoryview(body).cast("B"))
    return path


def read_ply(path: str) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """Reader for the files `write_ply` produces (tests, tools)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    n = int(next(l for l in lines if l.startswith("element vertex")).split()[-1])
    has_c = any("red" in l for l in lines)
    if has_c:
        rec = np.frombuffer(data[end:], dtype=[("p", "<f8", 3), ("c", "u1", 3)], count=n)
        return rec["p"].copy(), rec["c"].copy()
    return np.frombuffer(data[end:], dtype="<f8", count=3 * n).reshape(n, 3).copy(), None


# ---- what every point-cloud stage checks first -----------------------------------------------------

def _count_tensor(count, device):
    """The live count (None, an int or a tensor) as a device int32 tensor of one element, or None."""
    if count is None:
        return None
    if not torch.is_tensor(count):
        count = torch.tensor([int(count)], dtype=torch.int32, device=device)
    return count.detach().to(device=device, dtype=torch.int32).reshape(1)


def _points_args(points: torch.Tensor, count, what: str):
    """(lib, contiguous points, N, device count or None, its pointer or None, stream) of a stage; `what`
    is the stage's error for a host tensor (it names the stage's source file)."""
    if points.device.type != "cuda":
        raise _lib.DPError(what)
    if points.dtype != torch.float64 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("points must be an (N, 3) float64 tensor")
    pts = points.contiguous()
    n = pts.shape[0]
    if n >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 points")
    count = _count_tensor(count, pts.device)
    stream = torch.cuda.current_stream(pts.device).cuda_stream
    return _lib.load(), pts, n, count, (None if count is None else count.data_ptr()), stream


# ---- ground-plane fit, levelling, grid adjustment (csrc/dp_ground.hip) ---------------------------

MAX_GRID = _lib.DP_GROUND_MAX_GRID
_GROUND = "ground normalisation runs on the ROCm device (csrc/dp_ground.hip)"


def _check_grid(grid_size: int) -> int:
    g = int(grid_size)
    if not 1 <= g <= MAX_GRID:
        raise ValueError(f"grid_size must be in [1, {MAX_GRID}] (got {grid_size})")
    return g


def segmented_select(keys: torch.Tensor, seg: torch.Tensor, n_seg: int, *, q: Optional[float] = None,
                     frac: Optional[float] = None, kmin: int = 1, min_count: int = 0, count=None):
    """Order statistic per segment on the device (`dp_seg_select`), asynchronous.

    keys: (n,) float64, seg: (n,) int32 ids in [0, n_seg) or -1; give `q` for np.percentile(q)
    (method "linear") or `frac` for the k-th smallest with k = min(count, max(kmin, int(frac * count))).
    Returns (counts (n_seg,) int32, values (n_seg,) float64; NaN where count <= min_count)."""
    if (q is None) == (frac is None):
        raise ValueError("give exactly one of q and frac")
    if keys.device.type != "cuda":
        raise _lib.DPError("segmented_select runs on the ROCm device (dp_seg_select)")
    keys = keys.contiguous()
    seg = seg.contiguous()
    if keys.dtype != torch.float64 or seg.dtype != torch.int32 or keys.dim() != 1 or seg.shape != keys.shape:
        raise ValueError("keys must be (n,) float64 and seg (n,) int32")
    n, dev = keys.shape[0], keys.device
    lib = _lib.load()
    count = _count_tensor(count, dev)
    counts = torch.empty(n_seg, dtype=torch.int32, device=dev)
    values = torch.empty(n_seg, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.dp_ground_workspace_size(n)), dtype=torch.uint8, device=dev)
    mode, param = (_lib.DP_SEL_PERCENTILE, float(q)) if q is not None else (_lib.DP_SEL_KTH, float(frac))
    check(lib.dp_seg_select(keys.data_ptr(), 1, seg.data_ptr(), None if count is None else count.data_ptr(), n,
                            int(n_seg), mode, param, int(kmin), int(min_count), counts.data_ptr(), values.data_ptr(),
                            ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream), "dp_seg_select")
    return counts, values


def ground_trace(points: torch.Tensor, count=None, grid_size: int = 20):
    """The fit's ground trace on the device (`dp_ground_trace`), then read back (one synchronisation):
    (trace (g, 4) = mean x, y, z + bin count, valid (g,) bool, info = [finite, non-finite, z_min, z_max])."""
    g = _check_grid(grid_size)
    lib, pts, n, count, cptr, stream = _points_args(points, count, _GROUND)
    ws = torch.empty(int(lib.dp_ground_workspace_size(n)), dtype=torch.uint8, device=pts.device)
    blob = torch.empty(g * 4 + 4 + (g + 1) // 2, dtype=torch.float64, device=pts.device)   # trace | info | valid (int32)
    base = blob.data_ptr()
    check(lib.dp_ground_trace(pts.data_ptr(), cptr, n, g, base, base + (g * 4 + 4) * 8, base + g * 32,
                              ws.data_ptr(), ws.numel(), stream), "dp_ground_trace")
    host = blob.cpu().numpy()
    valid = host[g * 4 + 4:].view(np.int32)[:g] != 0
    return host[:g * 4].reshape(g, 4).copy(), valid, host[g * 4:g * 4 + 4].copy()


def _lowest_points(points: torch.Tensor, count=None) -> np.ndarray:
    """The fit's fallback trace (:702-707): the max(10, int(0.05 n)) lowest-y points, in index order."""
    lib, pts, n, count, cptr, stream = _points_args(points, count, _GROUND)
    ws = torch.empty(int(lib.dp_ground_workspace_size(n)), dtype=torch.uint8, device=pts.device)
    cap = min(n, max(10, int(0.05 * n)))
    out = torch.empty(cap, 3, dtype=torch.float64, device=pts.device)
    idx = torch.empty(cap, dtype=torch.int32, device=pts.device)
    info = torch.empty(2, dtype=torch.float64, device=pts.device)
    check(lib.dp_ground_lowest(pts.data_ptr(), cptr, n, out.data_ptr(), idx.data_ptr(), cap, info.data_ptr(),
                               ws.data_ptr(), ws.numel(), stream), "dp_ground_lowest")
    k = min(cap, int(info.cpu()[0].item()))
    order = np.argsort(idx[:k].cpu().numpy(), kind="stable")
    return out[:k].cpu().numpy()[order]


def distance_percentile(points: torch.Tensor, normal, d: float, q: float, count=None) -> torch.Tensor:
    """Device tensor [np.percentile(points . normal + d, q), points below the plane, finite points,
    non-finite points] (`dp_ground_dist_percentile`); asynchronous."""
    lib, pts, n, count, cptr, stream = _points_args(points, count, _GROUND)
    ws = torch.empty(int(lib.dp_ground_workspace_size(n)), dtype=torch.uint8, device=pts.device)
    out = torch.empty(4, dtype=torch.float64, device=pts.device)
    plane = (ctypes.c_double * 4)(float(normal[0]), float(normal[1]), float(normal[2]), float(d))
    check(lib.dp_ground_dist_percentile(pts.data_ptr(), cptr, n, plane, float(q), out.data_ptr(), ws.data_ptr(),
                                        ws.numel(), stream), "dp_ground_dist_percentile")
    return out


def fit_trace_plane(trace: np.ndarray):
    """Host part of the fit on the trace points ((k, 3), numpy only): (unit normal, d) before the push-down.

    Least-squares plane y = a x + c z + d, refitted after dropping the trace points with residual
    > 0.1 until nothing changes -- the deterministic limit of the reference's RANSACRegressor
    (min_samples=10, residual_threshold=0.1, :718-725), which it reaches whenever every trace point
    is an inlier.  Fewer than 10 trace points (RANSAC raises in the reference), fewer than 3 inliers
    or a plane steeper than 20 degrees give the horizontal plane at the trace's median y (:754-764).
    As in the reference, d is the intercept of the un-normalised plane (it is not divided by the
    normal's length)."""
    trace = np.asarray(trace, dtype=np.float64).reshape(-1, 3)
    horizontal = (np.array([0.0, 1.0, 0.0]), -float(np.median(trace[:, 1])))
    if len(trace) < 10:
        return horizontal
    X, y = trace[:, [0, 2]], trace[:, 1]
    keep = np.ones(len(trace), dtype=bool)
    while True:
        if keep.sum() < 3:
            return horizontal
        xm, ym = X[keep].mean(axis=0), y[keep].mean()
        coef = np.linalg.lstsq(X[keep] - xm, y[keep] - ym, rcond=None)[0]
        icpt = ym - xm @ coef
        new = np.abs(y - (X @ coef + icpt)) <= 0.1
        if (new == keep).all():
            break
        keep = new
    normal = np.array([-coef[0], 1.0, -coef[1]])
    normal = normal / np.linalg.norm(normal)
    angle = np.arccos(np.abs(normal[1])) * 180 / np.pi
    if angle > 20:
        return horizontal
    return normal, -float(icpt)


def fit_ground_plane(points: torch.Tensor, count=None, grid_size: int = 20) -> dict:
    """The reference's `grid_based_ground_plane_fit(points, None, grid_size)` (:601-816): a model
    dict with its keys `normal` (unit, y up), `d`, `origin`.

    Device: the z-binned ground trace (or the lowest-5 % fallback when fewer than 10 bins qualify)
    and the 0.1-percentile of the signed distances.  Host: `fit_trace_plane` on <= 32 points, then
    the reference's push-down (d -= percentile + 0.05 when more than 0.1 % of the points lie below).
    Two small read-backs (the trace, about 4 * grid_size + 4 doubles, then 4 doubles), each a
    synchronisation; the fallback reads its selected points back as well.
    Stated differences: the reference's RANSAC is stochastic, this is the deterministic limit it
    reaches when every trace point is an inlier; `optimize_ground_plane` and the reference's random
    50 000-point pre-sample are not built; points with a non-finite coordinate are ignored."""
    trace, valid, info = ground_trace(points, count, grid_size)
    if info[0] == 0:
        raise ValueError("fit_ground_plane: no finite points")
    tr = trace[valid, :3]
    if len(tr) < 10:
        tr = _lowest_points(points, count)
    normal, d = fit_trace_plane(tr)
    if normal[1] < 0:
        normal, d = -normal, -d
    pct, below, total, _ = distance_percentile(points, normal, d, 0.1, count).cpu().tolist()
    if below > 0 and below > 0.001 * total:
        d -= (pct + 0.05)
    return {"normal": normal, "d": float(d), "origin": np.array([0.0, -d / normal[1] if normal[1] != 0 else 0.0, 0.0])}


def ground_rotation(ground_model: dict) -> np.ndarray:
    """The 15 host doubles `dp_ground_normalize` takes: unit normal, d, R (row-major), const, rotate
    flag -- the reference's Rodrigues construction (:908-946), its |n . y| > 0.99 no-rotation branch
    (which also skips `const`) included."""
    normal = np.asarray(ground_model["normal"], dtype=np.float64)
    d = float(ground_model["d"])
    unit = normal / np.linalg.norm(normal)             # point_plane_distances (:872-873)
    to_vec = np.array([0.0, 1.0, 0.0])
    R, const, rotate = np.eye(3), 0.0, 0.0
    if not np.abs(np.dot(normal, to_vec)) > 0.99:
        from_vec = normal / np.linalg.norm(normal)
        axis = np.cross(from_vec, to_vec)
        axis = axis / np.linalg.norm(axis)
        angle = np.arccos(np.clip(np.dot(from_vec, to_vec), -1.0, 1.0))
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
        const = -d / (R @ normal)[1]
        rotate = 1.0
    return np.concatenate([unit, [d], R.reshape(-1), [const, rotate]]).astype(np.float64)


NORMALIZE_STATS = ("finite", "non_finite", "near_ground", "ground_level", "level_taken", "ground_points",
                   "set_to_zero", "limited_to_minus_10cm")
ADJUST_STATS = ("finite", "non_finite", "cells_non_empty", "cells_with_points", "cells_adjusted", "points_adjusted",
                "reserved0", "reserved1")


def normalize_to_ground(points: torch.Tensor, ground_model: dict, count=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`normalize_point_cloud_to_ground` (:880-981) on the device: (levelled (N, 3) float64 tensor,
    stats (8,) float64 device tensor in `NORMALIZE_STATS` order).  Asynchronous; rows past `count`
    are left uninitialised; points with a non-finite coordinate are copied unchanged and counted."""
    lib, pts, n, count, cptr, stream = _points_args(points, count, _GROUND)
    ws = torch.empty(int(lib.dp_ground_workspace_size(n)), dtype=torch.uint8, device=pts.device)
    out = torch.empty_like(pts)
    stats = torch.empty(8, dtype=torch.float64, device=pts.device)
    m = ground_rotation(ground_model)
    model = (ctypes.c_double * 15)(*m.tolist())
    check(lib.dp_ground_normalize(pts.data_ptr(), out.data_ptr(), cptr, n, model, stats.data_ptr(), ws.data_ptr(),
                                  ws.numel(), stream), "dp_ground_normalize")
    return out, stats


def ground_adjust(points: torch.Tensor, grid_size: int = 20, percentile: float = 5, count=None
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """`grid_based_ground_adjustment` (:983-1118) on the device: (adjusted (N, 3) float64 tensor,
    stats (8,) float64 device tensor in `ADJUST_STATS` order).  Asynchronous, as `normalize_to_ground`."""
    g = _check_grid(grid_size)
    if not 0 <= float(percentile) <= 100:
        raise ValueError("percentile must be in [0, 100]")
    lib, pts, n, count, cptr, stream = _points_args(points, count, _GROUND)
    ws = torch.empty(int(lib.dp_ground_workspace_size(n)), dtype=torch.uint8, device=pts.device)
    out = torch.empty_like(pts)
    stats = torch.empty(8, dtype=torch.float64, device=pts.device)
    check(lib.dp_ground_adjust(pts.data_ptr(), out.data_ptr(), cptr, n, g, float(percentile), stats.data_ptr(),
                               ws.data_ptr(), ws.numel(), stream), "dp_ground_adjust")
    return out, stats


# ---- cleaning: stray points, shadow columns (csrc/dp_clean.hip) -----------------------------------

STRAY_STATS = ("finite", "non_finite", "kept", "removed", "error", "reserved0", "reserved1", "reserved2")
SHADOW_STATS = ("finite", "non_finite", "columns_occupied", "columns_tested", "columns_removed", "points_removed",
                "cell_size", "error")


_CLEAN = "point-cloud cleaning runs on the ROCm device (csrc/dp_clean.hip)"


def sort_pairs(keys: torch.Tensor, values: torch.Tensor, count=None, bit_lo: int = 0, bit_hi: int = 64
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Stable ascending radix sort of (key, value) pairs by the key bits [bit_lo, bit_hi)
    (`dp_sort_pairs`), asynchronous.  keys: (n,) int64 / uint64 (sorted as unsigned 64-bit patterns),
    values: (n,) int32 / uint32.  Returns sorted copies; with `count` (int or device int32) only the
    first `count` pairs are sorted and the others come back unchanged."""
    if keys.device.type != "cuda":
        raise _lib.DPError("sort_pairs runs on the ROCm device (dp_sort_pairs)")
    if keys.dtype not in (torch.int64, torch.uint64) or values.dtype not in (torch.int32, torch.uint32) \
            or keys.dim() != 1 or values.shape != keys.shape:
        raise ValueError("keys must be (n,) int64 / uint64 and values (n,) int32 / uint32")
    if not 0 <= int(bit_lo) <= int(bit_hi) <= 64:
        raise ValueError("need 0 <= bit_lo <= bit_hi <= 64")
    k, v = keys.contiguous().clone(), values.contiguous().clone()
    n, dev = k.shape[0], k.device
    if n >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 pairs")
    count = _count_tensor(count, dev)
    lib = _lib.load()
    ws = torch.empty(int(lib.dp_clean_workspace_size(n)), dtype=torch.uint8, device=dev)
    check(lib.dp_sort_pairs(k.data_ptr(), v.data_ptr(), None if count is None else count.data_ptr(), n, int(bit_lo),
                            int(bit_hi), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream),
          "dp_sort_pairs")
    return k, v


def stray_mask(points: torch.Tensor, count=None, nb_points: int = 20, radius: float = 0.1
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """`dp_clean_stray`: (keep (N,) uint8 -- rows past `count` unwritten --, stats (8,) float64 in
    `STRAY_STATS` order), both on the device, asynchronous."""
    if int(nb_points) < 1:
        raise ValueError(f"nb_points must be >= 1 (got {nb_points})")
    if not (np.isfinite(radius) and float(radius) > 0):
        raise ValueError(f"radius must be finite and > 0 (got {radius})")
    lib, pts, n, count, cptr, stream = _points_args(points, count, _CLEAN)
    ws = torch.empty(int(lib.dp_clean_workspace_size(n)), dtype=torch.uint8, device=pts.device)
    keep = torch.empty(n, dtype=torch.uint8, device=pts.device)
    stats = torch.empty(8, dtype=torch.float64, device=pts.device)
    check(lib.dp_clean_stray(pts.data_ptr(), cptr, n, float(radius), int(nb_points), keep.data_ptr(), stats.data_ptr(),
                             ws.data_ptr(), ws.numel(), stream), "dp_clean_stray")
    return keep, stats


def shadow_mask(points: torch.Tensor, count=None, shadow_height_threshold: float = 0.1, max_shadow_angle: float = 75,
                min_points_per_column: int = 3) -> Tuple[torch.Tensor, torch.Tensor]:
    """`dp_clean_shadows`: (keep (N,) uint8, stats (8,) float64 in `SHADOW_STATS` order), on the
    device, asynchronous."""
    if int(min_points_per_column) < 1:
        raise ValueError("min_points_per_column must be >= 1")
    lib, pts, n, count, cptr, stream = _points_args(points, count, _CLEAN)
    ws = torch.empty(int(lib.dp_clean_workspace_size(n)), dtype=torch.uint8, device=pts.device)
    keep = torch.empty(n, dtype=torch.uint8, device=pts.device)
    stats = torch.empty(8, dtype=torch.float64, device=pts.device)
    check(lib.dp_clean_shadows(pts.data_ptr(), cptr, n, float(shadow_height_threshold), float(max_shadow_angle),
                               int(min_points_per_column), keep.data_ptr(), stats.data_ptr(), ws.data_ptr(),
                               ws.numel(), stream), "dp_clean_shadows")
    return keep, stats


def compact_points(points: torch.Tensor, colors: Optional[torch.Tensor], keep: torch.Tensor, count=None):
    """`dp_compact_points`: (points buffer (N, 3), colours buffer or None, device int32 count); the
    first `count` rows are the kept rows in their original order, the rest is uninitialised."""
    lib, pts, n, count, cptr, stream = _points_args(points, count, _CLEAN)
    ws = torch.empty(int(lib.dp_clean_workspace_size(n)), dtype=torch.uint8, device=pts.device)
    keep = keep.contiguous()
    if keep.dtype not in (torch.uint8, torch.bool) or keep.shape != (n,):
        raise ValueError("keep must be an (N,) uint8 / bool tensor")
    cols = None
    if colors is not None:
        cols = colors.contiguous()
        if cols.dtype != torch.uint8 or tuple(cols.shape) != (n, 3):
            raise ValueError("colors must be an (N, 3) uint8 tensor")
    out = torch.empty_like(pts)
    cout = None if cols is None else torch.empty_like(cols)
    n_out = torch.empty(1, dtype=torch.int32, device=pts.device)
    check(lib.dp_compact_points(pts.data_ptr(), None if cols is None else cols.data_ptr(), keep.data_ptr(), cptr, n,
                                out.data_ptr(), None if cout is None else cout.data_ptr(), n_out.data_ptr(),
                                ws.data_ptr(), ws.numel(), stream), "dp_compact_points")
    return out, cout, n_out


def remove_stray_points(points: torch.Tensor, colors: Optional[torch.Tensor] = None, count=None, nb_points: int = 20,
                        radius: float = 0.1):
    """The reference's `remove_stray_points` (pointcloud_cleaner.py:142-207) on the device:
    (points buffer (N, 3), colours buffer or None, device int32 count, stats in `STRAY_STATS` order).
    Asynchronous, no read-back; the first `count` rows are the result.
    A point is kept iff at least `nb_points` finite points (itself included) lie at squared distance
    (dx*dx + dy*dy) + dz*dz < radius*radius -- the strict-`<` restatement of Open3D's radius search
    (Open3D was not at hand to compare with).  Stated differences: points with a non-finite coordinate
    are removed; a cloud spanning more than 2^21 - 2 cells of edge `radius` on an axis raises
    stats["error"] and is returned whole."""
    keep, stats = stray_mask(points, count, nb_points, radius)
    out, cols, n_out = compact_points(points, colors, keep, count)
    return out, cols, n_out, stats


def clean_shadows(points: torch.Tensor, colors: Optional[torch.Tensor] = None, count=None,
                  shadow_height_threshold: float = 0.1, max_shadow_angle: float = 75, min_points_per_column: int = 3):
    """The reference's `clean_shadows` (pointcloud_cleaner.py:209-309) on the device, same return
    convention as `remove_stray_points` (stats in `SHADOW_STATS` order; stats[6] is the cell size the
    device derived from the cloud's density).  Stated differences: a column's points are ordered by
    y with ties in index order (the reference's argsort is unstable above 16 points); points with a
    non-finite coordinate are in no column and kept; 2^31 or more columns raise stats["error"] and
    keep everything."""
    keep, stats = shadow_mask(points, count, shadow_height_threshold, max_shadow_angle, min_points_per_column)
    out, cols, n_out = compact_points(points, colors, keep, count)
    return out, cols, n_out, stats


def clean_pointcloud(points: torch.Tensor, colors: Optional[torch.Tensor] = None, count=None, nb_points: int = 20,
                     radius: float = 0.1, shadow_height_threshold: float = 0.1, max_shadow_angle: float = 75,
                     min_points_per_column: int = 3):
    """`remove_stray_points` then `clean_shadows` (the reference pipeline's step 2); the shadow
    stage's density and cell size come from the cloud after stray removal, as in the reference.
    Returns (points buffer, colours buffer or None, device int32 count, stray stats, shadow stats)."""
    p1, c1, n1, st1 = remove_stray_points(points, colors, count, nb_points, radius)
    p2, c2, n2, st2 = clean_shadows(p1, c1, n1, shadow_height_threshold, max_shadow_angle, min_points_per_column)
    return p2, c2, n2, st1, st2


# ---- clustering: exact DBSCAN labels over (x, z), cluster table (csrc/dp_cluster.hip) --------------

CLUSTER_STATS = ("finite", "non_finite", "participants", "core", "border", "noise", "clusters", "error")
CLUSTER_COLUMNS = ("count", "min_core_row", "x_min", "x_max", "z_min", "z_max", "y_min", "y_max", "sum_x", "sum_y",
                   "sum_z", "reserved")


_CLUSTER = "point-cloud clustering runs on the ROCm device (csrc/dp_cluster.hip)"


def _check_cluster(eps, min_samples, max_points) -> None:
    if not (np.isfinite(float(eps)) and float(eps) > 0):
        raise ValueError(f"eps must be finite and > 0 (got {eps})")
    if int(min_samples) < 1:
        raise ValueError(f"min_samples must be >= 1 (got {min_samples})")
    if int(max_points) < 0:
        raise ValueError(f"max_points must be >= 0 (got {max_points})")


def dbscan_labels(points: torch.Tensor, count=None, eps: float = 0.2, min_samples: int = 5,
                  height_threshold: Optional[float] = None, max_points: int = 0
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """`dp_cluster_dbscan`: the labels sklearn's `DBSCAN(eps, min_samples).fit(points[:, [0, 2]])` gives
    the participants -- the finite rows with y >= `height_threshold` (None / NaN: every height), thinned
    to an even stride of `max_points` rows when there are more (0: all) -- as (labels (N,) int32:
    cluster number, -1 noise, -2 not a participant; rows past `count` unwritten --, device int32 cluster
    count, stats (8,) float64 in `CLUSTER_STATS` order).  On the device, asynchronous, no read-back.
    The returned labels keep the call's workspace alive (it holds the clusters' smallest core rows,
    which `cluster_table` reports)."""
    _check_cluster(eps, min_samples, max_points)
    lib, pts, n, count, cptr, stream = _points_args(points, count, _CLUSTER)
    thr = float("nan") if height_threshold is None else float(height_threshold)
    ws = torch.empty(int(lib.dp_cluster_workspace_size(n)), dtype=torch.uint8, device=pts.device)
    labels = torch.empty(n, dtype=torch.int32, device=pts.device)
    ncl = torch.empty((), dtype=torch.int32, device=pts.device)
    stats = torch.empty(8, dtype=torch.float64, device=pts.device)
    check(lib.dp_cluster_dbscan(pts.data_ptr(), cptr, n, float(eps), int(min_samples), thr, int(max_points),
                                labels.data_ptr(), ncl.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), stream),
          "dp_cluster_dbscan")
    labels._dp_cluster_ws = ws
    return labels, ncl, stats


def cluster_table(points: torch.Tensor, labels: torch.Tensor, n_clusters: torch.Tensor, count=None,
                  max_clusters: int = 4096) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """`dp_cluster_table`: (table (max_clusters, 12) float64 in `CLUSTER_COLUMNS` order, order (N,)
    int32, offsets (max_clusters + 1,) int32), on the device, asynchronous.  With K = min(n_clusters,
    max_clusters), rows c < K of the table and entries c <= K of the offsets are written; cluster c's
    rows are `order[offsets[c]:offsets[c + 1]]`, ascending.  `min_core_row` is known for labels that
    come straight from `dbscan_labels` (for any other labels tensor it is -1)."""
    if int(max_clusters) < 0:
        raise ValueError(f"max_clusters must be >= 0 (got {max_clusters})")
    lib, pts, n, count, cptr, stream = _points_args(points, count, _CLUSTER)
    if labels.device != pts.device or not torch.is_tensor(n_clusters) or n_clusters.device != pts.device:
        raise _lib.DPError("labels and n_clusters must be on the points' device")
    if labels.dtype != torch.int32 or tuple(labels.shape) != (n,) or not labels.is_contiguous():
        raise ValueError("labels must be a contiguous (N,) int32 tensor")
    if n_clusters.dtype != torch.int32 or n_clusters.numel() != 1:
        raise ValueError("n_clusters must be a device int32 scalar")
    need = int(lib.dp_cluster_workspace_size(n))
    ws = getattr(labels, "_dp_cluster_ws", None)
    if ws is None or ws.numel() < need or ws.device != pts.device:
        ws = torch.zeros(need, dtype=torch.uint8, device=pts.device)
    mc = int(max_clusters)
    table = torch.zeros(mc, 12, dtype=torch.float64, device=pts.device)
    order = torch.empty(n, dtype=torch.int32, device=pts.device)
    offsets = torch.zeros(mc + 1, dtype=torch.int32, device=pts.device)
    check(lib.dp_cluster_table(pts.data_ptr(), labels.data_ptr(), cptr, n, n_clusters.data_ptr(), mc,
                               table.data_ptr(), order.data_ptr(), offsets.data_ptr(), ws.data_ptr(), ws.numel(),
                               stream), "dp_cluster_table")
    return table, order, offsets


def cluster_pointcloud(points: torch.Tensor, count=None, eps: float = 0.2, min_samples: int = 5,
                       height_threshold: Optional[float] = 1.3, max_points: int = 100000, max_clusters: int = 4096):
    """`dbscan_labels` then `cluster_table`, with the reference's `fit_shapes_to_clusters` defaults
    (eps 0.2, min_samples 5, y >= 1.3, at most 100 000 points).  Returns (labels, n_clusters, stats,
    table, order, offsets), all on the device, nothing synchronised."""
    labels, ncl, stats = dbscan_labels(points, count, eps, min_samples, height_threshold, max_points)
    table, order, offsets = cluster_table(points, labels, ncl, count, max_clusters)
    return labels, ncl, stats, table, order, offsets


def cluster_summary(table_host, stats_host, params: Optional[dict] = None) -> dict:
    """The `{base}_clusters.json` content from arrays already on the host: `table_host` (K, 12) rows of
    `cluster_table` (K clusters), `stats_host` (8,) in `CLUSTER_STATS` order.  Host only."""
    t = np.asarray(table_host, dtype=np.float64).reshape(-1, 12)
    st = np.asarray(stats_host, dtype=np.float64).reshape(8)
    clusters = []
    for c, r in enumerate(t):
        cnt = int(r[0])
        clusters.append({
            "id": c, "count": cnt, "min_core_row": int(r[1]),
            "bbox": {"x": [float(r[2]), float(r[3])], "z": [float(r[4]), float(r[5])], "y": [float(r[6]), float(r[7])]},
            "centroid": [float(r[8] / cnt), float(r[9] / cnt), float(r[10] / cnt)] if cnt else None,
        })
    out = {"parameters": dict(params or {})}
    out.update({k: int(v) for k, v in zip(CLUSTER_STATS, st)})
    out["clusters_listed"] = len(clusters)
    out["cluster_table"] = clusters
    return out


# ---- cluster shapes: hull, minimum-area rectangle, circle, decision (csrc/dp_shapes.hip) ------------

SHAPE_COLUMNS = ("kind", "count", "rect_cu", "rect_cv", "width", "height", "angle", "area", "xc", "yc", "r", "fit_error",
                 "hull_area", "hull_vertices", "circ", "error")
SHAPE_SKIPPED, SHAPE_RECTANGLE, SHAPE_CIRCLE = 0, 1, 2


def fit_shapes(points: torch.Tensor, order: torch.Tensor, offsets: torch.Tensor, n_clusters: torch.Tensor, count=None,
               max_clusters: int = 4096, circularity_threshold: float = 0.85
               ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """`dp_cluster_shapes` on the `order` / `offsets` / cluster count of `cluster_table` (same
    `max_clusters`): per cluster the convex hull, the minimum-area rectangle, the least-squares circle
    and the reference's circle-or-rectangle decision, in the top-down frame u = -x, v = z.  Returns
    (shapes (max_clusters, 16) float64 in `SHAPE_COLUMNS` order, hull_rows (N,) int32, hull_offsets
    (max_clusters + 1,) int32): with K = min(n_clusters, max_clusters), rows c < K of the table are
    written and cluster c's hull vertices are rows `hull_rows[hull_offsets[c]:hull_offsets[c + 1]]`,
    counter-clockwise from the smallest (u, v).  On the device, asynchronous, no read-back."""
    mc = int(max_clusters)
    if mc < 0:
        raise ValueError(f"max_clusters must be >= 0 (got {max_clusters})")
    if np.isnan(float(circularity_threshold)):
        raise ValueError("circularity_threshold must not be NaN")
    lib, pts, n, count, cptr, stream = _points_args(points, count, _CLUSTER)
    for t in (order, offsets, n_clusters):
        if not torch.is_tensor(t) or t.device != pts.device:
            raise _lib.DPError("order, offsets and n_clusters must be on the points' device")
    if order.dtype != torch.int32 or tuple(order.shape) != (n,) or not order.is_contiguous():
        raise ValueError("order must be a contiguous (N,) int32 tensor")
    if offsets.dtype != torch.int32 or tuple(offsets.shape) != (mc + 1,) or not offsets.is_contiguous():
        raise ValueError("offsets must be a contiguous (max_clusters + 1,) int32 tensor")
    if n_clusters.dtype != torch.int32 or n_clusters.numel() != 1:
        raise ValueError("n_clusters must be a device int32 scalar")
    ws = torch.empty(int(lib.dp_shapes_workspace_size(n, mc)), dtype=torch.uint8, device=pts.device)
    shapes = torch.zeros(mc, 16, dtype=torch.float64, device=pts.device)
    hull_rows = torch.empty(n, dtype=torch.int32, device=pts.device)
    hull_offsets = torch.zeros(mc + 1, dtype=torch.int32, device=pts.device)
    check(lib.dp_cluster_shapes(pts.data_ptr(), cptr, n, order.data_ptr(), offsets.data_ptr(), n_clusters.data_ptr(), mc,
                                float(circularity_threshold), shapes.data_ptr(), hull_rows.data_ptr(),
                                hull_offsets.data_ptr(), ws.data_ptr(), ws.numel(), stream), "dp_cluster_shapes")
    return shapes, hull_rows, hull_offsets


def cluster_shapes(points: torch.Tensor, count=None, eps: float = 0.2, min_samples: int = 5,
                   height_threshold: Optional[float] = 1.3, max_points: int = 100000, max_clusters: int = 4096,
                   circularity_threshold: float = 0.85):
    """`cluster_pointcloud` then `fit_shapes`, with the reference's `fit_shapes_to_clusters` defaults.
    Returns `cluster_pointcloud`'s six tensors followed by (shapes, hull_rows, hull_offsets), all on
    the device, nothing synchronised."""
    labels, ncl, stats, table, order, offsets = cluster_pointcloud(points, count, eps, min_samples, height_threshold,
                                                                   max_points, max_clusters)
    return (labels, ncl, stats, table, order, offsets) + fit_shapes(points, order, offsets, ncl, count, max_clusters,
                                                                    circularity_threshold)


def split_large_rectangle(cu: float, cv: float, width: float, height: float, angle: float):
    """The reference's forced split of a very large rectangle (simple_pointcloud_viewer.py:284-330):
    two halves along the longer side.  Pure arithmetic on one rectangle."""
    a = angle * np.pi / 180.0
    if width > height:
        d = width / 4
        return [(cu - d * np.cos(a), cv - d * np.sin(a), width / 2, height, angle),
                (cu + d * np.cos(a), cv + d * np.sin(a), width / 2, height, angle)]
    d = height / 4
    return [(cu - d * np.sin(a), cv + d * np.cos(a), width, height / 2, angle),
            (cu + d * np.sin(a), cv - d * np.cos(a), width, height / 2, angle)]


# ---- the rectangle list and the L-shape split (csrc/dp_lshape.hip) ----------------------------------

RECT_COLUMNS = ("cu", "cv", "width", "height", "angle", "cluster", "flags", "reserved")
RECT_HALF, RECT_L_PART = 1, 2          # bits of the flags column
LSHAPE_STATUS = ("split", "small", "few_points", "thin", "no_empty_region", "empty_ratio", "one_part", "few_parts",
                 "area_ratio", "capacity")
LSHAPE_INFO = ("status", "points_inside", "grid_width", "grid_height", "empty_cells", "occupied_parts", "parts_listed",
               "error")
LSHAPE_MAX_SIDE = _lib.DP_LSHAPE_MAX_SIDE
_LSHAPE = "the L-shape split runs on the ROCm device (csrc/dp_lshape.hip)"


def rectangle_list(shapes: torch.Tensor, n_clusters: torch.Tensor, max_clusters: int = 4096
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """`dp_shape_rectangles`: the rectangle list the reference's `fit_shapes_to_clusters` builds from the
    (max_clusters, 16) table of `fit_shapes` -- every rectangle row in cluster order, one with width * height >
    100 and more than 1000 members as its two halves (`split_large_rectangle`).  Returns (rects
    (2 * max_clusters, 8) float64 in `RECT_COLUMNS` order, device int32 count).  On the device, asynchronous."""
    mc = int(max_clusters)
    if mc < 0:
        raise ValueError(f"max_clusters must be >= 0 (got {max_clusters})")
    if not torch.is_tensor(shapes) or shapes.device.type != "cuda":
        raise _lib.DPError(_LSHAPE)
    if shapes.dtype != torch.float64 or tuple(shapes.shape) != (mc, 16) or not shapes.is_contiguous():
        raise ValueError("shapes must be a contiguous (max_clusters, 16) float64 tensor")
    if not torch.is_tensor(n_clusters) or n_clusters.device != shapes.device:
        raise _lib.DPError("n_clusters must be on the shapes' device")
    if n_clusters.dtype != torch.int32 or n_clusters.numel() != 1:
        raise ValueError("n_clusters must be a device int32 scalar")
    rects = torch.zeros(2 * mc, 8, dtype=torch.float64, device=shapes.device)
    n_rects = torch.zeros((), dtype=torch.int32, device=shapes.device)
    stream = torch.cuda.current_stream(shapes.device).cuda_stream
    check(_lib.load().dp_shape_rectangles(shapes.data_ptr(), n_clusters.data_ptr(), mc, rects.data_ptr(),
                                          n_rects.data_ptr(), stream), "dp_shape_rectangles")
    return rects, n_rects


def split_l_shapes(points: torch.Tensor, labels: torch.Tensor, rects: torch.Tensor, n_rects: torch.Tensor, count=None,
                   max_out: Optional[int] = None, max_cells: int = 1 << 20
                   ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """`dp_lshape_split`: the reference's `detect_and_split_l_shapes` on a rectangle list (`rectangle_list`, or
    any (R, 8) rows in `RECT_COLUMNS` order with a device int32 count) against the DBSCAN participants of
    `labels` (every row with label >= -1).  Returns (rects_out (max_out, 8) float64, n_out (2,) int32 =
    (rows, error word), info (R, 8) float64 in `LSHAPE_INFO` order, one row per input rectangle).  `max_out`
    defaults to R + 4096 rows; `max_cells` is the capacity of all the rectangles' 0.2 m grids together.
    On the device, asynchronous, no read-back."""
    lib, pts, n, count, cptr, stream = _points_args(points, count, _LSHAPE)
    for t in (labels, rects, n_rects):
        if not torch.is_tensor(t) or t.device != pts.device:
            raise _lib.DPError("labels, rects and n_rects must be on the points' device")
    if labels.dtype != torch.int32 or tuple(labels.shape) != (n,) or not labels.is_contiguous():
        raise ValueError("labels must be a contiguous (N,) int32 tensor")
    if rects.dtype != torch.float64 or rects.dim() != 2 or rects.shape[1] != 8 or not rects.is_contiguous():
        raise ValueError("rects must be a contiguous (R, 8) float64 tensor")
    if n_rects.dtype != torch.int32 or n_rects.numel() != 1:
        raise ValueError("n_rects must be a device int32 scalar")
    mr = rects.shape[0]
    mo = mr + 4096 if max_out is None else int(max_out)
    mcells = int(max_cells)
    if mo < 0 or mcells < 0 or mcells >= 2 ** 31 or mo >= 2 ** 27:
        raise ValueError(f"max_out and max_cells must be >= 0 and in range (got {max_out}, {max_cells})")
    ws = torch.empty(int(lib.dp_lshape_workspace_size(mr, mcells)), dtype=torch.uint8, device=pts.device)
    out = torch.zeros(mo, 8, dtype=torch.float64, device=pts.device)
    n_out = torch.zeros(2, dtype=torch.int32, device=pts.device)
    info = torch.zeros(mr, 8, dtype=torch.float64, device=pts.device)
    check(lib.dp_lshape_split(pts.data_ptr(), labels.data_ptr(), cptr, n, rects.data_ptr(), n_rects.data_ptr(), mr, mo,
                              mcells, out.data_ptr(), n_out.data_ptr(), info.data_ptr(), ws.data_ptr(), ws.numel(), stream),
          "dp_lshape_split")
    return out, n_out, info


def shape_summary(shapes_host, params: Optional[dict] = None, rects_host=None, info_host=None) -> dict:
    """The `{base}_shapes.json` content from the (K, 16) rows of `fit_shapes` already on the host:
    parameters, counts, and the `rectangles` and `circles` lists in cluster order, as the reference's
    `fit_shapes_to_clusters` builds them -- a rectangle with width * height > 100 and more than 1000
    members is split in two (`split_large_rectangle`), each half marked `"split": true`.
    With `rects_host` (the written rows of `split_l_shapes`' output) and `info_host` (its info rows, one per
    input rectangle) the rectangles are listed from `rects_host` instead -- the reference's list after
    `detect_and_split_l_shapes` -- each with `"l_part"`, and the summary gains `"l_split": true` and an
    `"l_shapes"` block: per input rectangle the status name and the `LSHAPE_INFO` columns.  Without them
    `detect_and_split_l_shapes` is not applied.  Host only."""
    t = np.asarray(shapes_host, dtype=np.float64).reshape(-1, 16)
    if (rects_host is None) != (info_host is None):
        raise ValueError("rects_host and info_host go together")
    if rects_host is not None:
        return _shape_summary_split(t, params, np.asarray(rects_host, dtype=np.float64).reshape(-1, 8),
                                    np.asarray(info_host, dtype=np.float64).reshape(-1, 8))
    rects, circles = [], []
    skipped = errors = 0
    for c, r in enumerate(t):
        kind, cnt = int(r[0]), int(r[1])
        errors += int(r[15] != 0)
        if kind == SHAPE_CIRCLE:
            circles.append({"cluster": c, "count": cnt, "center": [float(r[8]), float(r[9])], "radius": float(r[10]),
                            "fit_error": float(r[11]), "circularity": float(r[14])})
        elif kind == SHAPE_RECTANGLE:
            parts = [(float(r[2]), float(r[3]), float(r[4]), float(r[5]), float(r[6]))]
            split = bool(r[4] * r[5] > 100 and cnt > 1000)
            if split:
                parts = [tuple(float(v) for v in q) for q in split_large_rectangle(*parts[0])]
            for q in parts:
                rects.append({"cluster": c, "count": cnt, "center": [q[0], q[1]], "width": q[2], "height": q[3],
                              "angle": q[4], "split": split, "hull_area": float(r[12]), "hull_vertices": int(r[13]),
                              "circularity": float(r[14])})
        else:
            skipped += 1
    return {"parameters": dict(params or {}), "clusters_listed": len(t), "skipped": skipped, "errors": errors,
            "rectangles": rects, "circles": circles}


def _shape_summary_split(t, params, rows, info) -> dict:
    """`shape_summary` with the rectangle list of `split_l_shapes`."""
    base = shape_summary(t, params)
    rects = []
    for q in rows:
        c, flags = int(q[5]), int(q[6])
        r = t[c] if 0 <= c < len(t) else np.zeros(16)
        rects.append({"cluster": c, "count": int(r[1]), "center": [float(q[0]), float(q[1])], "width": float(q[2]),
                      "height": float(q[3]), "angle": float(q[4]), "split": bool(flags & RECT_HALF),
                      "l_part": bool(flags & RECT_L_PART), "hull_area": float(r[12]), "hull_vertices": int(r[13]),
                      "circularity": float(r[14])})
    base["rectangles"] = rects
    base["l_split"] = True
    base["l_shapes"] = [dict({"status_name": LSHAPE_STATUS[int(i[0])] if 0 <= int(i[0]) < len(LSHAPE_STATUS) else "unknown"},
                             **{k: int(v) for k, v in zip(LSHAPE_INFO, i)}) for i in info]
    return base


def export_shape_text(summary: dict, path: str) -> None:
    """Write the reference's `export_shape_data` text (simple_pointcloud_viewer.py:414-453), line for
    line, from a `shape_summary`."""
    rects, circles = summary["rectangles"], summary["circles"]
    with open(path, "w") as f:
        f.write("# Floor Plan Shape Data\n")
        f.write("# Units: meters\n\n")
        f.write(f"Total Shapes: {len(rects) + len(circles)}\n")
        f.write(f"Rectangles: {len(rects)}\n")
        f.write(f"Circles: {len(circles)}\n\n")
        total = sum(r["width"] * r["height"] for r in rects) + sum(np.pi * c["radius"] ** 2 for c in circles)
        f.write(f"Total Area: {total:.2f} square meters\n\n")
        f.write("# Rectangles\n")
        f.write("# Format: ID, center_x, center_y, width, height, angle_degrees, area_m2\n")
        for i, r in enumerate(rects):
            f.write(f"{i + 1}, {r['center'][0]:.3f}, {r['center'][1]:.3f}, {r['width']:.3f}, {r['height']:.3f}, "
                    f"{r['angle']:.1f}, {r['width'] * r['height']:.3f}\n")
        f.write("\n# Circles\n")
        f.write("# Format: ID, center_x, center_y, radius, area_m2\n")
        for i, c in enumerate(circles):
            f.write(f"{len(rects) + i + 1}, {c['center'][0]:.3f}, {c['center'][1]:.3f}, {c['radius']:.3f}, "
                    f"{np.pi * c['radius'] ** 2:.3f}\n")


# ---- oriented mesh points: voxel grid, hybrid search, normals (csrc/dp_normals.hip) -----------------

VOXEL_STATS = ("finite", "non_finite", "voxels", "reserved0", "reserved1", "error", "reserved2", "reserved3")
KNN_STATS = ("finite", "non_finite", "few_neighbors", "truncated", "reserved0", "error", "reserved1", "reserved2")
NORMAL_STATS = ("finite", "non_finite", "few_neighbors", "truncated", "flipped", "error", "reserved0", "reserved1")
MAX_NN = 64

_NORMALS = "oriented mesh points run on the ROCm device (csrc/dp_normals.hip)"


def _check_search(radius, max_nn) -> None:
    if not (np.isfinite(float(radius)) and float(radius) > 0):
        raise ValueError(f"radius must be finite and > 0 (got {radius})")
    if not 1 <= int(max_nn) <= MAX_NN:
        raise ValueError(f"max_nn must be in [1, {MAX_NN}] (got {max_nn})")


def voxel_downsample(points: torch.Tensor, colors: Optional[torch.Tensor] = None, count=None, voxel_size: float = 0.05):
    """Open3D's `voxel_down_sample(voxel_size)` on the device (`dp_voxel_downsample`): (points buffer (N, 3),
    colours buffer or None, members per voxel (N,) int32, voxel of every input row (N,) int32 -- -1 for a
    non-finite row --, device int32 voxel count, stats (8,) float64 in `VOXEL_STATS` order).  The first
    `count` rows of the first three are the voxels, in ascending order of their packed grid index (Open3D's
    order is a hash map's); a voxel's point is the mean of its members, its colour the mean rounded half up.
    Asynchronous, no read-back.  A cloud spanning more than 2^21 - 2 voxels on an axis raises
    stats["error"] and gives no voxels."""
    if not (np.isfinite(float(voxel_size)) and float(voxel_size) > 0):
        raise ValueError(f"voxel_size must be finite and > 0 (got {voxel_size})")
    lib, pts, n, count, cptr, stream = _points_args(points, count, _NORMALS)
    cols = None
    if colors is not None:
        cols = colors.contiguous()
        if cols.dtype != torch.uint8 or tuple(cols.shape) != (n, 3):
            raise ValueError("colors must be an (N, 3) uint8 tensor")
    dev = pts.device
    ws = torch.empty(int(lib.dp_normals_workspace_size(n)), dtype=torch.uint8, device=dev)
    out = torch.empty_like(pts)
    cout = None if cols is None else torch.empty_like(cols)
    members = torch.empty(n, dtype=torch.int32, device=dev)
    voxel_of = torch.empty(n, dtype=torch.int32, device=dev)
    n_out = torch.empty(1, dtype=torch.int32, device=dev)
    stats = torch.empty(8, dtype=torch.float64, device=dev)
    check(lib.dp_voxel_downsample(pts.data_ptr(), None if cols is None else cols.data_ptr(), cptr, n, float(voxel_size),
                                  out.data_ptr(), None if cout is None else cout.data_ptr(), members.data_ptr(),
                                  voxel_of.data_ptr(), n_out.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), stream),
          "dp_voxel_downsample")
    return out, cout, members, voxel_of, n_out, stats


def knn_search(points: torch.Tensor, count=None, radius: float = 0.1, max_nn: int = 30):
    """Open3D's `KDTreeSearchParamHybrid(radius, max_nn)` for every row at once (`dp_knn_search`): (neighbours
    (N, max_nn) int32 -- row numbers in ascending (squared distance, row) order, the row itself first, padded
    with -1 --, their number (N,) int32, stats (8,) float64 in `KNN_STATS` order).  A neighbour lies at squared
    distance (dx*dx + dy*dy) + dz*dz < radius*radius, as in `remove_stray_points`; non-finite rows have none.
    Asynchronous, no read-back; rows past `count` are not written.  A cloud spanning more than 2^21 - 2 cells
    of edge `radius` on an axis raises stats["error"] and every count is 0."""
    _check_search(radius, max_nn)
    lib, pts, n, count, cptr, stream = _points_args(points, count, _NORMALS)
    dev = pts.device
    ws = torch.empty(int(lib.dp_normals_workspace_size(n)), dtype=torch.uint8, device=dev)
    nbr = torch.empty(n, int(max_nn), dtype=torch.int32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    stats = torch.empty(8, dtype=torch.float64, device=dev)
    check(lib.dp_knn_search(pts.data_ptr(), cptr, n, float(radius), int(max_nn), nbr.data_ptr(), cnt.data_ptr(),
                            stats.data_ptr(), ws.data_ptr(), ws.numel(), stream), "dp_knn_search")
    return nbr, cnt, stats


def normals_from_neighbors(points: torch.Tensor, nbr: torch.Tensor, nbr_count: torch.Tensor, count=None,
                           camera_location=(0, 0, 0), orient: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """`dp_estimate_normals` on the lists of a `knn_search` over the same points: (normals (N, 3) float64, stats
    (8,) float64 -- finite, non-finite, rows with fewer than 3 neighbours, 0, flipped, 0, 0, 0)."""
    lib, pts, n, count, cptr, stream = _points_args(points, count, _NORMALS)
    if nbr.device != pts.device or nbr_count.device != pts.device:
        raise _lib.DPError("nbr and nbr_count must be on the points' device")
    if nbr.dtype != torch.int32 or nbr.dim() != 2 or nbr.shape[0] != n or not nbr.is_contiguous() or \
            not 1 <= nbr.shape[1] <= MAX_NN:
        raise ValueError(f"nbr must be a contiguous (N, max_nn <= {MAX_NN}) int32 tensor")
    if nbr_count.dtype != torch.int32 or tuple(nbr_count.shape) != (n,) or not nbr_count.is_contiguous():
        raise ValueError("nbr_count must be a contiguous (N,) int32 tensor")
    cam = [float(v) for v in camera_location]
    if len(cam) != 3 or not all(np.isfinite(cam)):
        raise ValueError("camera_location must be three finite numbers")
    normals = torch.empty_like(pts)
    stats = torch.empty(8, dtype=torch.float64, device=pts.device)
    check(lib.dp_estimate_normals(pts.data_ptr(), cptr, n, nbr.data_ptr(), nbr_count.data_ptr(), int(nbr.shape[1]),
                                  (ctypes.c_double * 3)(*cam), int(bool(orient)), normals.data_ptr(), stats.data_ptr(),
                                  stream), "dp_estimate_normals")
    return normals, stats


def estimate_normals(points: torch.Tensor, count=None, radius: float = 0.1, max_nn: int = 30, camera_location=(0, 0, 0),
                     orient: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """Open3D's `estimate_normals(KDTreeSearchParamHybrid(radius, max_nn))` and, with `orient`,
    `orient_normals_towards_camera_location(camera_location)` on the device: `knn_search`, then per row the unit
    eigenvector of the smallest eigenvalue of its neighbours' centred covariance (two passes, fp64), negated where
    it points away from the camera.  Fewer than 3 neighbours give (0, 0, 1) (oriented like any other), a
    non-finite row (0, 0, 0).  Returns (normals (N, 3) float64, stats (8,) float64 in `NORMAL_STATS` order: the
    search's `truncated` and `error` beside the normals' own counts).  Asynchronous, no read-back.
    Stated difference: Open3D uses the one-pass uncentred moments and a closed-form solver."""
    nbr, cnt, kst = knn_search(points, count, radius, max_nn)
    normals, stats = normals_from_neighbors(points, nbr, cnt, count, camera_location, orient)
    stats[3] = kst[3]
    stats[5] = kst[5]
    return normals, stats


def oriented_points(points: torch.Tensor, colors: Optional[torch.Tensor] = None, count=None, voxel_size: float = 0.05,
                    max_nn: int = 30, camera_location=(0, 0, 0)):
    """What every meshing method of the reference's `create_mesh_from_pointcloud` (pointcloud_to_mesh.py:313-395)
    starts from: `voxel_downsample(voxel_size)`, then `estimate_normals` with radius = 2 * voxel_size and `max_nn`
    (the reference's values), oriented towards `camera_location`.  Returns (points buffer, colours buffer or
    None, device int32 count, normals buffer, voxel stats, normal stats); the first `count` rows are the
    oriented point set.  (The reference's first `estimate_normals`, on the full cloud, is overwritten by this
    one and is not computed.)  On the device, nothing synchronised."""
    out, cout, _, _, n_out, vst = voxel_downsample(points, colors, count, voxel_size)
    normals, nst = estimate_normals(out, n_out, 2.0 * float(voxel_size), max_nn, camera_location, True)
    return out, cout, n_out, normals, vst, nst


PLY_NORMALS_RECORD = 51   # bytes per vertex: double x, y, z, nx, ny, nz + uchar red, green, blue


def _ply_normals_header(n: int, colored: bool) -> bytes:
    props = [f"property double {k}" for k in ("x", "y", "z", "nx", "ny", "nz")]
    if colored:
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    return ("\n".join(["ply", "format binary_little_endian 1.0", f"element vertex {n}", *props, "end_header"])
            + "\n").encode("ascii")


def write_ply_normals(path: str, points: np.ndarray, normals: np.ndarray, colors: Optional[np.ndarray] = None) -> str:
    """Binary little-endian PLY: double x, y, z, nx, ny, nz (+ uchar red, green, blue) -- the vertex layout
    Open3D writes for a cloud with normals."""
    pts = np.asarray(points, dtype="<f8").reshape(-1, 3)
    nrm = np.asarray(normals, dtype="<f8").reshape(-1, 3)
    n = pts.shape[0]
    if nrm.shape[0] != n:
        raise ValueError("points and normals differ in length")
    if colors is not None:
        col = np.asarray(colors, dtype=np.uint8).reshape(-1, 3)
        if col.shape[0] != n:
            raise ValueError("points and colors differ in length")
        body = np.empty(n, dtype=[("p", "<f8", 3), ("n", "<f8", 3), ("c", "u1", 3)])
        body["c"] = col
    else:
        body = np.empty(n, dtype=[("p", "<f8", 3), ("n", "<f8", 3)])
    body["p"], body["n"] = pts, nrm
    if not path.endswith(".ply"):
        path = path + ".ply"
    with open(path, "wb") as f:
        f.write(_ply_normals_header(n, colors is not None))
        f.write(memoryview(body.view(np.uint8)))
    return path


def ply_normals_records_async(xyz: torch.Tensor, normals: torch.Tensor, cols: Optional[torch.Tensor]) -> torch.Tensor:
    """The vertex records `write_ply_normals` writes, interleaved on the device ((N, 51) uint8, or (N, 48) without
    colours), queued on the current stream, no sync -- `ply_records_async` for a cloud with normals."""
    n = xyz.shape[0]
    width = PLY_NORMALS_RECORD if cols is not None else PLY_NORMALS_RECORD - 3
    rec = torch.empty(n, width, dtype=torch.uint8, device=xyz.device)
    rec[:, :24].copy_(xyz.contiguous().view(torch.uint8).view(n, 24))
    rec[:, 24:48].copy_(normals.contiguous().view(torch.uint8).view(n, 24))
    if cols is not None:
        rec[:, 48:].copy_(cols.view(n, 3))
    return rec


def write_ply_normals_records(path: str, records: np.ndarray) -> str:
    """`write_ply_normals` for vertex records already in file layout (`ply_normals_records_async`)."""
    rec = np.ascontiguousarray(records, dtype=np.uint8)
    if rec.ndim != 2 or rec.shape[1] not in (PLY_NORMALS_RECORD, PLY_NORMALS_RECORD - 3):
        raise ValueError(f"records must be (n, {PLY_NORMALS_RECORD}) or (n, {PLY_NORMALS_RECORD - 3}) uint8")
    if not path.endswith(".ply"):
        path = path + ".ply"
    with open(path, "wb") as f:
        f.write(_ply_normals_header(rec.shape[0], rec.shape[1] == PLY_NORMALS_RECORD))
        f.write(memoryview(rec.reshape(-1)))            # flat first: a frame may leave no points
    return path


def read_ply_normals(path: str) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
    """Reader for the files `write_ply_normals` produces: (points, normals, colours or None).  (`read_ply` keeps
    reading the files without normals; it is not extended, so nothing changes for them.)"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    n = int(next(l for l in lines if l.startswith("element vertex")).split()[-1])
    if not any(l == "property double nx" for l in lines):
        raise ValueError(f"{path} has no normals")
    dt = [("p", "<f8", 3), ("n", "<f8", 3)] + ([("c", "u1", 3)] if any("red" in l for l in lines) else [])
    rec = np.frombuffer(data[end:], dtype=dt, count=n)
    return rec["p"].copy(), rec["n"].copy(), (rec["c"].copy() if len(dt) == 3 else None)


# ---- triangle mesh: exact k nearest, fan, triangle clean-up (csrc/dp_mesh.hip) -----------------------

KNN_EXACT_STATS = ("finite", "non_finite", "few_neighbors", "max_ring", "error", "reserved0", "reserved1", "reserved2")
TRIANGLE_STATS = ("input", "invalid", "degenerate", "duplicated", "kept", "error", "reserved0", "reserved1")
MAX_K = 64

_MESH = "the triangle mesh runs on the ROCm device (csrc/dp_mesh.hip)"


def _check_knn(k, cell_edge) -> None:
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f"k must be in [1, {MAX_K}] (got {k})")
    if not (np.isfinite(float(cell_edge)) and float(cell_edge) > 0):
        raise ValueError(f"cell_edge must be finite and > 0 (got {cell_edge})")


def knn_exact(points: torch.Tensor, count=None, k: int = 6, cell_edge: float = 0.1):
    """The k nearest other rows of every row (`dp_knn_exact`), what Open3D's `search_knn_vector_3d(p, k + 1)[1:]` lists:
    (neighbours (N, k) int32 in ascending (squared distance, row) order, padded with -1; their number (N,) int32 --
    min(k, finite rows - 1), 0 for a non-finite row; their squared distances (N, k) float64, (dx*dx + dy*dy) + dz*dz;
    stats (8,) float64 in `KNN_EXACT_STATS` order).  `cell_edge` is the search grid's cell size, a speed parameter that
    never changes the result.  Asynchronous, no read-back; rows past `count` are not written.  A cloud spanning more
    than 2^21 - 2 cells on an axis raises stats["error"] and every count is 0.  Stated difference: the query is
    excluded by identity, not as the list's first entry, so an exact duplicate of it is listed."""
    _check_knn(k, cell_edge)
    lib, pts, n, count, cptr, stream = _points_args(points, count, _MESH)
    dev = pts.device
    ws = torch.empty(int(lib.dp_mesh_workspace_size(n, 0)), dtype=torch.uint8, device=dev)
    nbr = torch.empty(n, int(k), dtype=torch.int32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    d2 = torch.empty(n, int(k), dtype=torch.float64, device=dev)
    stats = torch.empty(8, dtype=torch.float64, device=dev)
    check(lib.dp_knn_exact(pts.data_ptr(), cptr, n, int(k), float(cell_edge), nbr.data_ptr(), cnt.data_ptr(), d2.data_ptr(),
                           stats.data_ptr(), ws.data_ptr(), ws.numel(), stream), "dp_knn_exact")
    return nbr, cnt, d2, stats


def _lists_args(nbr: torch.Tensor, nbr_count: torch.Tensor, count):
    """(lib, N, k, device count pointer or None, stream, the count tensor) of a call on the lists of `knn_exact`."""
    if nbr.device.type != "cuda":
        raise _lib.DPError(_MESH)
    if nbr_count.device != nbr.device:
        raise _lib.DPError("nbr and nbr_count must be on one device")
    if nbr.dim() != 2 or not nbr.is_contiguous() or not 1 <= nbr.shape[1] <= MAX_K:
        raise ValueError(f"the lists must be a contiguous (N, k <= {MAX_K}) tensor")
    if nbr_count.dtype != torch.int32 or tuple(nbr_count.shape) != (nbr.shape[0],) or not nbr_count.is_contiguous():
        raise ValueError("nbr_count must be a contiguous (N,) int32 tensor")
    count = _count_tensor(count, nbr.device)
    return (_lib.load(), nbr.shape[0], nbr.shape[1], None if count is None else count.data_ptr(),
            torch.cuda.current_stream(nbr.device).cuda_stream, count)


def fan_triangles(nbr: torch.Tensor, nbr_count: torch.Tensor, count=None) -> torch.Tensor:
    """The reference's triangle loop (pointcloud_to_mesh.py:448-457) over the lists of `knn_exact` (`dp_mesh_fan`):
    row i with m listed neighbours gives (i, nbr[i, j], nbr[i, j + 1]) for j < m - 1 at slot i * (k - 1) + j of the
    (N * (k - 1), 3) int32 result; a live row's other slots are (-1, -1, -1), which `clean_triangles` drops.
    Asynchronous; the slots of rows past `count` are not written."""
    if nbr.dtype != torch.int32:
        raise ValueError("nbr must be int32")
    lib, n, k, cptr, stream, _ = _lists_args(nbr, nbr_count, count)
    if n * (k - 1) >= 2 ** 31 // 3:
        raise ValueError("at most 2^31 / 3 - 1 triangle slots")
    tri = torch.empty(n * (k - 1), 3, dtype=torch.int32, device=nbr.device)
    check(lib.dp_mesh_fan(nbr.data_ptr(), nbr_count.data_ptr(), cptr, n, k, tri.data_ptr(), stream), "dp_mesh_fan")
    return tri


def clean_triangles(tri: torch.Tensor, n_vertices: int, count=None):
    """Open3D's `remove_degenerate_triangles` then `remove_duplicated_triangles` on a plain (T, 3) int32 list
    (`dp_mesh_clean_triangles`): (triangle buffer (T, 3), device int32 count, stats (8,) float64 in `TRIANGLE_STATS`
    order).  Dropped: a triangle with an index outside [0, n_vertices), one with two equal indices, and every later
    copy of a triangle -- two are copies when they are cyclic rotations of each other; the mirror image is another
    triangle.  The kept ones come in their input order and as they were.  Asynchronous, no read-back; `count`: the
    live triangles (int or device int32)."""
    if tri.dtype != torch.int32 or tri.dim() != 2 or tri.shape[1] != 3:
        raise ValueError("tri must be a (T, 3) int32 tensor")
    if not 0 <= int(n_vertices) < 2 ** 31:
        raise ValueError(f"n_vertices must be in [0, 2^31) (got {n_vertices})")
    if tri.device.type != "cuda":
        raise _lib.DPError(_MESH)
    src = tri.contiguous()
    t, dev = src.shape[0], src.device
    if t >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 triangles")
    count = _count_tensor(count, dev)
    lib = _lib.load()
    ws = torch.empty(int(lib.dp_mesh_workspace_size(0, t)), dtype=torch.uint8, device=dev)
    out = torch.empty_like(src)
    n_out = torch.empty(1, dtype=torch.int32, device=dev)
    stats = torch.empty(8, dtype=torch.float64, device=dev)
    check(lib.dp_mesh_clean_triangles(src.data_ptr(), None if count is None else count.data_ptr(), t, int(n_vertices),
                                      out.data_ptr(), n_out.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream(dev).cuda_stream), "dp_mesh_clean_triangles")
    return out, n_out, stats


def triangulate(points: torch.Tensor, count=None, neighbors: int = 6, cell_edge: float = 0.1):
    """`knn_exact(k = neighbors)`, `fan_triangles`, `clean_triangles` over one point set: (triangle buffer, device int32
    triangle count, knn stats, triangle stats).  The reference's create_simple_triangulated_mesh on points that are
    already down-sampled.  Nothing synchronised."""
    if not 2 <= int(neighbors) <= MAX_K:
        raise ValueError(f"neighbors must be in [2, {MAX_K}] (got {neighbors})")
    nbr, cnt, _, kst = knn_exact(points, count, neighbors, cell_edge)
    n, slots = nbr.shape[0], int(neighbors) - 1
    tri = fan_triangles(nbr, cnt, count)
    live = None
    if count is not None:                   # the fan's live slots, still on the device
        live = (_count_tensor(count, nbr.device).clamp(0, n) * slots).to(torch.int32)
    out, n_tri, tst = clean_triangles(tri, n, live)
    return out, n_tri, kst, tst


def simple_mesh(points: torch.Tensor, colors: Optional[torch.Tensor] = None, count=None, voxel_size: float = 0.05,
                neighbors: int = 6):
    """The reference's `--mesh_method simple` (pointcloud_to_mesh.py:313-395 with create_simple_triangulated_mesh,
    :423-465): `voxel_downsample(voxel_size)`, then for every voxel its `neighbors` nearest others (`knn_exact` on a
    grid of 2 * voxel_size), the fan of triangles over them, and the removal of degenerate and duplicated triangles.
    Returns (vertex buffer, colour buffer or None, device int32 vertex count, triangle buffer, device int32 triangle
    count, {"voxel": ..., "knn": ..., "triangles": ...} stats); the first `count` rows of each are the mesh.  On the
    device, nothing synchronised.  Not built: remove_duplicated_vertices (nothing to do after a voxel grid) and
    remove_non_manifold_edges (Open3D's result depends on a hash map's order)."""
    out, cout, _, _, n_out, vst = voxel_downsample(points, colors, count, voxel_size)
    tri, n_tri, kst, tst = triangulate(out, n_out, neighbors, 2.0 * float(voxel_size))
    return out, cout, n_out, tri, n_tri, {"voxel": vst, "knn": kst, "triangles": tst}


def mean_neighbor_distance(points: torch.Tensor, count=None, k: int = 20, cell_edge: float = 0.1) -> torch.Tensor:
    """The reference's `get_average_point_distance(pcd, k)` without its random sample (`dp_mesh_mean_distance` on the
    lists of `knn_exact`): per row the mean of sqrt(d2) over its listed neighbours in list order, then the mean over
    the rows that have any -- a device float64 scalar, 0 without such a row.  The reference's ball-pivoting radii are
    [2, 4, 8, 16] times it.  Stated difference: the reference averages over 1000 randomly sampled rows."""
    _, cnt, d2, _ = knn_exact(points, count, k, cell_edge)
    lib, n, k, cptr, stream, _ = _lists_args(d2, cnt, count)
    ws = torch.empty(int(lib.dp_mesh_workspace_size(n, 0)), dtype=torch.uint8, device=d2.device)
    out = torch.empty(2, dtype=torch.float64, device=d2.device)
    check(lib.dp_mesh_mean_distance(d2.data_ptr(), cnt.data_ptr(), cptr, n, k, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                    stream), "dp_mesh_mean_distance")
    return out[0]


BALL_PIVOT_FACTORS = (2, 4, 8, 16)      # the reference's radii, as multiples of the mean neighbour distance
PLY_FACE_RECORD = 13                    # bytes per face: uchar 3, then three uint32 vertex indices


def _mesh_ply_header(n: int, t: int, colored: bool) -> bytes:
    props = ["property double x", "property double y", "property double z"]
    if colored:
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    return ("\n".join(["ply", "format binary_little_endian 1.0", f"element vertex {n}", *props, f"element face {t}",
                       "property list uchar uint vertex_indices", "end_header"]) + "\n").encode("ascii")


def mesh_ply_records_async(xyz: torch.Tensor, cols: Optional[torch.Tensor], tri: torch.Tensor):
    """The records `write_mesh_ply` writes, interleaved on the device: vertex records ((N, 27) uint8 as
    `ply_records_async` makes them, (N, 24) without colours) and face records ((T, 13) uint8: the byte 3, then the
    three indices as little-endian uint32).  Queued on the current stream, no sync."""
    n, t = xyz.shape[0], tri.shape[0]
    if cols is not None:
        vrec = ply_records_async(xyz.contiguous(), cols)
    else:
        vrec = xyz.contiguous().view(torch.uint8).view(n, 24).clone()
    frec = torch.empty(t, PLY_FACE_RECORD, dtype=torch.uint8, device=tri.device)
    frec[:, 0] = 3
    frec[:, 1:].copy_(tri.contiguous().view(torch.uint8).view(t, 12))
    return vrec, frec


def write_mesh_ply(path: str, vertex_records: np.ndarray, face_records: np.ndarray) -> str:
    """Binary little-endian PLY of a triangle mesh from records already in file layout (`mesh_ply_records_async`):
    `element vertex` with double x, y, z (+ uchar red, green, blue), then `element face` with `property list uchar
    uint vertex_indices`.  Stated difference: the reference's default file is an OBJ written by Open3D."""
    vrec = np.ascontiguousarray(vertex_records, dtype=np.uint8)
    frec = np.ascontiguousarray(face_records, dtype=np.uint8)
    if vrec.ndim != 2 or vrec.shape[1] not in (PLY_RECORD, PLY_RECORD - 3):
        raise ValueError(f"vertex records must be (n, {PLY_RECORD}) or (n, {PLY_RECORD - 3}) uint8")
    if frec.ndim != 2 or frec.shape[1] != PLY_FACE_RECORD:
        raise ValueError(f"face records must be (t, {PLY_FACE_RECORD}) uint8")
    if not path.endswith(".ply"):
        path = path + ".ply"
    with open(path, "wb") as f:
        f.write(_mesh_ply_header(vrec.shape[0], frec.shape[0], vrec.shape[1] == PLY_RECORD))
        f.write(memoryview(vrec.reshape(-1)))            # flat first: a frame may leave no points
        f.write(memoryview(frec.reshape(-1)))
    return path


def read_mesh_ply(path: str) -> Tuple[np.ndarray, Optional[np.ndarray], np.ndarray]:
    """Reader for the files `write_mesh_ply` produces: (points (n, 3) float64, colours (n, 3) uint8 or None, triangles
    (t, 3) uint32)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    n = int(next(l for l in lines if l.startswith("element vertex")).split()[-1])
    face = [l for l in lines if l.startswith("element face")]
    if not face or "property list uchar uint vertex_indices" not in lines:
        raise ValueError(f"{path} has no faces")
    t = int(face[0].split()[-1])
    dt = [("p", "<f8", 3)] + ([("c", "u1", 3)] if any("red" in l for l in lines) else [])
    vert = np.frombuffer(data[end:], dtype=dt, count=n)
    faces = np.frombuffer(data[end + vert.nbytes:], dtype=[("k", "u1"), ("v", "<u4", 3)], count=t)
    if t and not (faces["k"] == 3).all():
        raise ValueError(f"{path} has faces that are not triangles")
    return vert["p"].copy(), (vert["c"].copy() if len(dt) == 2 else None), faces["v"].copy()


# ---- occupancy floor plan: raster, morphology, regions, picture (csrc/dp_floorplan.hip) -------------

GRID_STATS = ("participants", "non_finite", "below_threshold", "dropped", "occupied_cells", "height", "width", "error")
REGION_STATS = ("set_cells", "regions", "rows", "overflow", "height", "width", "reserved0", "reserved1")
REGION_COLUMNS = ("cells", "area", "gx0", "gz0", "gx1", "gz1", "cx", "cz", "x", "z", "points", "max_height", "mean_height")
FLOOR_MAX_DIM, FLOOR_MAX_KERNEL = _lib.DP_FLOOR_MAX_DIM, _lib.DP_FLOOR_MAX_KERNEL

_FLOOR = "the occupancy floor plan runs on the ROCm device (csrc/dp_floorplan.hip)"


def _check_floor(resolution=0.1, padding=0.0, height_threshold=1.3, max_cells=0, close_size=1, close_iters=0, open_size=1,
                 min_area=0.0, max_height=1.0, max_regions=0) -> None:
    if not (np.isfinite(float(resolution)) and float(resolution) > 0):
        raise ValueError(f"resolution must be finite and > 0 (got {resolution})")
    if not (np.isfinite(float(padding)) and float(padding) >= 0):
        raise ValueError(f"padding must be finite and >= 0 (got {padding})")
    if np.isinf(float(height_threshold)):
        raise ValueError("height_threshold must be finite, or NaN for every height")
    if not 0 <= int(max_cells) < 2 ** 31 or not 0 <= int(max_regions) < 2 ** 31:
        raise ValueError("max_cells and max_regions must be in [0, 2^31 - 1]")
    for name, k in (("close_size", close_size), ("open_size", open_size)):
        if not (1 <= int(k) <= FLOOR_MAX_KERNEL and int(k) % 2 == 1):
            raise ValueError(f"{name} must be odd and in [1, {FLOOR_MAX_KERNEL}] (got {k})")
    if int(close_iters) < 0:
        raise ValueError(f"close_iters must be >= 0 (got {close_iters})")
    if not (np.isfinite(float(min_area)) and float(min_area) >= 0):
        raise ValueError(f"min_area must be finite and >= 0 (got {min_area})")
    if not (np.isfinite(float(max_height)) and float(max_height) > 0):
        raise ValueError(f"max_height must be finite and > 0 (got {max_height})")


def _grid_args(grid: torch.Tensor, dims: torch.Tensor, dtype=torch.uint8, what: str = "grid"):
    """(lib, flat contiguous grid, capacity in cells, stream) of a grid stage; `dims` is the device (H, W)."""
    if grid.device.type != "cuda":
        raise _lib.DPError(_FLOOR)
    if grid.dtype != dtype:
        raise ValueError(f"{what} must be a {dtype} tensor")
    if not torch.is_tensor(dims) or dims.device != grid.device or dims.dtype != torch.int32 or dims.numel() != 2:
        raise ValueError("dims must be a device int32 tensor (H, W) on the grid's device")
    g = grid.contiguous().reshape(-1)
    if g.numel() >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 cells")
    return _lib.load(), g, g.numel(), torch.cuda.current_stream(g.device).cuda_stream


def grid_dims(shape, device) -> torch.Tensor:
    """A device `dims` for a grid made on the host: int32 (H, W)."""
    h, w = (int(v) for v in shape)
    return torch.tensor([h, w], dtype=torch.int32, device=device)


def occupancy_grid(points: torch.Tensor, colors: Optional[torch.Tensor] = None, count=None,
                   height_threshold: Optional[float] = 1.3, resolution: float = 0.1, padding: float = 0.2,
                   max_cells: int = 1 << 22) -> dict:
    """The reference's top-down density grid (`create_density_grid_from_points`, `create_direct_floorplan`) of the
    levelled cloud on the device (`dp_occupancy_grid`): the rows with y >= `height_threshold` (None or NaN: every
    height) fall into cells of `resolution` metres over (x, z) from (min - padding).  Returns a dict of device
    tensors: `density` (max_cells,) int32 holding the uint32 member counts, `height` (max_cells,) float32 (the
    largest y of a cell, 0 where empty), `color` (max_cells, 3) uint8 or None (the colour of the highest member, the
    smallest row among equals), `occupied` (max_cells,) uint8, `dims` int32 (H, W), `origin` float64 (min_x, min_z),
    `stats` (8,) float64 in `GRID_STATS` order.  The first H * W entries are the grid, row-major, row 0 = smallest z;
    x and z are as stored (no flip).  Asynchronous, no read-back.  stats["error"]: 1 without participants, 2 when
    the grid would exceed `max_cells` (or 8192 cells on a side); dims are then (0, 0) and nothing is written."""
    thr = float("nan") if height_threshold is None else float(height_threshold)
    _check_floor(resolution, padding, thr, max_cells)
    lib, pts, n, count, cptr, stream = _points_args(points, count, _FLOOR)
    cols = None
    if colors is not None:
        cols = colors.contiguous()
        if cols.dtype != torch.uint8 or tuple(cols.shape) != (n, 3):
            raise ValueError("colors must be an (N, 3) uint8 tensor")
    dev, mc = pts.device, int(max_cells)
    ws = torch.empty(int(lib.dp_floorplan_workspace_size(mc, 0)), dtype=torch.uint8, device=dev)
    out = {"density": torch.empty(mc, dtype=torch.int32, device=dev), "height": torch.empty(mc, dtype=torch.float32, device=dev),
           "color": None if cols is None else torch.empty(mc, 3, dtype=torch.uint8, device=dev),
           "occupied": torch.empty(mc, dtype=torch.uint8, device=dev), "dims": torch.empty(2, dtype=torch.int32, device=dev),
           "origin": torch.empty(2, dtype=torch.float64, device=dev), "stats": torch.empty(8, dtype=torch.float64, device=dev)}
    check(lib.dp_occupancy_grid(pts.data_ptr(), None if cols is None else cols.data_ptr(), cptr, n, thr, float(resolution),
                                float(padding), mc, out["density"].data_ptr(), out["height"].data_ptr(),
                                None if cols is None else out["color"].data_ptr(), out["occupied"].data_ptr(),
                                out["dims"].data_ptr(), out["origin"].data_ptr(), out["stats"].data_ptr(), ws.data_ptr(),
                                ws.numel(), stream), "dp_occupancy_grid")
    return out


def grid_morphology(grid: torch.Tensor, dims: torch.Tensor, close_size: int = 7, close_iters: int = 2, open_size: int = 3,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`cv2.morphologyEx` on a binary uint8 grid (`dp_grid_morphology`): `close_iters` closings by a `close_size`
    square of ones, then one opening by `open_size` -- the reference's `process_height_slice` with the defaults.
    OpenCV's border rule: a dilation reads outside cells as 0, an erosion as 1.  `grid` holds the capacity, `dims`
    (device int32 H, W) says what is used.  Returns a 0 / 1 grid of the same capacity (`out=grid`: in place).
    Asynchronous, no read-back."""
    _check_floor(close_size=close_size, close_iters=close_iters, open_size=open_size)
    lib, g, mc, stream = _grid_args(grid, dims)
    if out is None:
        out = torch.empty_like(g)
    elif out.dtype != torch.uint8 or out.device != g.device or out.numel() != mc or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 tensor of the grid's size on its device")
    ws = torch.empty(int(lib.dp_floorplan_workspace_size(mc, 0)), dtype=torch.uint8, device=g.device)
    check(lib.dp_grid_morphology(g.data_ptr(), dims.data_ptr(), mc, int(close_size), int(close_iters), int(open_size),
                                 out.data_ptr(), ws.data_ptr(), ws.numel(), stream), "dp_grid_morphology")
    return out


def grid_regions(grid: torch.Tensor, dims: torch.Tensor, density: torch.Tensor, height: torch.Tensor, origin: torch.Tensor,
                 resolution: float = 0.1, max_regions: int = 4096):
    """The 8-connected regions of a binary uint8 grid and their table (`dp_grid_regions`): (labels (max_cells,) int32 --
    0 on background, regions numbered from 1 in row-major order of their first cell, as
    `scipy.ndimage.label(structure=ones((3, 3)))` --, device int32 region count, table (max_regions,
    len(REGION_COLUMNS)) float64 in `REGION_COLUMNS` order, stats (8,) float64 in `REGION_STATS` order).  `density`,
    `height` and `origin` are `occupancy_grid`'s.  Regions past `max_regions` keep their labels, have no row and raise
    stats["overflow"].  Asynchronous, no read-back."""
    _check_floor(resolution, max_regions=max_regions)
    lib, g, mc, stream = _grid_args(grid, dims)
    dev, mr = g.device, int(max_regions)
    for name, t, dt, numel in (("density", density, torch.int32, mc), ("height", height, torch.float32, mc),
                               ("origin", origin, torch.float64, 2)):
        if not torch.is_tensor(t) or t.device != dev or t.dtype != dt or t.numel() != numel or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} tensor of {numel} entries on the grid's device")
    ws = torch.empty(int(lib.dp_floorplan_workspace_size(mc, mr)), dtype=torch.uint8, device=dev)
    labels = torch.empty(mc, dtype=torch.int32, device=dev)
    n_regions = torch.empty(1, dtype=torch.int32, device=dev)
    table = torch.zeros(mr, len(REGION_COLUMNS), dtype=torch.float64, device=dev)
    stats = torch.empty(8, dtype=torch.float64, device=dev)
    check(lib.dp_grid_regions(g.data_ptr(), density.data_ptr(), height.data_ptr(), dims.data_ptr(), origin.data_ptr(), mc,
                              float(resolution), mr, labels.data_ptr(), n_regions.data_ptr(), table.data_ptr(),
                              stats.data_ptr(), ws.data_ptr(), ws.numel(), stream), "dp_grid_regions")
    return labels, n_regions, table, stats


def floorplan_image(labels: torch.Tensor, dims: torch.Tensor, table: torch.Tensor, n_regions: torch.Tensor,
                    resolution: float = 0.1, min_area: float = 0.025, max_height: float = 2.5,
                    color_by_height: bool = True) -> torch.Tensor:
    """The picture of `create_direct_floorplan` from the regions (`dp_floorplan_image`): (max_cells, 3) uint8 RGB, the
    first H * W pixels row-major with row 0 = smallest z.  White background; a region with area >= `min_area` is filled
    with the reference's height colour of its mean height (grey 180 without `color_by_height`) and outlined in black
    where its 4-neighbourhood leaves it; smaller regions are blank; the reference's 1 m scale bar where its condition
    allows one, no text.  Asynchronous, no read-back."""
    _check_floor(resolution, min_area=min_area, max_height=max_height)
    lib, lab, mc, stream = _grid_args(labels, dims, torch.int32, "labels")
    if table.device != lab.device or table.dtype != torch.float64 or table.dim() != 2 or \
            table.shape[1] != len(REGION_COLUMNS) or not table.is_contiguous():
        raise ValueError(f"table must be a contiguous (max_regions, {len(REGION_COLUMNS)}) float64 tensor on the labels' device")
    if n_regions.device != lab.device or n_regions.dtype != torch.int32 or n_regions.numel() != 1:
        raise ValueError("n_regions must be a device int32 scalar")
    img = torch.empty(mc, 3, dtype=torch.uint8, device=lab.device)
    check(lib.dp_floorplan_image(lab.data_ptr(), dims.data_ptr(), mc, table.data_ptr(), n_regions.data_ptr(),
                                 int(table.shape[0]), float(resolution), float(min_area), float(max_height),
                                 int(bool(color_by_height)), img.data_ptr(), stream), "dp_floorplan_image")
    return img


def floor_plan(points: torch.Tensor, colors: Optional[torch.Tensor] = None, count=None,
               height_threshold: Optional[float] = 1.3, resolution: float = 0.1, padding: float = 0.2, close_size: int = 7,
               close_iters: int = 2, open_size: int = 3, min_area: float = 0.025, max_height: float = 2.5,
               max_cells: int = 1 << 22, max_regions: int = 4096) -> dict:
    """The reference's occupancy floor plan (`cleaned_pointcloud_to_floorplan.py`) up to its contour tracing:
    `occupancy_grid`, `grid_morphology`, `grid_regions`, `floorplan_image`, with the reference's height-threshold
    values (resolution 0.05 doubled, padding 0.2, closing 7 x 7 twice, opening 3 x 3, min_area 0.1 / 4, height_max
    2.5).  Returns `occupancy_grid`'s dict with `cleaned` (the grid after morphology), `labels`, `n_regions`, `table`,
    `region_stats` and `image` added, and the parameters under `parameters`; all tensors on the device, nothing
    synchronised.  Stated differences: a region's area is its cell count (the reference: `contourArea` of a traced
    outline); no text.  The traced outlines, their simplification and the polygons file are `floor_polygons`."""
    _check_floor(resolution, padding, float("nan") if height_threshold is None else float(height_threshold), max_cells,
                 close_size, close_iters, open_size, min_area, max_height, max_regions)
    out = occupancy_grid(points, colors, count, height_threshold, resolution, padding, max_cells)
    out["cleaned"] = grid_morphology(out["occupied"], out["dims"], close_size, close_iters, open_size)
    out["labels"], out["n_regions"], out["table"], out["region_stats"] = grid_regions(
        out["cleaned"], out["dims"], out["density"], out["height"], out["origin"], resolution, max_regions)
    out["image"] = floorplan_image(out["labels"], out["dims"], out["table"], out["n_regions"], resolution, min_area,
                                   max_height)
    out["parameters"] = {"height_threshold": None if height_threshold is None or height_threshold != height_threshold
                         else float(height_threshold), "resolution": float(resolution), "padding": float(padding),
                         "close_size": int(close_size), "close_iters": int(close_iters), "open_size": int(open_size),
                         "min_area": float(min_area), "max_height": float(max_height)}
    return out


def floor_plan_summary(plan: dict) -> dict:
    """The `{base}_floorplan.json` content and the picture from a `floor_plan` result: the one read-back (it
    synchronises the current stream).  Returns {"origin", "resolution", "height", "width", "parameters", "stats",
    "region_stats", "regions": one object per region with area >= min_area in label order, "image": (H, W, 3) uint8
    numpy array}.  Everything but "image" is JSON-serialisable."""
    small = torch.cat([plan["dims"].to(torch.float64), plan["origin"], plan["stats"], plan["region_stats"],
                       plan["n_regions"].to(torch.float64)]).cpu().numpy()
    h, w = int(small[0]), int(small[1])
    params = plan["parameters"]
    rows = min(int(small[20]), plan["table"].shape[0])
    table = plan["table"][:rows].cpu().numpy()
    img = plan["image"][:h * w].cpu().numpy().reshape(h, w, 3)
    regions = [{"label": r + 1, **{k: (int(v) if k in ("cells", "gx0", "gz0", "gx1", "gz1", "points") else float(v))
                                  for k, v in zip(REGION_COLUMNS, row)}}
               for r, row in enumerate(table) if row[1] >= params["min_area"]]
    return {"origin": [float(small[2]), float(small[3])], "resolution": params["resolution"], "height": h, "width": w,
            "parameters": dict(params), "stats": {k: float(v) for k, v in zip(GRID_STATS, small[4:12])},
            "region_stats": {k: float(v) for k, v in zip(REGION_STATS, small[12:20])}, "regions": regions, "image": img}


# ---- floor-plan polygons: outlines, simplification, the polygons file (csrc/dp_outline.hip) -----------

OUTLINE_COLUMNS = ("vertices", "border_cells", "shoelace", "start_cell")
OUTLINE_MEASURES = ("area", "perimeter")
OUTLINE_STATS = ("regions", "rows", "vertices", "vertices_written", "vertex_overflow", "region_overflow", "height", "width")
POLYGON_COLUMNS = ("label", "vertices", "flags", "area_cells", "area", "epsilon", "drop_reason", "outline_vertices")
POLYGON_STATS = ("rows", "polygons", "vertices", "vertices_written", "overflow", "too_small", "too_few", "invalid")
DROP_REASONS = ("kept", "too_small", "fewer_than_3_vertices", "invalid", "overflow")
POLYGON_SNAPPED = 1

_OUTLINE = "the floor-plan polygons run on the ROCm device (csrc/dp_outline.hip)"


def _plan_args(plan: dict, keys):
    """The device tensors `keys` of a `floor_plan` result, checked; (lib, device, max_regions, stream)."""
    if not isinstance(plan, dict) or any(k not in plan for k in keys):
        raise ValueError(f"plan must be a floor_plan result holding {', '.join(keys)}")
    dev = plan[keys[0]].device
    if dev.type != "cuda":
        raise _lib.DPError(_OUTLINE)
    for k in keys:
        t = plan[k]
        if not torch.is_tensor(t) or t.device != dev or not t.is_contiguous():
            raise ValueError(f"plan[{k!r}] must be a contiguous tensor on the plan's device")
    return _lib.load(), dev, int(plan["table"].shape[0]), torch.cuda.current_stream(dev).cuda_stream


def _check_capacity(name: str, v) -> int:
    if not 0 <= int(v) < 2 ** 31:
        raise ValueError(f"{name} must be in [0, 2^31 - 1] (got {v})")
    return int(v)


def region_outlines(plan: dict, max_vertices: int = 1 << 20) -> dict:
    """The outline of every region of a `floor_plan` result (`dp_region_outlines`): `cv2.findContours(RETR_EXTERNAL,
    CHAIN_APPROX_SIMPLE)` restated as rules O1-O5 of the header.  Adds to `plan` and returns it: `outline_offsets`
    (max_regions + 1,) int32, `outline_vertices` (max_vertices, 2) int32 (x = gx, y = gz), `outline_columns`
    (max_regions, 4) int64 in `OUTLINE_COLUMNS` order, `outline_measures` (max_regions, 2) float64 (`contourArea`,
    `arcLength`), `outline_stats` (8,) float64 in `OUTLINE_STATS` order.  A region whose vertices do not fit keeps its
    columns, writes none and raises stats["vertex_overflow"].  Asynchronous, no read-back."""
    mv = _check_capacity("max_vertices", max_vertices)
    lib, dev, mr, stream = _plan_args(plan, ("labels", "dims", "n_regions", "table"))
    lab, dims, nreg = plan["labels"], plan["dims"], plan["n_regions"]
    if lab.dtype != torch.int32 or dims.dtype != torch.int32 or dims.numel() != 2 or nreg.dtype != torch.int32 or nreg.numel() != 1:
        raise ValueError("plan labels, dims and n_regions must be int32 tensors as floor_plan returns them")
    mc = lab.numel()
    ws = torch.empty(int(lib.dp_outline_workspace_size(mc, mr, mv)), dtype=torch.uint8, device=dev)
    plan["outline_offsets"] = torch.zeros(mr + 1, dtype=torch.int32, device=dev)
    plan["outline_vertices"] = torch.empty(mv, 2, dtype=torch.int32, device=dev)
    plan["outline_columns"] = torch.zeros(mr, len(OUTLINE_COLUMNS), dtype=torch.int64, device=dev)
    plan["outline_measures"] = torch.zeros(mr, len(OUTLINE_MEASURES), dtype=torch.float64, device=dev)
    plan["outline_stats"] = torch.empty(8, dtype=torch.float64, device=dev)
    check(lib.dp_region_outlines(lab.data_ptr(), dims.data_ptr(), mc, nreg.data_ptr(), mr, mv, plan["outline_offsets"].data_ptr(),
                                 plan["outline_vertices"].data_ptr(), plan["outline_columns"].data_ptr(),
                                 plan["outline_measures"].data_ptr(), plan["outline_stats"].data_ptr(), ws.data_ptr(),
                                 ws.numel(), stream), "dp_region_outlines")
    return plan


def _simplify(plan: dict, max_polygon_vertices: int, resolution: Optional[float], call) -> dict:
    """The part `simplify_outlines` and `simplify_outlines_with` share: checks, the output tensors, and `call(lib, head,
    res, tail)` with the entry point's arguments in front of and behind its own parameters."""
    mp = _check_capacity("max_polygon_vertices", max_polygon_vertices)
    keys = ("outline_offsets", "outline_vertices", "outline_columns", "outline_measures", "n_regions", "table")
    if isinstance(plan, dict) and "outline_offsets" not in plan and "labels" in plan:
        raise ValueError("plan holds no outlines: call region_outlines first")
    lib, dev, mr, stream = _plan_args(plan, keys)
    res = float(plan.get("parameters", {})["resolution"] if resolution is None else resolution)
    _check_floor(res)
    mv = int(plan["outline_vertices"].shape[0])
    ws = torch.empty(int(lib.dp_outline_workspace_size(0, mr, mv)), dtype=torch.uint8, device=dev)
    plan["polygon_offsets"] = torch.zeros(mr + 1, dtype=torch.int32, device=dev)
    plan["polygon_vertices"] = torch.empty(mp, 2, dtype=torch.float64, device=dev)
    plan["polygons"] = torch.zeros(mr, len(POLYGON_COLUMNS), dtype=torch.float64, device=dev)
    plan["polygon_stats"] = torch.empty(8, dtype=torch.float64, device=dev)
    head = (plan["outline_offsets"].data_ptr(), plan["outline_vertices"].data_ptr(), plan["outline_columns"].data_ptr(),
            plan["outline_measures"].data_ptr(), plan["n_regions"].data_ptr(), mr, mv, res)
    tail = (mp, plan["polygon_offsets"].data_ptr(), plan["polygon_vertices"].data_ptr(), plan["polygons"].data_ptr(),
            plan["polygon_stats"].data_ptr(), ws.data_ptr(), ws.numel(), stream)
    call(lib, head, tail)
    return plan


def simplify_outlines(plan: dict, max_polygon_vertices: int = 1 << 18, resolution: Optional[float] = None,
                      min_area: Optional[float] = None) -> dict:
    """The reference's `approximate_contour` on the outlines of `region_outlines` (`dp_simplify_outlines`, rules S1-S7
    of the header): area filter (`min_area` / 4), epsilon = 0.005 * perimeter, closed Douglas-Peucker, `is_valid`, the
    rectangle snap.  `resolution` and `min_area` default to the plan's parameters.  Adds to `plan` and returns it:
    `polygon_offsets` (max_regions + 1,) int32, `polygon_vertices` (max_polygon_vertices, 2) float64 in grid units,
    `polygons` (max_regions, 8) float64 in `POLYGON_COLUMNS` order -- one row per region, `drop_reason` indexing
    `DROP_REASONS` -- and `polygon_stats` (8,) float64 in `POLYGON_STATS` order.  Asynchronous, no read-back.
    Stated difference: OpenCV's final clean-up pass of `approxPolyDP` is not built."""
    _check_capacity("max_polygon_vertices", max_polygon_vertices)
    if isinstance(plan, dict) and "outline_offsets" not in plan and "labels" in plan:
        raise ValueError("plan holds no outlines: call region_outlines first")
    if not isinstance(plan, dict):
        raise ValueError("plan must be a floor_plan result")
    area = float(plan.get("parameters", {})["min_area"] if min_area is None else min_area)
    _check_floor(min_area=area)
    return _simplify(plan, max_polygon_vertices, resolution, lambda lib, head, tail: check(
        lib.dp_simplify_outlines(*head, area, *tail), "dp_simplify_outlines"))


def simplify_outlines_with(plan: dict, area_floor: float, alpha: float, max_polygon_vertices: int = 1 << 18,
                           resolution: Optional[float] = None) -> dict:
    """`simplify_outlines` with the two constants of rules S1 and S2 given by the caller (`dp_simplify_outlines_with`):
    a region is dropped when its outline's area in m^2 is below `area_floor`, and epsilon = `alpha` * perimeter.
    `simplify_outlines(min_area)` is `(min_area / 4, 0.005)`, the reference's height-threshold mode; its default mode
    is `(0.1, 0.01)`.  Same outputs; asynchronous, no read-back."""
    for name, v in (("area_floor", area_floor), ("alpha", alpha)):
        if not (np.isfinite(float(v)) and float(v) >= 0):
            raise ValueError(f"{name} must be finite and >= 0 (got {v})")
    return _simplify(plan, max_polygon_vertices, resolution, lambda lib, head, tail: check(
        lib.dp_simplify_outlines_with(*head, float(area_floor), float(alpha), *tail), "dp_simplify_outlines_with"))


def floor_mean_height(points: torch.Tensor, count=None, height_threshold: Optional[float] = 1.3) -> torch.Tensor:
    """(2,) float64 on the device: the mean y of the raster's participants (the finite rows with y >= the threshold;
    None or NaN: every finite row) and their number -- the height label of the reference's polygons file
    (`create_height_slices`).  Without participants the mean is the threshold.  Asynchronous, no read-back."""
    thr = float("nan") if height_threshold is None else float(height_threshold)
    _check_floor(height_threshold=thr)
    lib, pts, n, count, cptr, stream = _points_args(points, count, _OUTLINE)
    out = torch.empty(2, dtype=torch.float64, device=pts.device)
    check(lib.dp_floor_mean_height(pts.data_ptr(), cptr, n, thr, out.data_ptr(), stream), "dp_floor_mean_height")
    return out


def floor_polygons(plan: dict, points: Optional[torch.Tensor] = None, count=None, max_vertices: int = 1 << 20,
                   max_polygon_vertices: int = 1 << 18) -> dict:
    """`region_outlines`, then `simplify_outlines`, on a `floor_plan` result; with `points` (the cloud the plan was made
    from) also `mean_height` (`floor_mean_height` with the plan's threshold).  Returns `plan` with their tensors added;
    all on the device, nothing synchronised."""
    _check_capacity("max_vertices", max_vertices)
    _check_capacity("max_polygon_vertices", max_polygon_vertices)
    region_outlines(plan, max_vertices)
    simplify_outlines(plan, max_polygon_vertices)
    if points is not None:
        plan["mean_height"] = floor_mean_height(points, count, plan["parameters"]["height_threshold"])
    return plan


def reference_world(xy: np.ndarray, origin, resolution: float) -> np.ndarray:
    """Grid-unit vertices as the reference's file holds them: `shapely.affinity.scale` with its default origin scales
    about the centre of the polygon's bounding box (in grid units), then the grid origin is added."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    cx = (xy[:, 0].min() + xy[:, 0].max()) / 2.0
    cy = (xy[:, 1].min() + xy[:, 1].max()) / 2.0
    return np.stack([cx + (xy[:, 0] - cx) * resolution + origin[0], cy + (xy[:, 1] - cy) * resolution + origin[1]], axis=1)


def floor_polygons_summary(plan: dict) -> dict:
    """The `{base}_floorplan_polygons.json` content from a `floor_polygons` result: the one read-back (it synchronises
    the current stream).  {"origin", "resolution", "height" (the mean height of the participants; the threshold when the
    plan has no `mean_height`), "participants", "parameters", "outline_stats", "polygon_stats", "polygons": one object
    per kept polygon in label order -- label, snapped, flags, area_cells, area, epsilon, outline_vertices,
    vertices_grid, vertices (origin + x * resolution) and vertices_reference (the reference file's arithmetic) --,
    "dropped": [{label, reason}]}.  JSON-serialisable."""
    if "polygons" not in plan or "polygon_offsets" not in plan:
        raise ValueError("plan holds no polygons: call floor_polygons first")
    params = plan["parameters"]
    mean = plan.get("mean_height")
    small = torch.cat([plan["origin"], plan["outline_stats"], plan["polygon_stats"], plan["n_regions"].to(torch.float64),
                       mean if mean is not None else torch.zeros(2, dtype=torch.float64, device=plan["origin"].device)]
                      ).cpu().numpy()
    origin = [float(small[0]), float(small[1])]
    res = params["resolution"]
    rows = min(max(int(small[18]), 0), plan["polygons"].shape[0])
    pol = plan["polygons"][:rows].cpu().numpy()
    off = plan["polygon_offsets"][:rows + 1].cpu().numpy()
    verts = plan["polygon_vertices"][:int(off[rows]) if rows else 0].cpu().numpy()
    thr = params.get("height_threshold")
    height = float(small[19]) if mean is not None else (float(thr) if thr is not None else 0.0)
    polygons, dropped = [], []
    for r, row in enumerate(pol):
        if row[6] != 0 or row[1] < 1:
            dropped.append({"label": r + 1, "reason": DROP_REASONS[int(row[6])]})
            continue
        xy = verts[off[r]:off[r + 1]]
        polygons.append({"label": r + 1, "snapped": bool(int(row[2]) & POLYGON_SNAPPED), "flags": int(row[2]),
                         "area_cells": float(row[3]), "area": float(row[4]), "epsilon": float(row[5]),
                         "outline_vertices": int(row[7]), "vertices_grid": xy.tolist(),
                         "vertices": (np.asarray(origin) + xy * res).tolist(),
                         "vertices_reference": reference_world(xy, origin, res).tolist()})
    return {"origin": origin, "resolution": res, "height": height,
            "participants": int(small[20]) if mean is not None else None, "parameters": dict(params),
            "outline_stats": {k: float(v) for k, v in zip(OUTLINE_STATS, small[2:10])},
            "polygon_stats": {k: float(v) for k, v in zip(POLYGON_STATS, small[10:18])}, "polygons": polygons,
            "dropped": dropped}


def export_floorplan_text(path: str, summary: dict) -> str:
    """The reference's `{base}_floorplan.txt` (`save_floorplan_data`) from a `floor_polygons_summary`: its five header
    lines, then one line per polygon, `height, n, x1, z1, ...` with three decimals, in the reference's coordinates
    (`vertices_reference`).  All heights are equal, so the reference's stable sort keeps OpenCV's contour order, which
    is last-found first: descending label."""
    lines = ["# Floor Plan Data\n", "# Units: meters\n\n", "# Shapes by height\n",
             "# Format: height, num_points, x1, z1, x2, z2, ...\n"]
    height = summary["height"]
    for p in sorted(summary["polygons"], key=lambda q: -q["label"]):
        xy = p["vertices_reference"]
        lines.append(f"{height:.3f}, {len(xy)}" + "".join(f", {x:.3f}, {z:.3f}" for x, z in xy) + "\n")
    tmp = path + ".tmp"
    with open(tmp, "w") as f:
        f.write("".join(lines))
    os.replace(tmp, path)
    return path


# ---- height-sliced floor plan: slices, adaptive closing, polygons (csrc/dp_slices.hip) -----------------

SLICE_STATS = ("participants", "dropped", "occupied_cells", "height", "width", "status", "reserved0", "reserved1")
SLICE_STATUS = ("ok", "too_few_points", "too_large")
SLICE_MAX = _lib.DP_SLICE_MAX

_SLICES = "the height-sliced floor plan runs on the ROCm device (csrc/dp_slices.hip)"


def _check_slices(num_slices, max_cells, height_min=0.0, height_max=1.0, min_points=0) -> Tuple[int, int]:
    s, mc = int(num_slices), int(max_cells)
    if not 1 <= s <= SLICE_MAX:
        raise ValueError(f"num_slices must be in [1, {SLICE_MAX}] (got {num_slices})")
    if mc < 0 or s * mc >= 2 ** 31:
        raise ValueError("max_cells must be >= 0 with num_slices * max_cells <= 2^31 - 1")
    if not (np.isfinite(float(height_min)) and np.isfinite(float(height_max)) and float(height_max) > float(height_min)):
        raise ValueError(f"height_min and height_max must be finite with height_max > height_min (got {height_min}, {height_max})")
    if int(min_points) < 0:
        raise ValueError(f"min_points must be >= 0 (got {min_points})")
    return s, mc


def _stack_args(grid: torch.Tensor, dims: torch.Tensor):
    """(lib, contiguous (S, max_cells) grid, S, max_cells, stream) of a stage over stacked slice grids."""
    if grid.device.type != "cuda":
        raise _lib.DPError(_SLICES)
    if grid.dtype != torch.uint8 or grid.dim() != 2:
        raise ValueError("grid must be a (num_slices, max_cells) uint8 tensor")
    s, mc = _check_slices(grid.shape[0], grid.shape[1])
    if not torch.is_tensor(dims) or dims.device != grid.device or dims.dtype != torch.int32 or tuple(dims.shape) != (s, 2) or \
            not dims.is_contiguous():
        raise ValueError("dims must be a contiguous device int32 tensor (num_slices, 2) on the grid's device")
    return _lib.load(), grid.contiguous(), s, mc, torch.cuda.current_stream(grid.device).cuda_stream


def slice_grids(points: torch.Tensor, count=None, height_min: float = 0.1, height_max: float = 2.5, num_slices: int = 5,
                resolution: float = 0.05, padding: float = 0.5, min_points: int = 10, max_cells: int = 1 << 20) -> dict:
    """The grids of all height slices of the levelled cloud in two passes over it (`dp_slice_grids`, rules R1-R4 of the
    header): the reference's `create_height_slices` and the raster of `process_height_slice`.  Slice s holds the finite
    rows with lo_s <= y < hi_s; each has its own bounds, grid and origin.  Returns a dict of device tensors, S =
    `num_slices`: `density` (S, max_cells) int32 holding the uint32 counts, `height` (S, max_cells) float32, `occupied`
    (S, max_cells) uint8, `dims` (S, 2) int32 (H, W), `origin` (S, 2) float64, `bounds` (S, 3) float64 (lo, hi, mid),
    `stats` (S, 8) float64 in `SLICE_STATS` order.  `max_cells` is the capacity per slice; row s of a per-cell tensor is
    slice s, its first H * W entries the grid.  status 1: fewer than `min_points` rows, 2: the grid would exceed
    `max_cells`; such a slice has dims (0, 0) and the others are unaffected.  Asynchronous, no read-back."""
    s, mc = _check_slices(num_slices, max_cells, height_min, height_max, min_points)
    _check_floor(resolution, padding)
    lib, pts, n, count, cptr, stream = _points_args(points, count, _SLICES)
    dev = pts.device
    ws = torch.empty(int(lib.dp_slices_workspace_size(s, mc)), dtype=torch.uint8, device=dev)
    out = {"density": torch.empty(s, mc, dtype=torch.int32, device=dev), "height": torch.empty(s, mc, dtype=torch.float32, device=dev),
           "occupied": torch.empty(s, mc, dtype=torch.uint8, device=dev), "dims": torch.empty(s, 2, dtype=torch.int32, device=dev),
           "origin": torch.empty(s, 2, dtype=torch.float64, device=dev), "bounds": torch.empty(s, 3, dtype=torch.float64, device=dev),
           "stats": torch.empty(s, 8, dtype=torch.float64, device=dev)}
    check(lib.dp_slice_grids(pts.data_ptr(), cptr, n, float(height_min), float(height_max), s, float(resolution), float(padding),
                             int(min_points), mc, out["density"].data_ptr(), out["height"].data_ptr(), out["occupied"].data_ptr(),
                             out["dims"].data_ptr(), out["origin"].data_ptr(), out["bounds"].data_ptr(), out["stats"].data_ptr(),
                             ws.data_ptr(), ws.numel(), stream), "dp_slice_grids")
    return out


def slice_closing_sizes(grid: torch.Tensor, dims: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The closing size each slice's raw binary grid asks for (`dp_slice_closing_sizes`, rules C1-C2): the reference's
    `get_optimal_closing_kernel_size` -- the mean size of the 8-connected components picks 3, 5, 7, 9 or 11 -- as an
    exact integer rule.  `grid` (S, max_cells) uint8 and `dims` (S, 2) are `slice_grids`' `occupied` and `dims`.
    Returns (close_size (S,) int32, counts (S, 2) int64 = set cells, components) on the device; no read-back."""
    lib, g, s, mc, stream = _stack_args(grid, dims)
    ws = torch.empty(int(lib.dp_slices_workspace_size(s, mc)), dtype=torch.uint8, device=g.device)
    size = torch.empty(s, dtype=torch.int32, device=g.device)
    counts = torch.empty(s, 2, dtype=torch.int64, device=g.device)
    check(lib.dp_slice_closing_sizes(g.data_ptr(), dims.data_ptr(), s, mc, size.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                     ws.numel(), stream), "dp_slice_closing_sizes")
    return size, counts


def slice_morphology(grid: torch.Tensor, dims: torch.Tensor, close_size: torch.Tensor, close_iters: int = 1, open_size: int = 3,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`grid_morphology` for all slices in one call, the closing size of slice s read on the device from `close_size`
    (S,) int32 (`dp_slice_morphology`); a size that is not odd or not in [1, 15] acts as 1.  `close_iters` closings,
    then one opening by `open_size` -- the reference's default mode with (1, 3).  Returns a 0 / 1 grid (S, max_cells)
    (`out=grid`: in place).  Asynchronous, no read-back."""
    _check_floor(close_iters=close_iters, open_size=open_size)
    lib, g, s, mc, stream = _stack_args(grid, dims)
    if not torch.is_tensor(close_size) or close_size.device != g.device or close_size.dtype != torch.int32 or \
            close_size.numel() != s or not close_size.is_contiguous():
        raise ValueError("close_size must be a contiguous device int32 tensor of num_slices entries on the grid's device")
    if out is None:
        out = torch.empty_like(g)
    elif out.dtype != torch.uint8 or out.device != g.device or tuple(out.shape) != (s, mc) or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 tensor of the grid's shape on its device")
    ws = torch.empty(int(lib.dp_slices_workspace_size(s, mc)), dtype=torch.uint8, device=g.device)
    check(lib.dp_slice_morphology(g.data_ptr(), dims.data_ptr(), s, mc, close_size.data_ptr(), int(close_iters), int(open_size),
                                  out.data_ptr(), ws.data_ptr(), ws.numel(), stream), "dp_slice_morphology")
    return out


def sliced_floor_plan(points: torch.Tensor, count=None, height_min: float = 0.1, height_max: float = 2.5, num_slices: int = 5,
                      resolution: float = 0.05, padding: float = 0.5, min_points: int = 10, min_area: float = 0.1,
                      alpha: float = 0.01, open_size: int = 3, max_cells: int = 1 << 20, max_regions: int = 4096,
                      max_vertices: int = 1 << 20, max_polygon_vertices: int = 1 << 18) -> dict:
    """The default mode of the reference's `cleaned_pointcloud_to_floorplan.py` (no height threshold): `slice_grids`,
    `slice_closing_sizes` and `slice_morphology` once for all slices, then per slice, on the views of its rows,
    `grid_regions`, `region_outlines` and `simplify_outlines_with(min_area, alpha)` -- one closing of the adaptive size,
    one opening, alpha and min_area undivided.  Returns `slice_grids`' dict with `close_size`, `counts`, `cleaned`,
    `parameters` and `slices` added: a list of one plan dict per slice with the keys `floor_plan`, `region_outlines`
    and `simplify_outlines` use.  Every slice runs every stage (its status is only known on the device; a skipped slice
    has an empty grid and no regions).  All tensors on the device, nothing synchronised."""
    _check_slices(num_slices, max_cells, height_min, height_max, min_points)
    _check_floor(resolution, padding, max_cells=max_cells, open_size=open_size, min_area=min_area, max_regions=max_regions)
    if not (np.isfinite(float(alpha)) and float(alpha) >= 0):
        raise ValueError(f"alpha must be finite and >= 0 (got {alpha})")
    _check_capacity("max_vertices", max_vertices)
    _check_capacity("max_polygon_vertices", max_polygon_vertices)
    out = slice_grids(points, count, height_min, height_max, num_slices, resolution, padding, min_points, max_cells)
    out["close_size"], out["counts"] = slice_closing_sizes(out["occupied"], out["dims"])
    out["cleaned"] = slice_morphology(out["occupied"], out["dims"], out["close_size"], 1, open_size)
    out["parameters"] = {"height_min": float(height_min), "height_max": float(height_max), "num_slices": int(num_slices),
                         "resolution": float(resolution), "padding": float(padding), "min_points": int(min_points),
                         "min_area": float(min_area), "alpha": float(alpha), "close_iters": 1, "open_size": int(open_size)}
    out["slices"] = []
    for s in range(int(num_slices)):
        plan = {k: out[k][s] for k in ("density", "height", "occupied", "cleaned", "dims", "origin")}
        plan["parameters"] = {"resolution": float(resolution), "min_area": float(min_area), "alpha": float(alpha),
                              "height_threshold": None}
        plan["labels"], plan["n_regions"], plan["table"], plan["region_stats"] = grid_regions(
            plan["cleaned"], plan["dims"], plan["density"], plan["height"], plan["origin"], resolution, max_regions)
        region_outlines(plan, max_vertices)
        simplify_outlines_with(plan, min_area, alpha, max_polygon_vertices)
        out["slices"].append(plan)
    return out


def sliced_floor_plan_summary(plan: dict) -> dict:
    """The `{base}_floorslices.json` content from a `sliced_floor_plan` result: the read-back (it synchronises the
    current stream).  {"resolution", "parameters", "slices": one object per slice in ascending height -- index, lo, hi,
    height (the slice's mid height, the label of its polygons), participants, dropped_rows, occupied_cells, status
    (`SLICE_STATUS`), grid [H, W], origin, set_cells, components, close_size, region_stats, and `floor_polygons_summary`'s
    outline_stats, polygon_stats, polygons and dropped}.  JSON-serialisable."""
    if "slices" not in plan or "bounds" not in plan:
        raise ValueError("plan holds no slices: call sliced_floor_plan first")
    n = len(plan["slices"])
    small = torch.cat([plan["bounds"].reshape(-1), plan["stats"].reshape(-1), plan["origin"].reshape(-1),
                       plan["counts"].to(torch.float64).reshape(-1), plan["close_size"].to(torch.float64)]).cpu().numpy()
    bounds, stats = small[:3 * n].reshape(n, 3), small[3 * n:11 * n].reshape(n, 8)
    origin, counts, sizes = small[11 * n:13 * n].reshape(n, 2), small[13 * n:15 * n].reshape(n, 2), small[15 * n:16 * n]
    slices = []
    for s, sub in enumerate(plan["slices"]):
        p = floor_polygons_summary(sub)
        slices.append({"index": s, "lo": float(bounds[s, 0]), "hi": float(bounds[s, 1]), "height": float(bounds[s, 2]),
                       "participants": int(stats[s, 0]), "dropped_rows": int(stats[s, 1]), "occupied_cells": int(stats[s, 2]),
                       "status": SLICE_STATUS[int(stats[s, 5])], "grid": [int(stats[s, 3]), int(stats[s, 4])],
                       "origin": [float(origin[s, 0]), float(origin[s, 1])], "set_cells": int(counts[s, 0]),
                       "components": int(counts[s, 1]), "close_size": int(sizes[s]),
                       "region_stats": {k: float(v) for k, v in zip(REGION_STATS, sub["region_stats"].cpu().numpy())},
                       "outline_stats": p["outline_stats"], "polygon_stats": p["polygon_stats"], "polygons": p["polygons"],
                       "dropped": p["dropped"]})
    return {"resolution": plan["parameters"]["resolution"], "parameters": dict(plan["parameters"]), "slices": slices}


def export_sliced_floorplan_text(path: str, summary: dict) -> str:
    """The reference's floor-plan file (`save_floorplan_data`) for all slices, from a `sliced_floor_plan_summary`: the
    five header lines, then one line per kept polygon, `height, n, x1, z1, ...` with three decimals, labelled with its
    slice's mid height, in the reference's coordinates (`vertices_reference`).  Slices in ascending height (the
    reference's sort is stable and the slices arrive in ascending order); within a slice descending label, as
    `export_floorplan_text` and for the same reason.  Written through a temporary file and `os.replace`."""
    lines = ["# Floor Plan Data\n", "# Units: meters\n\n", "# Shapes by height\n",
             "# Format: height, num_points, x1, z1, x2, z2, ...\n"]
    for sl in sorted(summary["slices"], key=lambda q: q["index"]):
        for p in sorted(sl["polygons"], key=lambda q: -q["label"]):
            xy = p["vertices_reference"]
            lines.append(f"{sl['height']:.3f}, {len(xy)}" + "".join(f", {x:.3f}, {z:.3f}" for x, z in xy) + "\n")
    tmp = path + ".tmp"
    with open(tmp, "w") as f:
        f.write("".join(lines))
    os.replace(tmp, path)
    return path


GROUND_JSON = "ground.json"


def save_ground_plane_params(ground_model: Optional[dict], image_path: str, output_dir: Optional[str] = None
                             ) -> Optional[str]:
    """Write the plane as the reference does (:225-263): `ground.json` in `output_dir` (default: the
    image's directory), keys `normal`, `d`, `origin`, `json.dump(..., indent=4)`."""
    if ground_model is None:
        return None
    as_list = lambda v: v.tolist() if isinstance(v, np.ndarray) else v   # noqa: E731
    model = {"normal": as_list(ground_model["normal"]), "d": float(ground_model["d"]),
             "origin": as_list(ground_model["origin"])}
    if output_dir is None:
        output_dir = os.path.dirname(image_path)
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, GROUND_JSON)
    with open(path, "w") as f:
        json.dump(model, f, indent=4)
    return path


def load_ground_plane_params(image_path: str, input_dir: Optional[str] = None) -> Optional[dict]:
    """Read the plane back (:265-312): `ground.json`, else the legacy `{base}_ground_plane.json`;
    None if neither exists or the file cannot be read."""
    if input_dir is None:
        input_dir = os.path.dirname(image_path)
    path = os.path.join(input_dir, GROUND_JSON)
    if not os.path.exists(path):
        base = os.path.splitext(os.path.basename(image_path))[0]
        legacy = os.path.join(input_dir, f"{base}_ground_plane.json")
        if os.path.exists(legacy):
            path = legacy
    if not os.path.exists(path):
        return None
    try:
        with open(path) as f:
            m = json.load(f)
        return {"normal": np.array(m["normal"]), "d": m["d"], "origin": np.array(m["origin"]), "inliers_3d": None}
    except Exception:   # the reference returns None on any read / parse error
        return None


def apply_rotation_to_plane(ground_model: Optional[dict], rotation_offset) -> Optional[dict]:
    """Rotate the plane normal by [rx, ry, rz] degrees (R = Rz Ry Rx) and recompute d through the
    model's origin (:314-373).  Host only."""
    if ground_model is None:
        return None
    rx, ry, rz = np.radians(rotation_offset)
    Rx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
    Ry = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    Rz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
    R = Rz @ Ry @ Rx
    normal = R @ np.asarray(ground_model["normal"])
    normal = normal / np.linalg.norm(normal)
    out = dict(ground_model)
    out["normal"] = normal
    out["d"] = -np.dot(normal, ground_model["origin"])
    return out
