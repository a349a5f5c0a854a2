#!/usr/bin/env python3
"""Drop-in for the reference `generate_depth_maps.py` frame loop, on the MI355X engine.

Same CLI, same functions (`colorize_depth`, `generate_depth_map`,
`batch_generate_depth_maps`), same output names (`{base}_depth.png`) and formats
(turbo-coloured 8-bit RGB PNG over the per-frame depth range, or `--raw`
16-bit grey) as `generate_depth_maps.py:15-251` of the reference.

What changes is the loop: the model is created and packed ONCE
(the reference rebuilds it for every frame, `:76-80`), the forward replays one
HIP graph, frames are decoded by a thread pool ahead of the GPU, only the
uint8 frame crosses PCIe (7 MB at 1536^2 instead of 28 MB fp32), and PNG
encoding runs in writer threads behind the GPU.  Under `torchrun` (one process
per GPU) only rank 0 reads and packs the checkpoint and RCCL-broadcasts the
packed weights; the frame list is sharded k -> rank k mod N and every rank
writes its own frames (`--resume`: rank 0 decides which frames are still
missing, one broadcast before anything is written).  cv2 is not required: PNGs are written with Pillow (pixel-identical
content; the reference's cv2 encoder may choose different zlib settings).
"""

from __future__ import annotations

import argparse
import glob
import inspect
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from functools import partial
from typing import Callable, List, NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_pro  # noqa: E402  (this package's drop-in)
from depth_pro import distributed as D  # noqa: E402
from depth_pro import effects as FX  # noqa: E402
from depth_pro import pointcloud as PC  # noqa: E402
from depth_pro import shadows as SH  # noqa: E402
from depth_pro import render as RV  # noqa: E402
from depth_pro import overlay as OV  # noqa: E402


def colorize_depth(depth, min_depth=None, max_depth=None, cmap="turbo"):
    """Colorize a depth map (reference generate_depth_maps.py:15-44)."""
    import matplotlib.pyplot as plt

    if min_depth is None:
        min_depth = np.nanmin(depth)
    if max_depth is None:
        max_depth = np.nanmax(depth)
    depth_norm = (depth - min_depth) / (max_depth - min_depth)
    depth_norm = np.clip(depth_norm, 0, 1)
    mapper = plt.get_cmap(cmap)
    colored_depth = mapper(depth_norm)[:, :, :3]
    return (colored_depth * 255).astype(np.uint8)


def raw_depth_u16(depth_np: np.ndarray) -> np.ndarray:
    """--raw encoding (reference :135-143)."""
    min_depth = np.nanmin(depth_np)
    max_depth = np.nanmax(depth_np)
    return ((depth_np - min_depth) / (max_depth - min_depth) * 65535).astype(np.uint16)


def _png_parts(arr: np.ndarray, level: int = 1) -> list:
    """The PNG file of an 8-bit RGB (H, W, 3), 16-bit or 8-bit greyscale (H, W) image as a list of byte
    pieces: filter type 0 on every row and one zlib stream (level 1) -- the same pixels as any PNG
    writer (the reference's cv2.imwrite included), ~3x faster than PIL's adaptive filtering.
    zlib (compress, crc32) runs without the GIL and nothing here copies the image or the
    compressed stream with the GIL held, so the loop's writer threads scale."""
    import struct
    import zlib

    if arr.dtype == np.uint16 and arr.ndim == 2:
        depth, ctype, rows = 16, 0, arr.astype(">u2").view(np.uint8).reshape(arr.shape[0], -1)
    elif arr.dtype == np.uint8 and arr.ndim == 3 and arr.shape[2] == 3:
        depth, ctype, rows = 8, 2, arr.reshape(arr.shape[0], -1)
    elif arr.dtype == np.uint8 and arr.ndim == 2:
        depth, ctype, rows = 8, 0, arr
    else:
        raise ValueError(f"_png_bytes: unsupported image {arr.dtype} {arr.shape}")
    h, w = arr.shape[0], arr.shape[1]
    raw = np.empty((h, rows.shape[1] + 1), np.uint8)
    raw[:, 0] = 0
    raw[:, 1:] = rows

    def chunk(tag: bytes, data) -> list:
        crc = zlib.crc32(data, zlib.crc32(tag)) & 0xFFFFFFFF
        return [struct.pack(">I", len(data)), tag, data, struct.pack(">I", crc)]

    ihdr = struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0)
    idat = zlib.compress(memoryview(raw).cast("B"), level)
    return [b"\x89PNG\r\n\x1a\n", *chunk(b"IHDR", ihdr), *chunk(b"IDAT", idat), *chunk(b"IEND", b"")]


def _png_bytes(arr: np.ndarray, level: int = 1) -> bytes:
    """PNG file bytes of an 8-bit RGB (H, W, 3) or 16-bit greyscale (H, W) image (`_png_parts`)."""
    return b"".join(_png_parts(arr, level))


def _write_png(path: str, arr: np.ndarray) -> None:
    with open(path, "wb") as f:
        for part in _png_parts(np.ascontiguousarray(arr)):
            f.write(part)


_MODEL = {}


def _dist() -> Tuple[int, int]:
    """(world, rank).  Under torchrun (WORLD_SIZE > 1) the process group is created here if the
    caller has not: RCCL ("nccl") on the ROCm device, gloo otherwise."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return 1, 0
    if not dist.is_initialized():
        if torch.cuda.is_available():
            dev = _device()
            torch.cuda.set_device(dev)
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")
    return dist.get_world_size(), dist.get_rank()


def _model(device: torch.device, half_precision: bool):
    """One model per (device, precision) per process (the reference reloads it per frame, :76-80).
    In a process group only rank 0 reads and packs the checkpoint; the others receive the packed
    weights over RCCL (distributed.create_model_and_transforms_shared)."""
    key = (str(device), bool(half_precision))
    if key not in _MODEL:
        precision = torch.float16 if half_precision else torch.float32
        cfg = depth_pro.depth_pro.run_config()       # DEPTH_PRO_SYNTHETIC=1: synthetic weights if no checkpoint
        world, _ = _dist()
        if world > 1:
            model, transform = D.create_model_and_transforms_shared(cfg, device, precision)
        else:
            model, transform = depth_pro.create_model_and_transforms(cfg, device=device, precision=precision)
        model.eval()
        model.use_hip_graph(True)
        _MODEL[key] = (model, transform)
    return _MODEL[key]


def _device() -> torch.device:
    if torch.cuda.is_available():
        return torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    raise RuntimeError("the MI355X Depth Pro engine needs a ROCm GPU")


def _load(image_path: str, downscale_factor: float):
    """Decode (host thread): the frame and its EXIF focal length, scaled by --downscale_factor as
    the reference does (:108-110); the resize itself runs on the GPU (`_downscale`)."""
    image, _, f_px = depth_pro.load_rgb(image_path)
    if downscale_factor != 1.0 and downscale_factor > 0 and f_px is not None:
        f_px = f_px * downscale_factor
    if torch.cuda.is_available():
        # into pinned host memory here, in the decode thread: the upload is then an asynchronous
        # copy on the frame's stream, so the main thread queues frame i+1 while frame i computes
        # (a pageable upload blocks the host until the GPU has finished every earlier frame)
        image = torch.from_numpy(np.ascontiguousarray(image)).pin_memory()
    return image, f_px


def _downscale(image: np.ndarray, downscale_factor: float, device: torch.device):
    """The reference's cv2.resize (:95-107: new size int(H * f) x int(W * f), INTER_AREA for f < 1,
    INTER_LINEAR otherwise) on the GPU (dp_resize_u8_cv): uint8 upload, uint8 frame on the device.
    Without a factor the host frame is returned as is (the transform uploads it)."""
    if downscale_factor == 1.0 or downscale_factor <= 0:
        return image
    from depth_pro import ops

    h, w = image.shape[:2]
    src = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image))
    src = src.to(device, non_blocking=True)
    return ops.resize_u8_cv(src, int(h * downscale_factor), int(w * downscale_factor), area=downscale_factor < 1.0)


def _encode(depth_np: np.ndarray, output_path: str, colored: bool, cmap: str) -> str:
    if colored:
        _write_png(output_path, colorize_depth(depth_np, cmap=cmap))
    else:
        _write_png(output_path, raw_depth_u16(depth_np))
    return output_path


def _pinned(t: torch.Tensor) -> torch.Tensor:
    """A pinned host copy of a device tensor, queued on the current stream (no host sync)."""
    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    host.copy_(t, non_blocking=True)
    return host


def _image_async(depth: torch.Tensor, colored: bool, cmap: str) -> torch.Tensor:
    """The PNG content of a device depth map, made on the GPU (dp_depth_to_image: colorize_depth /
    --raw, byte-identical) and queued into pinned host memory on the current stream (no host
    sync): the writer thread only PNG-encodes it after the frame's event."""
    from depth_pro import ops

    return _pinned(ops.depth_to_image(depth.contiguous(), colored=colored, cmap=cmap))


def _host_image(host: torch.Tensor) -> np.ndarray:
    a = host.numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def generate_depth_map(image_path, output_path=None, downscale_factor=1.0, half_precision=False, colored=True,
                       cmap="turbo"):
    """One frame (reference :46-151); returns the output path or None on error."""
    try:
        if output_path is None:
            output_path = output_name(image_path)
        model, transform = _model(_device(), half_precision)
        image, f_px = _load(image_path, downscale_factor)
        image = _downscale(image, downscale_factor, _device())
        with torch.no_grad():
            depth = model.infer(transform(image), f_px=f_px)["depth"]
        model.last_status().check()
        if depth.is_cuda:
            host = _image_async(depth, colored, cmap)
            torch.cuda.current_stream(depth.device).synchronize()
            _write_png(output_path, _host_image(host))
            return output_path
        return _encode(depth.detach().cpu().numpy(), output_path, colored, cmap)
    except Exception as e:  # reference :147-151: report and skip the frame
        print(f"Error generating depth map for {image_path}: {str(e)}")
        import traceback

        traceback.print_exc()
        return None


def frame_file(image_path: str, suffix: str) -> str:
    """`{base}{suffix}`: the name of one of a frame's files, from its image path."""
    return os.path.splitext(os.path.basename(image_path))[0] + suffix


# the public names of a frame's files, from its image path
output_name = partial(frame_file, suffix="_depth.png")                  # reference :187-188
clusters_name = partial(frame_file, suffix="_clusters.json")            # --cluster_pointcloud; the labels go beside it
labels_name = partial(frame_file, suffix="_labels.npy")
shapes_name = partial(frame_file, suffix="_shapes.json")                # --fit_shapes; `{base}_shapes.txt` goes beside it
oriented_name = partial(frame_file, suffix="_oriented.ply")             # --mesh_points; parameters and statistics beside it
oriented_json_name = partial(frame_file, suffix="_oriented.json")
floorplan_name = partial(frame_file, suffix="_floorplan.png")           # --floor_plan; origin, statistics, regions beside it
floorplan_json_name = partial(frame_file, suffix="_floorplan.json")
boundary_name = partial(frame_file, suffix="_boundary.json")            # --boundary_dir: the score against `{base}.npy` there
anaglyph_name = partial(frame_file, suffix="_anaglyph.png")             # --anaglyph
parallax_name = partial(frame_file, suffix="_parallax.png")             # --parallax
shadows_name = partial(frame_file, suffix="_shadows.png")               # --depth_shadows; parameters and counts beside it
shadows_json_name = partial(frame_file, suffix="_shadows.json")
view_name = partial(frame_file, suffix="_view.png")                     # --render_view; cameras and counts beside it
view_json_name = partial(frame_file, suffix="_view.json")
plan_name = partial(frame_file, suffix="_plan.png")                     # --plan_shapes; parameters, camera and counts beside it
plan_json_name = partial(frame_file, suffix="_plan.json")


def cloud_name(image_path: str, cleaned: bool = False) -> str:
    """`{base}_points.ply`, or `{base}_clean.ply` (the reference cleaner's file name) with --clean_pointcloud."""
    return frame_file(image_path, "_clean.ply" if cleaned else "_points.ply")


def boundary_target_path(image_path: str, boundary_dir: str) -> str:
    return os.path.join(boundary_dir, frame_file(image_path, ".npy"))


def plan_frames(image_paths, output_dir: str, world: int, rank: int, resume: bool, cleaned: bool = False,
                clustered: bool = False, shaped: bool = False, oriented: bool = False, floor: bool = False,
                boundary: Optional[str] = None, stages=(), meshed: bool = False) -> List[int]:
    """Indices of the frames this rank processes: the frames still to do (all of them, or with
    `resume` those with an output file missing -- decided by rank 0 alone and broadcast before
    any rank writes, so every rank shards the same list), dealt round-robin over the ranks.
    Missing: a frame without its `{base}_depth.png`, or without a file that a stage which is on requires
    (`Stage.suffixes`).  On are the stages named in `stages`, and `cleaned` (--clean_pointcloud), `clustered`
    (--cluster_pointcloud), `shaped` (--fit_shapes), `oriented` (--mesh_points), `meshed` (--simple_mesh), `floor`
    (--floor_plan), `boundary` (--boundary_dir: only a frame with a target `{base}.npy` in that directory needs its `{base}_boundary.json`)."""
    todo = list(range(len(image_paths)))
    if resume:
        if rank == 0:
            on = set(stages) | {name for name, flag in (("clean", cleaned), ("cluster", clustered), ("shapes", shaped),
                                                        ("mesh", oriented), ("trimesh", meshed), ("floor", floor),
                                                        ("boundary", boundary)) if flag}
            need = ["_depth.png"] + [s for st in STAGES if st.name in on and st.name != "boundary" for s in st.suffixes]

            def done(k):
                have = lambda s: os.path.exists(os.path.join(output_dir, frame_file(image_paths[k], s)))   # noqa: E731
                return all(have(s) for s in need) and (
                    not boundary or not os.path.exists(boundary_target_path(image_paths[k], boundary)) or have("_boundary.json"))
            todo = [k for k in todo if not done(k)]
        if world > 1:
            box = [todo]
            dist.broadcast_object_list(box, src=0)
            todo = box[0]
    return [todo[i] for i in D.shard_frames(len(todo), rank, world)]


def _stages_on(o: dict) -> set:
    """The names of the stages that are on for the options `o` (all of them present): asked for, or implied."""
    on = set()
    for st in reversed(STAGES):             # a stage stands behind every stage it implies
        if st.name in on or st.on(o):
            on |= {st.name, st.implies} - {None}
    return on


def resolve_stages(**options) -> dict:
    """The stages a run has on, from the loop's options (`batch_generate_depth_maps`'s keywords; one left out has
    its default): {stage name: its parameter dict}, in the order of `STAGES`.  A stage is on when its own option is,
    or when a stage that is on implies it; the options of the stages that are on are checked (ValueError), the
    others are not looked at.  Touches no GPU and no file (but `check_boundary_dir`'s isdir)."""
    o = {**_DEFAULTS, **options}
    on = _stages_on(o)
    params = {st.name: st.params(o) for st in reversed(STAGES) if st.name in on}
    return {st.name: params[st.name] for st in STAGES if st.name in on}


def batch_generate_depth_maps(input_dir, output_dir, pattern="*.png", downscale_factor=1.0, half_precision=False,
                              colored=True, cmap="turbo", decode_workers=4, encode_workers=None, pointcloud=False,
                              resume=False, model=None, normalize_ground=False, ground_params_dir=None, grid_size=20,
                              ground_percentile=5, rotation_offset=None, clean_pointcloud=False, stray_radius=0.1,
                              stray_neighbors=20, cluster_pointcloud=False, cluster_eps=0.2, cluster_min_samples=5,
                              cluster_height=1.3, cluster_max_points=100000, fit_shapes=False,
                              circularity_threshold=0.85, mesh_points=False, voxel_size=0.05, normals_max_nn=30,
                              floor_plan=False, floor_resolution=0.1, floor_height=1.3, floor_min_area=0.025,
                              boundary_dir=None, split_l_shapes=False, simple_mesh=False, mesh_neighbors=6,
                              floor_polygons=False, floor_slices=0, floor_slice_min=0.1, floor_slice_max=2.5,
                              floor_slice_resolution=0.05, floor_slice_min_area=0.1, anaglyph=False,
                              anaglyph_separation=0.05, parallax=None, parallax_amplitude=0.05, parallax_period=150,
                              depth_shadows=False, shadow_threshold=0.2, shadow_min_region=100, drop_depth_shadows=False,
                              render_view=None, render_size="1280x720", render_point_size=7, render_min_height=None,
                              plan_shapes=False, plan_size="1280x720", plan_point_size=7, plan_stroke=3.0, plan_label_scale=2):
    """Directory loop (reference :153-206), pipelined decode -> GPU -> encode, frame-sharded across ranks.

    Every rank writes its own frames' files; each frame has exactly one owner.  resume=True skips
    frames whose `{base}_depth.png` already exists (checkpoint/resume row) and, with a stage on,
    that stage's files too.  `model`: an already-built (model, transform) pair (tests); default: `_model`.
    Returns the number of frames this rank wrote.  The stages (`STAGES`), each queued on the frame's stream
    like every other output; without a stage the loop writes exactly what it wrote before:
    pointcloud=True also writes `{base}_points.ply` per frame: the reference's depth_to_3d
    back-projection with the frame's focal length (EXIF, or the FOV head's) and RGB colours
    (SURVEY 8f).
    normalize_ground=True (implies pointcloud) levels that cloud first, as the
    reference's img_to_normalized_pointcloud.py does per image (:1228-1287): ground plane at y = 0
    (`PC.normalize_to_ground`), then the per-cell adjustment (`PC.ground_adjust` with grid_size /
    ground_percentile); same point order and colours, same writer path.  Video semantics (ours): the
    plane is read from `ground.json` in ground_params_dir (default: output_dir) if present, else
    fitted on the first frame this run processes (`PC.fit_ground_plane`, rank 0 under torchrun, which
    broadcasts it) and saved there; it is then reused for every frame, so a fixed camera does not get
    a jittering floor.  rotation_offset ([rx, ry, rz] degrees, `PC.apply_rotation_to_plane`) is
    applied to the plane in use, not to the saved file, so a re-run does not rotate twice.
    clean_pointcloud=True (implies normalize_ground) then cleans the levelled cloud on the GPU as the
    reference pipeline's next step does (`PC.clean_pointcloud`: remove_stray_points with stray_neighbors /
    stray_radius, then clean_shadows) and writes `{base}_clean.ply` in place of `{base}_points.ply`.
    cluster_pointcloud=True (implies clean_pointcloud) clusters the cleaned cloud's top-down projection as
    the reference's floor-plan step does (`PC.cluster_pointcloud`: DBSCAN with cluster_eps /
    cluster_min_samples over the points with y >= cluster_height -- NaN: every height --, thinned to
    cluster_max_points, 0 = all) and writes `{base}_clusters.json` (parameters, counts, per-cluster count,
    bounding box, centroid, smallest core row) and `{base}_labels.npy` (int32, in the row order of
    `{base}_clean.ply`) beside the cloud.
    fit_shapes=True (implies cluster_pointcloud) fits each cluster's convex hull, minimum-area rectangle
    and circle right after the cluster table (`PC.fit_shapes`, with the reference's
    circle-or-rectangle decision at circularity_threshold) and writes `{base}_shapes.json`
    (`PC.shape_summary`) and `{base}_shapes.txt` (the reference's `export_shape_data` layout).
    split_l_shapes=True (implies fit_shapes) queues the reference's `detect_and_split_l_shapes` behind the
    shapes (`PC.rectangle_list`, `PC.split_l_shapes`); both files then list the rectangles after the split.
    floor_plan=True (implies clean_pointcloud) makes the reference's occupancy floor plan of the cleaned cloud
    (`PC.floor_plan`: the rows with y >= floor_height -- NaN: every height -- rasterised at floor_resolution, closing
    7 x 7 twice, opening 3 x 3, 8-connected regions, regions of at least floor_min_area m^2 drawn)
    and writes `{base}_floorplan.png` (RGB, row 0 = smallest z) and `{base}_floorplan.json` (origin, resolution, size,
    parameters, statistics, one object per drawn region).
    mesh_points=True (implies clean_pointcloud) turns the cleaned cloud into the oriented point set every meshing
    method of the reference's pointcloud_to_mesh.py starts from (`PC.oriented_points`: voxel grid of voxel_size,
    normals over radius 2 * voxel_size and at most normals_max_nn neighbours, oriented towards the origin)
    and writes `{base}_oriented.ply` (double x y z nx ny nz + uchar rgb) and `{base}_oriented.json`
    (parameters, point count, both statistics).
    floor_polygons=True (implies floor_plan) traces the outline of every region of that plan, simplifies it as the
    reference's `approximate_contour` does (`PC.floor_polygons`) and writes the reference's polygons file
    `{base}_floorplan.txt` (`PC.export_floorplan_text`) and `{base}_floorplan_polygons.json` (every polygon in grid
    units and in both world coordinates, flags, areas, and why a region has none).
    floor_slices=N (N > 0; implies clean_pointcloud) makes the reference's default floor plan, the one without a height
    threshold (`PC.sliced_floor_plan`): N height slices between floor_slice_min and floor_slice_max, each rasterised at
    floor_slice_resolution, closed once with the size its raw grid asks for, opened 3 x 3, outlined and simplified with
    alpha 0.01 and floor_slice_min_area undivided; writes `{base}_floorslices.txt` (the reference's polygons file, every
    polygon labelled with its slice's mid height) and `{base}_floorslices.json` (per slice: bounds, counts, status, grid,
    closing size, polygons).
    simple_mesh=True (implies mesh_points) meshes those voxels as the reference's `--mesh_method simple` does
    (`PC.triangulate`: every voxel's mesh_neighbors nearest others, the fan of triangles over them, degenerate and
    duplicated triangles removed) and writes `{base}_mesh.ply` (the vertices of `{base}_oriented.ply` without normals,
    then `element face`) and `{base}_mesh.json` (parameters, counts, both statistics, the mean distance to the 20
    nearest voxels and the reference's four ball-pivoting radii).
    boundary_dir=DIR scores each frame whose target `DIR/{base}.npy` exists and has the depth's shape with the Depth Pro
    boundary metric (`depth_pro.eval.boundary_metrics`), from the device depth before its read-back:
    a float32 target is a depth (SI_boundary_F1), a bool or uint8 one a mask (SI_boundary_Recall, the raw values
    thresholded by > 0.1).  `{base}_boundary.json` holds the kind, the score, the per-threshold counts, the thresholds,
    H and W; a missing or unusable target is reported and the frame goes on without a score; rank 0 prints the mean.
    anaglyph=True writes `{base}_anaglyph.png`, the reference's red-cyan anaglyph (OLD_SCRIPTS/depth_video_effect.py
    :113-183) of the frame and its depth, both still on the device (`depth_pro.effects.anaglyph`, anaglyph_separation
    as the reference's --separation), as RGB.
    parallax="circle" | "zoom" | "swing" writes `{base}_parallax.png`, one frame of the reference's parallax video
    (:10-111, `depth_pro.effects.warp_views`) with parallax_amplitude, at phase (the frame's position in the sorted
    list of all frames) mod parallax_period of a parallax_period-frame cycle (150: the reference's 5 s x 30 fps): a
    directory of parallax_period copies of one still reproduces the reference's video frame by frame, a real video
    gets the camera motion laid over it; the phase does not depend on how the frames are dealt to the ranks.
    Both report, in one line per frame, the pixels written black for want of a finite depth when there are any.
    depth_shadows=True writes `{base}_shadows.png` (8-bit grey, 255 = shadow) and `{base}_shadows.json` (parameters, counts
    by name, gmax, nonfinite): the reference's find_depth_shadows (OLD_SCRIPTS/mesh_from_depth.py :1110-1170) of the depth
    still on the device (`depth_pro.shadows.find_depth_shadows` with shadow_threshold as its threshold_factor and
    shadow_min_region as its min_region_size), queued ahead of the cloud.
    drop_depth_shadows=True (implies depth_shadows; needs the cloud: pointcloud or a stage that implies it, else
    ValueError) back-projects the depth with the shadow pixels set to NaN, so the cloud and every later stage are without
    them.  This use of the mask is this project's own: the reference fills the shadow pixels and never drops them.
    render_view="front" | "top" | "side" | "isometric" | "multi" | "plan" (implies pointcloud) writes `{base}_view.png`, a
    picture of the frame's latest cloud (the cleaned one with clean_pointcloud, the levelled one with normalize_ground,
    else the raw one) made on the device (`depth_pro.render.render_views`: the reference's view presets, `multi` their
    2 x 2 sheet, `plan` the main pipeline's top-down picture, render_min_height its height threshold) at render_size
    ("WxH") with splats of render_point_size pixels, and `{base}_view.json` (the cameras and the counts).
    plan_shapes=True (implies fit_shapes) writes `{base}_plan.png`, the reference's main picture (pointcloud_pipeline.py's
    in_memory_pointcloud_visualization): the top-down plan of the cleaned cloud's rows at or above cluster_height, with the
    fitted rectangles (after the split with split_l_shapes) and circles stroked on it and numbered, all made on the device
    (`depth_pro.overlay.plan_with_shapes`) at plan_size ("WxH") with splats of plan_point_size pixels, strokes plan_stroke
    pixels wide and digits of plan_label_scale pixels per font pixel (0: no numbers), and `{base}_plan.json` (parameters,
    the camera record, the counts).
    """
    params = resolve_stages(**{k: v for k, v in locals().items() if k in _DEFAULTS}, output_dir=output_dir)
    on = [st for st in STAGES if st.name in params]
    os.makedirs(output_dir, exist_ok=True)
    image_paths = sorted(glob.glob(os.path.join(input_dir, pattern)))
    if not image_paths:
        print(f"No images found matching pattern {os.path.join(input_dir, pattern)}")
        return 0
    world, rank = _dist()
    mine = plan_frames(image_paths, output_dir, world, rank, resume, boundary=boundary_dir, stages=params)
    print(f"[rank {rank}/{world}] Found {len(image_paths)} images, processing {len(mine)}")
    if model is None:
        model = _model(_device(), half_precision)
    model, transform = model
    if encode_workers is None:   # PNG (+ PLY) writing is the host side's long pole: zlib drops the GIL
        encode_workers = max(4, min(8, len(os.sched_getaffinity(0)) // 2))

    successful = 0
    t0 = time.time()
    # frames queued to the writers but not written yet (each holds pinned host copies of its
    # depth map and, with --pointcloud, its points): at most this many, so host memory stays
    # bounded when PNG / PLY writing falls behind the GPU
    max_inflight = 2 * encode_workers

    def collect(f):
        nonlocal successful
        try:
            if f is not None and f.result() is not None:
                successful += 1
        except Exception as e:  # a bad frame or a write failure skips that frame, like the reference
            print(f"Error writing a depth map: {e}")

    with ThreadPoolExecutor(decode_workers) as dec, ThreadPoolExecutor(encode_workers) as enc:
        futs = {k: dec.submit(_load, image_paths[k], downscale_factor) for k in mine[: 2 * decode_workers]}
        nxt = 2 * decode_workers
        pending = []
        for n, k in enumerate(mine):
            base = os.path.join(output_dir, frame_file(image_paths[k], ""))
            while len(pending) >= max_inflight:
                collect(pending.pop(0))
            try:
                image, f_px = futs.pop(k).result()
                if nxt < len(mine):
                    futs[mine[nxt]] = dec.submit(_load, image_paths[mine[nxt]], downscale_factor)
                    nxt += 1
                if downscale_factor != 1.0 and downscale_factor > 0:
                    image = _downscale(image, downscale_factor, getattr(transform, "device", None) or _device())
                with torch.no_grad():
                    pred = model.infer(transform(image), f_px=f_px)
                    depth = pred["depth"]
                # this frame's health (engine.FrameStatus: a timed-out stream-K hand-off, NaN / inf
                # output), checked by the writer after the frame's event, before any file is written;
                # claimed, so the next infer's sweep of finished frames leaves it to that writer (a
                # bad frame is dropped once, by its writer, never the next frame in its place)
                status = model.last_status() if hasattr(model, "last_status") else None
                if status is not None and hasattr(status, "claim"):
                    status.claim()
                out = {}                    # what the writer gets: {stage name: its payload}
                if depth.is_cuda:
                    # the PNG content (colour / raw) made on the GPU, and every device->host copy,
                    # queued behind the frame on this stream; a writer thread waits on its event
                    host = _image_async(depth, colored, cmap)
                    if list(params) == ["cloud"]:           # the base cloud alone is one step (tools swap it)
                        out["cloud"] = _points(depth, pred["focallength_px"], image)
                    else:
                        frame = {"depth": depth, "f_px": pred["focallength_px"], "image": image, "path": image_paths[k],
                                 "world": world, "rank": rank, "index": k}
                        for st in on:
                            out[st.name] = st.queue(frame, params[st.name])
                        if "cloud" in params:                 # the records of the cloud as the stages have left it
                            out["cloud"] = _records(frame)
                    ev = torch.cuda.Event()
                    ev.record()
                else:
                    host, ev = depth, None

                def _finish(host=host, ev=ev, base=base, out=out, status=status):
                    if ev is not None:
                        ev.synchronize()
                    if status is not None:
                        status.check()          # raises: this frame is dropped, nothing written
                    for st in on:
                        if st.write is not None and out.get(st.name) is not None:
                            st.write(base, params, out)
                    if ev is not None:              # the PNG content was made on the GPU
                        _write_png(base + "_depth.png", _host_image(host))
                        return base + "_depth.png"
                    return _encode(host.numpy(), base + "_depth.png", colored, cmap)

                pending.append(enc.submit(_finish))
            except Exception as e:
                print(f"Error generating depth map for {image_paths[k]}: {str(e)}")
                pending.append(None)
            print(f"[{n + 1}/{len(mine)}] Processing {frame_file(image_paths[k], '')}")
        for f in pending:
            collect(f)
    for st in on:
        if st.end is not None:
            st.end(params[st.name], world, rank)
    dt = time.time() - t0
    print(f"Processing complete: {successful}/{len(mine)} images successfully processed "
          f"({len(mine) / max(dt, 1e-9):.2f} frames/s on rank {rank})")
    return successful


MAX_GRID_SIZE = PC.MAX_GRID


def check_grid_size(grid_size) -> None:
    if not 1 <= int(grid_size) <= MAX_GRID_SIZE:
        raise ValueError(f"--grid_size must be in [1, {MAX_GRID_SIZE}] (got {grid_size})")


def check_stray(radius, neighbors) -> None:
    if not (np.isfinite(float(radius)) and float(radius) > 0):
        raise ValueError(f"--stray_radius must be finite and > 0 (got {radius})")
    if int(neighbors) < 1:
        raise ValueError(f"--stray_neighbors must be >= 1 (got {neighbors})")


def check_cluster(eps, min_samples, max_points) -> None:
    if not (np.isfinite(float(eps)) and float(eps) > 0):
        raise ValueError(f"--cluster_eps must be finite and > 0 (got {eps})")
    if int(min_samples) < 1:
        raise ValueError(f"--cluster_min_samples must be >= 1 (got {min_samples})")
    if int(max_points) < 0:
        raise ValueError(f"--cluster_max_points must be >= 0 (got {max_points})")


def check_circularity(threshold) -> None:
    if np.isnan(float(threshold)):
        raise ValueError("--circularity_threshold must not be nan")


def check_mesh(voxel_size, max_nn) -> None:
    if not (np.isfinite(float(voxel_size)) and float(voxel_size) > 0):
        raise ValueError(f"--voxel_size must be finite and > 0 (got {voxel_size})")
    if not 1 <= int(max_nn) <= PC.MAX_NN:
        raise ValueError(f"--normals_max_nn must be in [1, {PC.MAX_NN}] (got {max_nn})")


def check_mesh_neighbors(neighbors) -> None:
    if not 2 <= int(neighbors) <= PC.MAX_K:
        raise ValueError(f"--mesh_neighbors must be in [2, {PC.MAX_K}] (got {neighbors})")


def check_floor(resolution, height, min_area) -> None:
    if not (np.isfinite(float(resolution)) and float(resolution) > 0):
        raise ValueError(f"--floor_resolution must be finite and > 0 (got {resolution})")
    if np.isinf(float(height)):
        raise ValueError(f"--floor_height must be finite, or nan for every height (got {height})")
    if not (np.isfinite(float(min_area)) and float(min_area) >= 0):
        raise ValueError(f"--floor_min_area must be finite and >= 0 (got {min_area})")


def check_floor_slices(num_slices, height_min, height_max, resolution, min_area) -> None:
    if not 1 <= int(num_slices) <= PC.SLICE_MAX:
        raise ValueError(f"--floor_slices must be in [1, {PC.SLICE_MAX}] (got {num_slices})")
    if not (np.isfinite(float(height_min)) and np.isfinite(float(height_max)) and float(height_max) > float(height_min)):
        raise ValueError(f"--floor_slice_min and --floor_slice_max must be finite with max > min (got {height_min}, {height_max})")
    if not (np.isfinite(float(resolution)) and float(resolution) > 0):
        raise ValueError(f"--floor_slice_resolution must be finite and > 0 (got {resolution})")
    if not (np.isfinite(float(min_area)) and float(min_area) >= 0):
        raise ValueError(f"--floor_slice_min_area must be finite and >= 0 (got {min_area})")


def check_boundary_dir(boundary_dir) -> None:
    if not os.path.isdir(str(boundary_dir)):
        raise ValueError(f"--boundary_dir must be an existing directory (got {boundary_dir})")


MAX_CLUSTERS = 4096     # rows of the per-frame cluster table (a frame with more lists the first 4096)


def _ground_plane(ground: dict, xyz, count, image_path):
    """The plane every frame of this run is levelled with, resolved once per rank: rank 0 loads
    `ground.json` or fits the frame at hand (two small read-backs) and saves it; with several ranks it
    then broadcasts normal, d and origin through the process group -- exactly one collective per rank
    and run, whatever the outcome (a rank without frames, or rank 0 without a plane, takes part with
    "no plane", and every later frame of the other ranks fails on that remembered outcome without
    another collective).  The rotation offset is applied last."""
    if ground["resolved"]:
        return ground["model"]
    model = None
    if ground["rank"] == 0:
        model = PC.load_ground_plane_params(image_path or os.path.join(ground["dir"], "frame"), ground["dir"])
        if model is None and xyz is not None:
            try:
                model = PC.fit_ground_plane(xyz, count, ground["grid"])
                PC.save_ground_plane_params(model, image_path, ground["dir"])
            except Exception as e:      # the other ranks must still get their broadcast
                print(f"Ground plane fit failed: {e}")
    if ground["world"] > 1:
        on_gpu = dist.get_backend() == "nccl"
        box = torch.zeros(8, dtype=torch.float64, device=(xyz.device if xyz is not None else _device()) if on_gpu
                          else "cpu")
        if model is not None:
            box[:7] = torch.from_numpy(np.concatenate([model["normal"], [model["d"]], model["origin"]]))
            box[7] = 1.0
        dist.broadcast(box, src=0)
        v = box.cpu().numpy()
        model = {"normal": v[:3].copy(), "d": float(v[3]), "origin": v[4:7].copy()} if v[7] else None
    if model is not None and ground["rot"] is not None and any(float(r) != 0.0 for r in ground["rot"]):
        model = PC.apply_rotation_to_plane(model, ground["rot"])
    ground["model"] = model
    ground["resolved"] = model is not None or ground["world"] > 1   # alone, the next frame may still fit one
    return model


def _backproject(frame: dict, p=None) -> None:
    """Queue the frame's point cloud on the GPU (depth_to_3d, img_to_normalized_pointcloud.py:819-856) on the
    current stream, without a host synchronisation: points, colours and the point count, all on the device."""
    depth, image = frame.get("cloud_depth", frame["depth"]), frame["image"]     # --drop_depth_shadows: shadows are NaN
    h, w = depth.shape
    rgb = image.to(depth.device, non_blocking=True) if torch.is_tensor(image) else \
        torch.from_numpy(np.ascontiguousarray(image)).to(depth.device, non_blocking=True)
    frame["xyz"], _, frame["cols"], frame["count"] = PC.depth_to_points_async(depth, frame["f_px"], w, h, rgb=rgb)


def _records(frame: dict) -> dict:
    """Queue the cloud's PLY vertex records, interleaved on the GPU, and their copy into a pinned host buffer: the
    full-size record buffer + the point count (the writer slices it after the frame's event and writes it as it is)."""
    return {"records": _pinned(PC.ply_records_async(frame["xyz"], frame["cols"])), "count": _pinned(frame["count"])}


def _points(depth: torch.Tensor, f_px, image) -> dict:
    """The base cloud step, all there is to a plain --pointcloud frame: back-projection, records and count."""
    frame = {"depth": depth, "f_px": f_px, "image": image}
    _backproject(frame)
    return _records(frame)


def _points_host(pc):
    """Writer-thread side (after the frame's event): exactly the valid points' records."""
    return pc["records"][:int(pc["count"])].numpy()


# ---- the stages: what each queues on the frame's stream (`frame`: depth, image and the cloud as the stages so far have
# left it, plus what one leaves on the device for a later one) and writes in the writer thread (`out`: {stage: payload}) ----

def _write_cloud(base: str, params: dict, out: dict) -> None:
    PC.write_ply_records(base + ("_clean.ply" if "clean" in params else "_points.ply"), _points_host(out["cloud"]))


def _queue_ground(frame: dict, p: dict) -> None:
    """The levelled cloud (--normalize_ground): no sync once the plane is known (its fit reads back a few dozen doubles)."""
    p.update(world=frame["world"], rank=frame["rank"])
    plane = _ground_plane(p, frame["xyz"], frame["count"], frame["path"])
    if plane is None:
        raise RuntimeError("no ground plane (rank 0 could neither load nor fit one)")
    xyz, _ = PC.normalize_to_ground(frame["xyz"], plane, frame["count"])
    frame["xyz"], _ = PC.ground_adjust(xyz, p["grid"], p["pct"], frame["count"])


def _end_ground(p: dict, world: int, rank: int) -> None:
    if world > 1 and not p["resolved"]:
        p.update(world=world, rank=rank)
        _ground_plane(p, None, None, None)      # a rank without frames still takes part in the broadcast


def _queue_clean(frame: dict, p: dict) -> None:
    """The cleaned cloud (--clean_pointcloud): stray points, then shadow columns; the count stays on the device."""
    frame["xyz"], frame["cols"], count = PC.clean_pointcloud(frame["xyz"], frame["cols"], frame["count"],
                                                             nb_points=p["nb"], radius=p["radius"])[:3]
    frame["count"] = count.reshape(())


def _queue_cluster(frame: dict, p: dict) -> dict:
    """Clusters of the cleaned cloud (--cluster_pointcloud): labels, table and counts, no sync."""
    labels, ncl, stats, table, order, offsets = PC.cluster_pointcloud(frame["xyz"], frame["count"], max_clusters=MAX_CLUSTERS, **p)
    frame.update(labels=labels, n_clusters=ncl, order=order, offsets=offsets)
    return {"labels": _pinned(labels), "n_clusters": _pinned(ncl), "stats": _pinned(stats), "table": _pinned(table)}


def _write_clusters(base: str, params: dict, out: dict) -> None:
    """Writer-thread side: `{base}_labels.npy` (the live rows' labels) and `{base}_clusters.json`."""
    c = out["cluster"]
    np.save(base + "_labels.npy", c["labels"][:int(out["cloud"]["count"])].numpy())
    k = min(int(c["n_clusters"]), MAX_CLUSTERS)
    with open(base + "_clusters.json", "w") as f:
        p = {key: (None if isinstance(v, float) and v != v else v) for key, v in params["cluster"].items()}   # NaN height
        json.dump(PC.cluster_summary(c["table"][:k].numpy(), c["stats"].numpy(), p), f, indent=1)


def _queue_shapes(frame: dict, p: dict) -> dict:
    """The clusters' shapes (--fit_shapes), right behind the table, and with --split_l_shapes the reference's
    detect_and_split_l_shapes behind them (rectangle list, split); only the small tables go to the host."""
    table = PC.fit_shapes(frame["xyz"], frame["order"], frame["offsets"], frame["n_clusters"], frame["count"], MAX_CLUSTERS,
                          p["circularity_threshold"])[0]
    payload = {"table": _pinned(table)}
    if p.get("l_split"):
        rects, n_rects = PC.rectangle_list(table, frame["n_clusters"], MAX_CLUSTERS)
        rows, n_out, info = PC.split_l_shapes(frame["xyz"], frame["labels"], rects, n_rects, frame["count"])
        payload["l_split"] = {"rows": _pinned(rows), "n_out": _pinned(n_out), "info": _pinned(info), "n_rects": _pinned(n_rects)}
        if p.get("plan"):
            frame.update(rects=rows, n_rects=n_out)     # on the device, for the plan picture
    if p.get("plan"):
        frame["shapes"] = table
    return payload


def _write_shapes(base: str, params: dict, out: dict) -> None:
    """Writer-thread side: `{base}_shapes.json` and `{base}_shapes.txt`."""
    s, split = out["shapes"], out["shapes"].get("l_split")
    table = s["table"][:min(int(out["cluster"]["n_clusters"]), MAX_CLUSTERS)].numpy()
    p = {key: (None if isinstance(v, float) and v != v else v) for key, v in {**params["cluster"], **params["shapes"]}.items()
         if key not in ("l_split", "plan")}
    if split is not None:
        summary = PC.shape_summary(table, p, split["rows"][:int(split["n_out"][0])].numpy(),
                                   split["info"][:int(split["n_rects"])].numpy())
        summary["l_overflow"] = bool(split["n_out"][1])
    else:
        summary = PC.shape_summary(table, p)
    with open(base + "_shapes.json", "w") as f:
        json.dump(summary, f, indent=1)
    PC.export_shape_text(summary, base + "_shapes.txt")


def _queue_floor(frame: dict, p: dict) -> dict:
    """The occupancy floor plan of the cleaned cloud (--floor_plan): raster, morphology, regions and picture, all left
    on the device (the grid's size is not known on the host yet); the writer makes the one read-back after the event."""
    plan = PC.floor_plan(frame["xyz"], frame["cols"], frame["count"], height_threshold=p["height_threshold"],
                         resolution=p["resolution"], min_area=p["min_area"])
    frame["floor"] = plan                                                      # what --floor_polygons outlines
    return plan


def _write_floorplan(base: str, params: dict, out: dict) -> None:
    """Writer-thread side (after the frame's event, so the plan is complete): the one read-back on a stream of this
    thread's own, then `{base}_floorplan.png` (PIL) and `{base}_floorplan.json`."""
    from PIL import Image

    plan = out["floor"]
    side = torch.cuda.Stream(plan["image"].device)
    with torch.cuda.stream(side):
        summary = PC.floor_plan_summary(plan)
    img = summary.pop("image")
    # no participants, or a grid past the capacity: a 1 x 1 white picture
    (Image.fromarray(img, "RGB") if img.size else Image.new("RGB", (1, 1), (255, 255, 255))).save(base + "_floorplan.png")
    with open(base + "_floorplan.json", "w") as f:
        json.dump(summary, f, indent=1)


def _queue_polygons(frame: dict, p: dict) -> dict:
    """The polygons of the floor plan the floor stage has left on the device (--floor_polygons): outlines,
    simplification, the mean height of the participants; the writer makes the one read-back after the event."""
    return PC.floor_polygons(dict(frame["floor"]), frame["xyz"], frame["count"])


def _write_polygons(base: str, params: dict, out: dict) -> None:
    """Writer-thread side (after the frame's event): the one read-back on a stream of this thread's own, then
    `{base}_floorplan.txt` (the reference's polygons file) and `{base}_floorplan_polygons.json`."""
    plan = out["polygons"]
    side = torch.cuda.Stream(plan["polygons"].device)
    with torch.cuda.stream(side):
        summary = PC.floor_polygons_summary(plan)
    PC.export_floorplan_text(base + "_floorplan.txt", summary)
    with open(base + "_floorplan_polygons.json", "w") as f:
        json.dump(summary, f, indent=1)


def _queue_slices(frame: dict, p: dict) -> dict:
    """The height-sliced floor plan of the cleaned cloud (--floor_slices): the slices' grids, closing sizes and
    morphology in one call each, then regions, outlines and polygons per slice, all left on the device; the writer makes
    the read-back after the event."""
    return PC.sliced_floor_plan(frame["xyz"], frame["count"], height_min=p["height_min"], height_max=p["height_max"],
                                num_slices=p["num_slices"], resolution=p["resolution"], min_area=p["min_area"])


def _write_slices(base: str, params: dict, out: dict) -> None:
    """Writer-thread side (after the frame's event): the read-back on a stream of this thread's own, then
    `{base}_floorslices.txt` (the reference's polygons file over all slices) and `{base}_floorslices.json`."""
    plan = out["slices"]
    side = torch.cuda.Stream(plan["stats"].device)
    with torch.cuda.stream(side):
        summary = PC.sliced_floor_plan_summary(plan)
    PC.export_sliced_floorplan_text(base + "_floorslices.txt", summary)
    with open(base + "_floorslices.json", "w") as f:
        json.dump(summary, f, indent=1)


def _queue_mesh(frame: dict, p: dict) -> dict:
    """The oriented point set of the cleaned cloud (--mesh_points): voxel grid, normals, orientation, PLY records.  Only
    the voxel count and the statistics are copied here; the records stay on the device and the writer fetches `count`."""
    op, oc, on, onrm, vst, nst = PC.oriented_points(frame["xyz"], frame["cols"], frame["count"], p["voxel_size"], p["max_nn"])
    frame.update(voxels=op, voxel_cols=oc, n_voxels=on, voxel_size=p["voxel_size"])      # what --simple_mesh meshes
    return {"count": _pinned(on.reshape(())), "voxel_stats": _pinned(vst), "normal_stats": _pinned(nst),
            "records": PC.ply_normals_records_async(op, onrm, oc)}


def _write_oriented(base: str, params: dict, out: dict) -> None:
    """Writer-thread side (after the frame's event, so the records are complete): fetch the first `count` records
    on a stream of this thread's own, then `{base}_oriented.ply` and `{base}_oriented.json`."""
    m, mesh = out["mesh"], params["mesh"]
    rec = m["records"]
    n = max(0, min(int(m["count"]), rec.shape[0]))
    side = torch.cuda.Stream(rec.device)
    with torch.cuda.stream(side):
        host = torch.empty((n, rec.shape[1]), dtype=rec.dtype, pin_memory=True)
        host.copy_(rec[:n], non_blocking=True)
    side.synchronize()
    PC.write_ply_normals_records(base + "_oriented.ply", host.numpy())
    summary = {"parameters": {"voxel_size": mesh["voxel_size"], "radius": 2.0 * mesh["voxel_size"], "max_nn": mesh["max_nn"],
                              "camera_location": [0.0, 0.0, 0.0]},
               "points": n,
               "voxel_stats": {k: float(v) for k, v in zip(PC.VOXEL_STATS, m["voxel_stats"].numpy())},
               "normal_stats": {k: float(v) for k, v in zip(PC.NORMAL_STATS, m["normal_stats"].numpy())}}
    with open(base + "_oriented.json", "w") as f:
        json.dump(summary, f, indent=1)


def _queue_trimesh(frame: dict, p: dict) -> dict:
    """The reference's simple mesh over the voxels the mesh stage has left on the device (--simple_mesh): the nearest
    neighbours of every voxel, the fan of triangles, the clean-up, the PLY records, and the mean distance to the 20 nearest
    from which the reference takes its ball-pivoting radii.  Counts and statistics are copied here; the writer fetches
    the records."""
    vox, n_vox, edge = frame["voxels"], frame["n_voxels"], 2.0 * frame["voxel_size"]
    tri, n_tri, kst, tst = PC.triangulate(vox, n_vox, p["neighbors"], edge)
    vrec, frec = PC.mesh_ply_records_async(vox, frame["voxel_cols"], tri)
    return {"vertices": _pinned(n_vox.reshape(())), "triangles": _pinned(n_tri.reshape(())), "knn_stats": _pinned(kst),
            "triangle_stats": _pinned(tst), "mean_distance": _pinned(PC.mean_neighbor_distance(vox, n_vox, 20, edge)),
            "vertex_records": vrec, "face_records": frec}


def _write_trimesh(base: str, params: dict, out: dict) -> None:
    """Writer-thread side (after the frame's event): fetch the live records on a stream of this thread's own, then
    `{base}_mesh.ply` and `{base}_mesh.json`."""
    m, p = out["trimesh"], params["trimesh"]
    side = torch.cuda.Stream(m["vertex_records"].device)
    host = []
    with torch.cuda.stream(side):
        for rec, count in ((m["vertex_records"], m["vertices"]), (m["face_records"], m["triangles"])):
            n = max(0, min(int(count), rec.shape[0]))
            host.append(torch.empty((n, rec.shape[1]), dtype=rec.dtype, pin_memory=True))
            host[-1].copy_(rec[:n], non_blocking=True)
    side.synchronize()
    PC.write_mesh_ply(base + "_mesh.ply", host[0].numpy(), host[1].numpy())
    mean = float(m["mean_distance"])
    summary = {"parameters": {"voxel_size": params["mesh"]["voxel_size"], "neighbors": p["neighbors"],
                              "cell_edge": 2.0 * params["mesh"]["voxel_size"], "method": "simple"},
               "vertices": host[0].shape[0], "triangles": host[1].shape[0],
               "knn_stats": {k: float(v) for k, v in zip(PC.KNN_EXACT_STATS, m["knn_stats"].numpy())},
               "triangle_stats": {k: float(v) for k, v in zip(PC.TRIANGLE_STATS, m["triangle_stats"].numpy())},
               "mean_neighbor_distance": mean, "mean_neighbor_distance_k": 20,
               "ball_pivoting_radii": [f * mean for f in PC.BALL_PIVOT_FACTORS]}
    with open(base + "_mesh.json", "w") as f:
        json.dump(summary, f, indent=1)


def _boundary(frame: dict, p: dict):
    """Queue the frame's boundary counts against its target (depth_pro.eval.boundary_metrics: the depth is still on the
    device) and their pinned host copy.  None, with a line of report, when the target is missing or cannot be used."""
    from depth_pro.eval import boundary_metrics as BM

    depth, target_path = frame["depth"], boundary_target_path(frame["path"], p["dir"])
    if not os.path.exists(target_path):
        print(f"No boundary target {target_path}: frame not scored")
        return None
    try:
        target = np.load(target_path)
        if tuple(target.shape) != tuple(depth.shape):
            raise ValueError(f"shape {target.shape}, the depth has {tuple(depth.shape)}")
        if target.dtype == np.float32:
            kind, name = BM.DP_BOUNDARY_DEPTH, "depth"
        elif target.dtype in (np.bool_, np.uint8):
            kind, name = BM.DP_BOUNDARY_MASK, "mask"
            target = target > 0.1                                           # the reference's alpha_threshold on the raw values
        else:
            raise ValueError(f"dtype {target.dtype} (float32: depth; bool / uint8: mask)")
        thresholds, _ = BM.get_thresholds_and_weights(1.05, 1.25, 10)
        passed = thresholds if kind == BM.DP_BOUNDARY_DEPTH else thresholds.astype(np.float32).astype(np.float64)
        counts = BM.boundary_counts(depth, target, passed, kind).view(torch.int64)
    except Exception as e:
        print(f"Boundary target {target_path} not used: {e}")
        return None
    return {"kind": kind, "name": name, "counts": _pinned(counts), "thresholds": thresholds, "shape": tuple(depth.shape)}


def _write_boundary(base: str, params: dict, out: dict) -> None:
    """Writer-thread side: the score from the counts, `{base}_boundary.json`; the run keeps the score for its mean."""
    from depth_pro.eval import boundary_metrics as BM

    bd = out["boundary"]
    counts = bd["counts"].numpy().tolist()
    score = float(BM.weighted_score(counts, bd["thresholds"], bd["kind"]))
    with open(base + "_boundary.json", "w") as f:
        json.dump({"kind": bd["name"], "metric": "SI_boundary_F1" if bd["kind"] == BM.DP_BOUNDARY_DEPTH else "SI_boundary_Recall",
                   "score": score, "thresholds": [float(t) for t in bd["thresholds"]], "directions": list(BM.DIRECTIONS),
                   "count_names": list(BM.COUNTS), "counts": counts, "H": bd["shape"][0], "W": bd["shape"][1]}, f, indent=1)
    params["boundary"]["scores"].append(score)


def _report_boundary(p: dict, world: int, rank: int) -> None:
    """Rank 0 prints the mean boundary score over the frames scored (one all-reduce of sum and count with several ranks)."""
    total, n = float(sum(p["scores"])), len(p["scores"])
    if world > 1:
        box = torch.tensor([total, float(n)], dtype=torch.float64, device=_device() if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(box)
        total, n = float(box[0]), int(box[1])
    if rank == 0:
        print(f"mean boundary score over {n} frames: {total / n:.6f}" if n else "no frame had a usable boundary target")


def _frame_rgb(frame: dict) -> torch.Tensor:
    """The frame's RGB image on the depth's device (uint8 (H, W, 3)), uploaded once for the stages that sample it."""
    if "rgb" not in frame:
        image = frame["image"]
        rgb = image if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(image))
        frame["rgb"] = rgb.to(frame["depth"].device, non_blocking=True)
    return frame["rgb"]


def _queue_anaglyph(frame: dict, p: dict) -> dict:
    """The red-cyan anaglyph of the frame (--anaglyph): one fused pass over image and depth, then its pinned host copy."""
    picture, bad = FX.anaglyph(_frame_rgb(frame), frame["depth"], p["separation"])
    return {"image": _pinned(picture), "bad": _pinned(bad)}


def _queue_parallax(frame: dict, p: dict) -> dict:
    """The frame's view of the parallax cycle (--parallax) at phase `index mod period`, then its pinned host copy."""
    h, w = frame["depth"].shape
    view = FX.view_params(p["motion"], p["amplitude"], w, h, int(frame["index"]) % p["period"], p["period"])
    pictures, bad = FX.warp_views(_frame_rgb(frame), frame["depth"], [view])
    return {"image": _pinned(pictures[0]), "bad": _pinned(bad[0])}


def _write_view(path: str, payload: dict) -> None:
    """Writer-thread side (after the frame's event): the RGB PNG, and a line when pixels had no finite depth."""
    _write_png(path, payload["image"].numpy())
    if int(payload["bad"]):
        print(f"{os.path.basename(path)}: {int(payload['bad'])} pixels without a finite depth written black")


def _write_anaglyph(base: str, params: dict, out: dict) -> None:
    _write_view(base + "_anaglyph.png", out["anaglyph"])


def _write_parallax(base: str, params: dict, out: dict) -> None:
    _write_view(base + "_parallax.png", out["parallax"])


def _queue_shadows(frame: dict, p: dict) -> dict:
    """The depth-shadow mask of the frame (--depth_shadows), ahead of the cloud: gradient, edges, region filter; with
    --drop_depth_shadows the cloud stage then back-projects the depth with the shadow pixels set to NaN."""
    res = SH.find_depth_shadows(frame["depth"], p["threshold_factor"], p["min_region_size"], drop=p["drop"])
    if p["drop"]:
        frame["cloud_depth"] = res["depth"]
    return {"mask": _pinned(res["mask"]), "stats": _pinned(res["stats"])}


def _write_shadows(base: str, params: dict, out: dict) -> None:
    """Writer-thread side (after the frame's event): `{base}_shadows.png` (8-bit grey, 255 = shadow) and `{base}_shadows.json`."""
    s, p = out["shadows"], params["shadows"]
    mask = s["mask"].numpy()
    _write_png(base + "_shadows.png", mask * np.uint8(255))
    stats = SH.stats_dict(s["stats"].numpy())
    with open(base + "_shadows.json", "w") as f:
        json.dump({"parameters": {"threshold_factor": p["threshold_factor"], "min_region_size": p["min_region_size"],
                                  "drop": p["drop"]},
                   "H": int(mask.shape[0]), "W": int(mask.shape[1]), "counts": {k: v for k, v in stats.items() if k != "gmax"},
                   "gmax": stats["gmax"], "nonfinite": stats["nonfinite"]}, f, indent=1)


def _queue_views(frame: dict, p: dict) -> dict:
    """The picture of the frame's cloud as the stages so far have left it (--render_view): bounds, cameras, one pass over
    the rows, the splats; then the pinned host copies."""
    res = RV.render_views(frame["xyz"], frame["cols"], views=p["views"], size=p["size"], point_size=p["point_size"],
                          count=frame["count"], sheet=p["sheet"], min_height=p["min_height"])
    return {k: _pinned(v) for k, v in res.items()}


def _write_views(base: str, params: dict, out: dict) -> None:
    """Writer-thread side (after the frame's event): `{base}_view.png` (RGB) and `{base}_view.json`."""
    r, p = out["views"], params["views"]
    image = r["image"].numpy()
    _write_png(base + "_view.png", image if p["sheet"] else image[0])
    cams = r["cameras"].numpy()
    with open(base + "_view.json", "w") as f:
        json.dump({"parameters": {"view": p["view"], "size": list(p["size"]), "point_size": p["point_size"],
                                  "min_height": p["min_height"]},
                   "views": list(p["views"]), "cameras": [[None if c != c else float(c) for c in cam] for cam in cams],
                   "counts": RV.stats_dict(r["stats"].numpy(), len(cams))}, f, indent=1)


def _queue_planshapes(frame: dict, p: dict) -> dict:
    """The plan picture with the shapes on it (--plan_shapes), behind the shapes: the plan of the rows the cluster stage
    fitted, the strokes and numbers from the tables still on the device; then the pinned host copies."""
    if "rects" not in frame:                            # no split: the reference's rectangle list of the table
        frame["rects"], frame["n_rects"] = PC.rectangle_list(frame["shapes"], frame["n_clusters"], MAX_CLUSTERS)
    res = OV.plan_with_shapes(frame["xyz"], frame["cols"], frame["count"], frame["rects"], frame["n_rects"], frame["shapes"],
                              frame["n_clusters"], size=p["size"], point_size=p["point_size"], min_height=p["min_height"],
                              stroke=p["stroke"], label_scale=p["label_scale"])
    return {k: _pinned(res[k]) for k in ("image", "camera", "stats", "plan_stats")}


def _write_planshapes(base: str, params: dict, out: dict) -> None:
    """Writer-thread side (after the frame's event): `{base}_plan.png` (RGB) and `{base}_plan.json`."""
    r, p = out["planshapes"], params["planshapes"]
    _write_png(base + "_plan.png", r["image"].numpy())
    with open(base + "_plan.json", "w") as f:
        json.dump({"parameters": {"size": list(p["size"]), "point_size": p["point_size"], "min_height": p["min_height"],
                                  "stroke": p["stroke"], "alpha": OV.STROKE_ALPHA, "label_scale": p["label_scale"],
                                  "split_l_shapes": p["split"]},
                   "camera": [None if c != c else float(c) for c in r["camera"].numpy()],
                   "counts": OV.stats_dict(r["stats"].numpy()),
                   "plan_counts": RV.stats_dict(r["plan_stats"].numpy(), 1)}, f, indent=1)


# ---- each stage's parameter dict from the loop's options `o`, checked first ----

def _ground_params(o: dict) -> dict:
    check_grid_size(o["grid_size"])
    return {"model": None, "dir": o["ground_params_dir"] or o.get("output_dir"), "grid": int(o["grid_size"]),
            "pct": o["ground_percentile"], "rot": o["rotation_offset"], "resolved": False}


def _clean_params(o: dict) -> dict:
    check_stray(o["stray_radius"], o["stray_neighbors"])
    return {"radius": float(o["stray_radius"]), "nb": int(o["stray_neighbors"])}


def _cluster_params(o: dict) -> dict:
    check_cluster(o["cluster_eps"], o["cluster_min_samples"], o["cluster_max_points"])
    return {"eps": float(o["cluster_eps"]), "min_samples": int(o["cluster_min_samples"]),
            "height_threshold": float(o["cluster_height"]), "max_points": int(o["cluster_max_points"])}


def _shapes_params(o: dict) -> dict:
    check_circularity(o["circularity_threshold"])
    return {"circularity_threshold": float(o["circularity_threshold"]), **({"l_split": True} if o["split_l_shapes"] else {}),
            **({"plan": True} if o["plan_shapes"] else {})}    # --plan_shapes: the tables stay in `frame` for that stage


def _floor_params(o: dict) -> dict:
    check_floor(o["floor_resolution"], o["floor_height"], o["floor_min_area"])
    return {"resolution": float(o["floor_resolution"]), "height_threshold": float(o["floor_height"]),
            "min_area": float(o["floor_min_area"])}


def _slices_params(o: dict) -> dict:
    check_floor_slices(o["floor_slices"], o["floor_slice_min"], o["floor_slice_max"], o["floor_slice_resolution"],
                       o["floor_slice_min_area"])
    return {"num_slices": int(o["floor_slices"]), "height_min": float(o["floor_slice_min"]),
            "height_max": float(o["floor_slice_max"]), "resolution": float(o["floor_slice_resolution"]),
            "min_area": float(o["floor_slice_min_area"])}


def _mesh_params(o: dict) -> dict:
    check_mesh(o["voxel_size"], o["normals_max_nn"])
    return {"voxel_size": float(o["voxel_size"]), "max_nn": int(o["normals_max_nn"])}


def _trimesh_params(o: dict) -> dict:
    check_mesh_neighbors(o["mesh_neighbors"])
    return {"neighbors": int(o["mesh_neighbors"])}


def _boundary_params(o: dict) -> dict:
    check_boundary_dir(o["boundary_dir"])
    return {"dir": o["boundary_dir"], "scores": []}


def check_anaglyph(separation) -> None:
    if not (np.isfinite(float(separation)) and float(separation) >= 0):
        raise ValueError(f"--anaglyph_separation must be finite and >= 0 (got {separation})")


def check_parallax(motion, amplitude, period) -> None:
    if motion not in FX.MOTIONS:
        raise ValueError(f"--parallax must be one of {', '.join(FX.MOTIONS)} (got {motion})")
    if not (np.isfinite(float(amplitude)) and float(amplitude) >= 0):
        raise ValueError(f"--parallax_amplitude must be finite and >= 0 (got {amplitude})")
    if int(period) < 1:
        raise ValueError(f"--parallax_period must be >= 1 (got {period})")


def _anaglyph_params(o: dict) -> dict:
    check_anaglyph(o["anaglyph_separation"])
    return {"separation": float(o["anaglyph_separation"])}


def _parallax_params(o: dict) -> dict:
    check_parallax(o["parallax"], o["parallax_amplitude"], o["parallax_period"])
    return {"motion": o["parallax"], "amplitude": float(o["parallax_amplitude"]), "period": int(o["parallax_period"])}


def check_shadows(threshold, min_region) -> None:
    if not np.isfinite(float(threshold)):
        raise ValueError(f"--shadow_threshold must be finite (got {threshold})")
    if int(min_region) < 0:
        raise ValueError(f"--shadow_min_region must be >= 0 (got {min_region})")


def _shadows_params(o: dict) -> dict:
    check_shadows(o["shadow_threshold"], o["shadow_min_region"])
    if o["drop_depth_shadows"] and "cloud" not in _stages_on(o):
        raise ValueError("--drop_depth_shadows requires --pointcloud (there is no cloud to drop the shadow pixels from)")
    return {"threshold_factor": float(o["shadow_threshold"]), "min_region_size": int(o["shadow_min_region"]),
            "drop": bool(o["drop_depth_shadows"])}


RENDER_VIEWS = tuple(RV.VIEW_PRESETS) + ("multi", RV.PLAN)


def check_render(view, size, point_size, min_height) -> Tuple[int, int]:
    if view not in RENDER_VIEWS:
        raise ValueError(f"--render_view must be one of {', '.join(RENDER_VIEWS)} (got {view})")
    try:
        w, h = (int(v) for v in str(size).lower().split("x"))
    except ValueError:
        raise ValueError(f"--render_size must be WxH (got {size})") from None
    if w < 1 or h < 1 or w * h >= 2 ** 31:
        raise ValueError(f"--render_size: W and H must be >= 1 and W * H < 2^31 (got {size})")
    if not (1 <= int(point_size) <= 15 and int(point_size) % 2 == 1):
        raise ValueError(f"--render_point_size must be odd and in [1, 15] (got {point_size})")
    if min_height is not None and not np.isfinite(float(min_height)):
        raise ValueError(f"--render_min_height must be finite (got {min_height})")
    return w, h


def _views_params(o: dict) -> dict:
    size = check_render(o["render_view"], o["render_size"], o["render_point_size"], o["render_min_height"])
    view = o["render_view"]
    plan = view == RV.PLAN
    return {"view": view, "views": RV.SHEET if view == "multi" else (view,), "sheet": view == "multi", "size": size,
            "point_size": int(o["render_point_size"]),
            "min_height": float(o["render_min_height"]) if plan and o["render_min_height"] is not None else None}


def check_plan_shapes(size, point_size, stroke, label_scale) -> Tuple[int, int]:
    try:
        w, h = (int(v) for v in str(size).lower().split("x"))
    except ValueError:
        raise ValueError(f"--plan_size must be WxH (got {size})") from None
    if w < 1 or h < 1 or w * h >= 2 ** 31:
        raise ValueError(f"--plan_size: W and H must be >= 1 and W * H < 2^31 (got {size})")
    if not (1 <= int(point_size) <= 15 and int(point_size) % 2 == 1):
        raise ValueError(f"--plan_point_size must be odd and in [1, 15] (got {point_size})")
    if not (np.isfinite(float(stroke)) and float(stroke) > 0):
        raise ValueError(f"--plan_stroke must be finite and > 0 (got {stroke})")
    if not 0 <= int(label_scale) <= 8:
        raise ValueError(f"--plan_label_scale must be in [0, 8] (got {label_scale})")
    return w, h


def _planshapes_params(o: dict) -> dict:
    size = check_plan_shapes(o["plan_size"], o["plan_point_size"], o["plan_stroke"], o["plan_label_scale"])
    height = float(o["cluster_height"])                 # the plan shows the rows the cluster stage fitted
    return {"size": size, "point_size": int(o["plan_point_size"]), "stroke": float(o["plan_stroke"]),
            "label_scale": int(o["plan_label_scale"]), "min_height": None if height != height else height,
            "split": bool(o["split_l_shapes"])}


class Stage(NamedTuple):
    """One stage of the frame loop, described once."""
    name: str
    implies: Optional[str]              # the stage that has to be on for this one
    on: Callable[[dict], bool]          # the loop's options -> does the caller ask for it
    params: Callable[[dict], dict]      # the loop's options -> its parameter dict, checked (ValueError)
    suffixes: Tuple[str, ...]           # --resume: a finished frame has `{base}{suffix}` for each
    queue: Callable                     # (frame, its parameters) -> payload: its GPU work, on the current stream
    write: Optional[Callable]           # (base path, {stage: parameters}, {stage: payload}): its files, writer thread
    end: Optional[Callable] = None      # (its parameters, world, rank): after the last frame


# in the order they are queued on a frame's stream; a stage stands behind the one it implies
STAGES = (
    Stage("shadows", None, lambda o: bool(o["depth_shadows"] or o["drop_depth_shadows"]), _shadows_params,
          ("_shadows.png", "_shadows.json"), _queue_shadows, _write_shadows),
    Stage("cloud", None, lambda o: o["pointcloud"], lambda o: {}, (), _backproject, _write_cloud),
    Stage("ground", "cloud", lambda o: o["normalize_ground"], _ground_params, (), _queue_ground, None, _end_ground),
    Stage("clean", "ground", lambda o: o["clean_pointcloud"], _clean_params, ("_clean.ply",), _queue_clean, None),
    Stage("views", "cloud", lambda o: o["render_view"] is not None, _views_params, ("_view.png", "_view.json"),
          _queue_views, _write_views),
    Stage("cluster", "clean", lambda o: o["cluster_pointcloud"], _cluster_params, ("_clusters.json",),
          _queue_cluster, _write_clusters),
    Stage("shapes", "cluster", lambda o: o["fit_shapes"] or o["split_l_shapes"], _shapes_params, ("_shapes.json",),
          _queue_shapes, _write_shapes),
    Stage("planshapes", "shapes", lambda o: bool(o["plan_shapes"]), _planshapes_params, ("_plan.png", "_plan.json"),
          _queue_planshapes, _write_planshapes),
    Stage("floor", "clean", lambda o: o["floor_plan"], _floor_params, ("_floorplan.png", "_floorplan.json"),
          _queue_floor, _write_floorplan),
    Stage("slices", "clean", lambda o: bool(o["floor_slices"]), _slices_params, ("_floorslices.txt", "_floorslices.json"),
          _queue_slices, _write_slices),
    Stage("mesh", "clean", lambda o: o["mesh_points"], _mesh_params, ("_oriented.ply", "_oriented.json"),
          _queue_mesh, _write_oriented),
    Stage("trimesh", "mesh", lambda o: o["simple_mesh"], _trimesh_params, ("_mesh.ply", "_mesh.json"),
          _queue_trimesh, _write_trimesh),
    Stage("boundary", None, lambda o: o["boundary_dir"] is not None, _boundary_params, ("_boundary.json",),
          _boundary, _write_boundary, _report_boundary),
    Stage("anaglyph", None, lambda o: bool(o["anaglyph"]), _anaglyph_params, ("_anaglyph.png",), _queue_anaglyph, _write_anaglyph),
    Stage("parallax", None, lambda o: o["parallax"] is not None, _parallax_params, ("_parallax.png",), _queue_parallax,
          _write_parallax),
    Stage("polygons", "floor", lambda o: o["floor_polygons"], lambda o: {}, ("_floorplan.txt", "_floorplan_polygons.json"),
          _queue_polygons, _write_polygons),
)
_DEFAULTS = {k: p.default for k, p in inspect.signature(batch_generate_depth_maps).parameters.items() if p.default is not p.empty}


def main():
    parser = argparse.ArgumentParser(description="Generate depth maps from input images")
    parser.add_argument("--input_dir", type=str, default="./TEMP/FRAMES", help="Directory containing input images")
    parser.add_argument("--output_dir", type=str, default="./TMP/DEPTH", help="Directory to save output depth maps")
    parser.add_argument("--pattern", type=str, default="*.png", help="Glob pattern to match input images")
    parser.add_argument("--downscale_factor", type=float, default=1.0,
                        help="Downscale input images for faster processing")
    parser.add_argument("--half_precision", action="store_true", help="Use float16 for faster computation")
    parser.add_argument("--raw", action="store_true", help="Save raw depth maps (grayscale) instead of colored ones")
    parser.add_argument("--pointcloud", action="store_true",
                        help="Also write {frame}_points.ply (depth_to_3d back-projection with RGB colours)")
    parser.add_argument("--normalize_ground", action="store_true",
                        help="Level {frame}_points.ply so the ground is y = 0 (implies --pointcloud): plane from "
                             "ground.json or fitted on the first frame, then the grid-based ground adjustment")
    parser.add_argument("--ground_params_dir", type=str, default=None,
                        help="Directory to save/load ground plane parameters (ground.json; default: --output_dir)")
    parser.add_argument("--rot_x", type=float, default=0.0, help="Ground plane rotation offset around X (degrees)")
    parser.add_argument("--rot_y", type=float, default=0.0, help="Ground plane rotation offset around Y (degrees)")
    parser.add_argument("--rot_z", type=float, default=0.0, help="Ground plane rotation offset around Z (degrees)")
    parser.add_argument("--grid_size", type=int, default=20,
                        help=f"Grid cells per axis for the ground adjustment (1..{MAX_GRID_SIZE}, default 20)")
    parser.add_argument("--ground_percentile", type=int, default=5,
                        help="Percentile of the lowest points per cell for the ground adjustment (default 5)")
    parser.add_argument("--clean_pointcloud", action="store_true",
                        help="Clean the levelled cloud (implies --normalize_ground): remove stray points, then shadow "
                             "columns; writes {frame}_clean.ply in place of {frame}_points.ply")
    parser.add_argument("--stray_radius", type=float, default=0.1,
                        help="Neighbourhood radius of the stray-point removal in metres (default 0.1)")
    parser.add_argument("--stray_neighbors", type=int, default=20,
                        help="Neighbours (the point itself included) a point needs within the radius (default 20)")
    parser.add_argument("--cluster_pointcloud", action="store_true",
                        help="Cluster the cleaned cloud's top-down projection (implies --clean_pointcloud): DBSCAN "
                             "labels to {frame}_labels.npy, counts and per-cluster boxes to {frame}_clusters.json")
    parser.add_argument("--cluster_eps", type=float, default=0.2, help="DBSCAN neighbourhood radius in metres (default 0.2)")
    parser.add_argument("--cluster_min_samples", type=int, default=5,
                        help="Neighbours (the point itself included) that make a core point (default 5)")
    parser.add_argument("--cluster_height", type=float, default=1.3,
                        help="Cluster the points with y >= this height in metres (default 1.3; nan: every height)")
    parser.add_argument("--cluster_max_points", type=int, default=100000,
                        help="Cluster at most this many points, an even stride of the rest (default 100000; 0: all)")
    parser.add_argument("--fit_shapes", action="store_true",
                        help="Fit a rectangle or a circle to every cluster (implies --cluster_pointcloud): "
                             "{frame}_shapes.json and the floor-plan text {frame}_shapes.txt")
    parser.add_argument("--split_l_shapes", action="store_true",
                        help="Split rectangles that hold separate occupied parts, as the reference's "
                             "detect_and_split_l_shapes does (implies --fit_shapes): the split list goes to "
                             "{frame}_shapes.json and {frame}_shapes.txt")
    parser.add_argument("--circularity_threshold", type=float, default=0.85,
                        help="Hull area over circle area above which a cluster may be a circle (default 0.85)")
    parser.add_argument("--mesh_points", action="store_true",
                        help="Write the oriented point set a mesher starts from (implies --clean_pointcloud): voxel grid, "
                             "normals, orientation towards the camera; {frame}_oriented.ply and {frame}_oriented.json")
    parser.add_argument("--voxel_size", type=float, default=0.05,
                        help="Voxel edge of --mesh_points in metres (default 0.05); normals use radius 2 * voxel_size")
    parser.add_argument("--normals_max_nn", type=int, default=30,
                        help=f"Neighbours at the most per normal (1..{PC.MAX_NN}, default 30)")
    # the two options below (and --floor_polygons, --floor_slices, --anaglyph, --parallax, --depth_shadows, --render_view, --plan_shapes and their options) are passed on only when given: a run without them passes the keywords it always passed
    parser.add_argument("--simple_mesh", action="store_true", default=argparse.SUPPRESS,
                        help="Mesh the voxels of --mesh_points (which it implies) as the reference's --mesh_method simple "
                             "does: nearest neighbours, a fan of triangles, clean-up; {frame}_mesh.ply and {frame}_mesh.json")
    parser.add_argument("--mesh_neighbors", type=int, default=argparse.SUPPRESS,
                        help=f"Nearest neighbours per vertex of --simple_mesh (2..{PC.MAX_K}, default 6)")
    parser.add_argument("--floor_plan", action="store_true",
                        help="Write the occupancy floor plan of the cleaned cloud (implies --clean_pointcloud): top-down "
                             "grid, closing and opening, connected regions; {frame}_floorplan.png and {frame}_floorplan.json")
    parser.add_argument("--floor_resolution", type=float, default=0.1, help="Cell size of --floor_plan in metres (default 0.1)")
    parser.add_argument("--floor_height", type=float, default=1.3,
                        help="Rasterise the points with y >= this height in metres (default 1.3; nan: every height)")
    parser.add_argument("--floor_min_area", type=float, default=0.025,
                        help="Draw the regions of at least this area in square metres (default 0.025)")
    parser.add_argument("--floor_polygons", action="store_true", default=argparse.SUPPRESS,
                        help="Trace and simplify the outline of every region of --floor_plan (which it implies), as the "
                             "reference's approximate_contour does: {frame}_floorplan.txt and {frame}_floorplan_polygons.json")
    parser.add_argument("--floor_slices", type=int, default=argparse.SUPPRESS, metavar="N",
                        help="Write the reference's default floor plan of the cleaned cloud (implies --clean_pointcloud): N "
                             "height slices (the reference: 5), each with its own grid, a closing of the size its grid asks "
                             "for, and polygons; {frame}_floorslices.txt and {frame}_floorslices.json")
    parser.add_argument("--floor_slice_min", type=float, default=argparse.SUPPRESS,
                        help="Lower end of the lowest slice of --floor_slices in metres (default 0.1)")
    parser.add_argument("--floor_slice_max", type=float, default=argparse.SUPPRESS,
                        help="Upper end of the highest slice of --floor_slices in metres (default 2.5)")
    parser.add_argument("--floor_slice_resolution", type=float, default=argparse.SUPPRESS,
                        help="Cell size of --floor_slices in metres (default 0.05)")
    parser.add_argument("--floor_slice_min_area", type=float, default=argparse.SUPPRESS,
                        help="Keep the polygons of --floor_slices of at least this area in square metres (default 0.1)")
    parser.add_argument("--anaglyph", action="store_true", default=argparse.SUPPRESS,
                        help="Write {frame}_anaglyph.png, the red-cyan anaglyph of the frame and its depth (RGB)")
    parser.add_argument("--anaglyph_separation", type=float, default=argparse.SUPPRESS,
                        help="Separation between the left and the right view of --anaglyph (default 0.05; 0.01-0.1 recommended)")
    parser.add_argument("--parallax", type=str, choices=list(FX.MOTIONS), default=argparse.SUPPRESS,
                        help="Write {frame}_parallax.png, the frame seen from a camera moving through the reference's "
                             "parallax cycle (circle, zoom or swing), at phase (frame position) mod --parallax_period")
    parser.add_argument("--parallax_amplitude", type=float, default=argparse.SUPPRESS,
                        help="Amplitude of the camera motion of --parallax (default 0.05; 0.01-0.2 recommended)")
    parser.add_argument("--parallax_period", type=int, default=argparse.SUPPRESS,
                        help="Frames per cycle of --parallax (default 150: 5 s at 30 frames/s)")
    parser.add_argument("--depth_shadows", action="store_true", default=argparse.SUPPRESS,
                        help="Write {frame}_shadows.png (8-bit, 255 = shadow) and {frame}_shadows.json: the depth-discontinuity "
                             "shadow mask of the frame's depth (the reference's find_depth_shadows)")
    parser.add_argument("--shadow_threshold", type=float, default=argparse.SUPPRESS,
                        help="Normalised gradient above which a pixel is an edge for --depth_shadows (default 0.2)")
    parser.add_argument("--shadow_min_region", type=int, default=argparse.SUPPRESS,
                        help="Free regions of fewer pixels than this are shadow for --depth_shadows (default 100)")
    parser.add_argument("--drop_depth_shadows", action="store_true", default=argparse.SUPPRESS,
                        help="Leave the shadow pixels out of the point cloud (implies --depth_shadows, requires --pointcloud); "
                             "the reference fills them instead, dropping them is this project's own")
    parser.add_argument("--render_view", type=str, choices=list(RENDER_VIEWS), default=argparse.SUPPRESS,
                        help="Write {frame}_view.png, a picture of the frame's latest point cloud made on the GPU (implies "
                             "--pointcloud): one of the reference's view presets, multi (their 2 x 2 sheet) or plan (top-down), "
                             "and {frame}_view.json (the cameras and the counts)")
    parser.add_argument("--render_size", type=str, default=argparse.SUPPRESS, metavar="WxH",
                        help="Size of the picture of --render_view (default 1280x720; each quadrant of multi has this size)")
    parser.add_argument("--render_point_size", type=int, default=argparse.SUPPRESS,
                        help="Side of a point's square in pixels for --render_view, odd, 1..15 (default 7)")
    parser.add_argument("--render_min_height", type=float, default=argparse.SUPPRESS,
                        help="Show only the points with y >= this height in --render_view plan (default: all)")
    parser.add_argument("--plan_shapes", action="store_true", default=argparse.SUPPRESS,
                        help="Write {frame}_plan.png, the top-down plan of the cleaned cloud with the fitted rectangles and circles "
                             "stroked on it and numbered, made on the GPU (implies --fit_shapes), and {frame}_plan.json (parameters, "
                             "camera, counts)")
    parser.add_argument("--plan_size", type=str, default=argparse.SUPPRESS, metavar="WxH",
                        help="Size of the picture of --plan_shapes (default 1280x720)")
    parser.add_argument("--plan_point_size", type=int, default=argparse.SUPPRESS,
                        help="Side of a point's square in pixels for --plan_shapes, odd, 1..15 (default 7)")
    parser.add_argument("--plan_stroke", type=float, default=argparse.SUPPRESS,
                        help="Width of the shapes' outlines in pixels for --plan_shapes (default 3.0)")
    parser.add_argument("--plan_label_scale", type=int, default=argparse.SUPPRESS,
                        help="Pixels per font pixel of the shapes' numbers for --plan_shapes, 0..8 (default 2; 0: no numbers)")
    parser.add_argument("--boundary_dir", type=str, default=None,
                        help="Score each frame against DIR/{frame}.npy with the Depth Pro boundary metric (float32: a depth, "
                             "SI_boundary_F1; bool / uint8: a mask, SI_boundary_Recall); writes {frame}_boundary.json")
    parser.add_argument("--resume", action="store_true",
                        help="Skip frames whose {frame}_depth.png (with --clean_pointcloud: and {frame}_clean.ply; with "
                             "--cluster_pointcloud: and {frame}_clusters.json; with --fit_shapes: and {frame}_shapes.json; with "
                             "--mesh_points: and {frame}_oriented.ply / .json; with --simple_mesh: and {frame}_mesh.ply / .json; "
                             "with --floor_plan: and {frame}_floorplan.png / .json; with --floor_polygons: and {frame}_floorplan.txt / "
                             "_floorplan_polygons.json; with --floor_slices: and {frame}_floorslices.txt / .json; with "
                             "--boundary_dir, for a frame with a target: and {frame}_boundary.json; with --anaglyph: and "
                             "{frame}_anaglyph.png; with --parallax: and {frame}_parallax.png; with --depth_shadows: and {frame}_shadows.png / "
                             ".json; with --render_view: and {frame}_view.png / .json; with --plan_shapes: and {frame}_plan.png / .json) already "
                             "exists in --output_dir")
    parser.add_argument("--colormap", type=str, default="turbo",
                        choices=["turbo", "viridis", "plasma", "inferno", "magma", "cividis", "jet"],
                        help="Colormap for depth visualization")
    args = parser.parse_args()
    kw = vars(args)
    kw.update(colored=not kw.pop("raw"), cmap=kw.pop("colormap"), rotation_offset=[kw.pop(f"rot_{a}") for a in "xyz"])
    try:
        check_grid_size(args.grid_size)
        if not 0 <= args.ground_percentile <= 100:
            raise ValueError("--ground_percentile must be in [0, 100]")
        check_stray(args.stray_radius, args.stray_neighbors)         # these, whether their stage is on or not
        check_cluster(args.cluster_eps, args.cluster_min_samples, args.cluster_max_points)
        check_circularity(args.circularity_threshold)
        if "mesh_neighbors" in kw:
            check_mesh_neighbors(kw["mesh_neighbors"])
        resolve_stages(**kw)                                        # and every stage that is on
    except ValueError as e:
        parser.error(str(e))
    batch_generate_depth_maps(**kw)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
