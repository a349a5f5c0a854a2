#!/usr/bin/env python3
"""Drop-in for the reference `OLD_SCRIPTS/depth_video_effect.py` (3D_EFFECTS_README.md), on the MI355X engine.

Same options and the same two functions (`create_parallax_effect`, `create_3d_anaglyph`); depth comes from this
package's model, the views from `depth_pro.effects` (csrc/dp_effects.hip).  What differs, on purpose (DESIGN.md
section 20): the views are not transposed, the anaglyph is written as RGB (the reference hands its RGB array to
`cv2.imwrite`, which swaps red and blue on file), and the parallax frames are written as numbered PNGs into
`{stem of output_path}_frames/` instead of an mp4 (no encoder here): `frame_00000.png` ... in the reference's frame
order, `int(duration * fps)` of them.  `--scale` other than 1.0 is refused (the reference resizes the float32 depth with
cv2.resize, which is not built).
"""

from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_pro  # noqa: E402
from depth_pro import effects as FX  # noqa: E402

CHUNK = 8        # parallax views made (and held on the host) at a time


def _frame(image_path, model):
    """(uint8 (H, W, 3) device image, float32 (H, W) device depth) of one image; `model`: an already-built
    (model, transform) pair (tests), default: the frame loop's cached one."""
    if model is None:
        import generate_depth_maps as G

        model = G._model(G._device(), False)
    model, transform = model
    image, _, f_px = depth_pro.load_rgb(image_path)
    image = np.ascontiguousarray(image)
    with torch.no_grad():
        depth = model.infer(transform(image), f_px=f_px)["depth"]
    return torch.from_numpy(image).to(depth.device), depth.to(torch.float32).contiguous()


def _report(bad: int, what: str) -> None:
    if bad:
        print(f"{what}: {bad} pixels without a finite depth written black")


def frames_dir(output_path: str) -> str:
    return os.path.splitext(output_path)[0] + "_frames"


def create_parallax_effect(image_path, output_path, duration=5.0, fps=30, amplitude=0.05, motion_type="circle",
                           resolution_scale=1.0, model=None):
    """The reference's parallax video (:10-111) as numbered PNG frames; returns the list of files written."""
    from generate_depth_maps import _write_png

    if motion_type not in FX.MOTIONS:
        raise ValueError(f"Unknown motion type: {motion_type}")
    if resolution_scale != 1.0:
        raise ValueError("--scale other than 1.0 is not supported (the reference's cv2.resize of the float32 depth is not built)")
    total_frames = int(duration * fps)
    image, depth = _frame(image_path, model)
    out_dir = frames_dir(output_path)
    os.makedirs(out_dir, exist_ok=True)
    print(f"Creating parallax effect with {total_frames} frames...")
    files, bad = [], 0
    for f0 in range(0, total_frames, CHUNK):
        frames = range(f0, min(f0 + CHUNK, total_frames))
        views, bad_dev = FX.parallax_views(image, depth, motion_type, amplitude, total_frames, frames)
        host, bad = views.cpu().numpy(), bad + int(bad_dev.sum())
        for f, picture in zip(frames, host):
            files.append(os.path.join(out_dir, f"frame_{f:05d}.png"))
            _write_png(files[-1], picture)
    _report(bad, out_dir)
    print(f"Frames saved to {out_dir}")
    return files


def create_3d_anaglyph(image_path, output_path, separation=0.05, model=None):
    """The reference's red-cyan anaglyph (:113-183), written to `output_path` as RGB; returns the array."""
    from PIL import Image

    image, depth = _frame(image_path, model)
    picture, bad = FX.anaglyph(image, depth, separation)
    picture = picture.cpu().numpy()
    Image.fromarray(picture, "RGB").save(output_path)
    _report(int(bad), output_path)
    print(f"Anaglyph image saved to {output_path}")
    return picture


def main():
    parser = argparse.ArgumentParser(description="Create 3D effects from a single image using depth")
    parser.add_argument("--image_path", type=str, required=True, help="Path to input image")
    parser.add_argument("--output_path", type=str, required=True,
                        help="Path to save output (parallax: its stem names the directory of frames)")
    parser.add_argument("--effect", type=str, default="parallax", choices=["parallax", "anaglyph"],
                        help="Type of 3D effect to create")
    parser.add_argument("--duration", type=float, default=5.0, help="Duration of video in seconds")
    parser.add_argument("--fps", type=int, default=30, help="Frames per second")
    parser.add_argument("--amplitude", type=float, default=0.05, help="Amplitude of camera motion (0.01-0.2 recommended)")
    parser.add_argument("--motion", type=str, default="circle", choices=list(FX.MOTIONS), help="Type of camera motion")
    parser.add_argument("--scale", type=float, default=1.0, help="Scale factor for output resolution (only 1.0)")
    parser.add_argument("--separation", type=float, default=0.05,
                        help="Separation between left and right views (0.01-0.1 recommended)")
    args = parser.parse_args()
    if args.scale != 1.0:
        parser.error("--scale other than 1.0 is not supported (the reference's cv2.resize of the float32 depth is not built)")
    if args.effect == "parallax":
        create_parallax_effect(args.image_path, args.output_path, duration=args.duration, fps=args.fps,
                               amplitude=args.amplitude, motion_type=args.motion, resolution_scale=args.scale)
    else:
        create_3d_anaglyph(args.image_path, args.output_path, separation=args.separation)


if __name__ == "__main__":
    main()
