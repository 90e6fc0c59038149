"""Depth hints for one stereo pair, on the GPU from the decoded frames on: KITTI/precompute_depth_hints.py without OpenCV.

    python tools/precompute_depth_hints.py BASE.jpg LOOKUP.jpg --side l|r --out hint.npy [--height 320 --width 1024]

PIL decodes the two files; kitti_inputs.color_pyramid resizes them (Pillow's Lanczos filter, the reference's
transforms.Resize(..., ANTIALIAS)); stereo.precompute_depth_hints runs the twelve matcher settings, converts disparities to
depth with the reference's intrinsics (K[0, 0] = 0.58 width, baseline 0.1) and keeps, per pixel, the candidate with the lowest
reprojection loss.  The file holds float32 [1,H,W] like the reference's, 0 where there is no hint.  --side is the base image's:
`l` (image_02) or `r` (image_03), which is matched mirrored.  The matcher follows the integer specification in DESIGN.md, not
OpenCV's code: the hints are of the same kind as the reference's, not equal to them, and the distance has not been measured."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from PIL import Image

from wavelet_monodepth_amd import kitti_inputs, stereo


def load(path):
    with open(path, "rb") as f:
        with Image.open(f) as img:
            return np.asarray(img.convert("RGB"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("base")
    ap.add_argument("lookup")
    ap.add_argument("--side", choices=("l", "r"), required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--height", type=int, default=320)
    ap.add_argument("--width", type=int, default=1024)
    opt = ap.parse_args()
    dev = torch.device("cuda:0")
    base, lookup = load(opt.base), load(opt.lookup)
    if base.shape != lookup.shape:
        sys.exit("the two images differ in size: %s, %s" % (base.shape, lookup.shape))
    frames = torch.from_numpy(np.stack([base, lookup])).to(dev)
    u8 = kitti_inputs.color_pyramid(frames, opt.height, opt.width, num_scales=1)[0][0]      # uint8 [2,h,w,3]
    K = np.array([[0.58 * opt.width, 0, 0.5 * opt.width, 0], [0, 1.92 * opt.height, 0.5 * opt.height, 0], [0, 0, 1, 0], [0, 0, 0, 1]],
                 dtype=np.float32)
    inv_K = np.linalg.pinv(K)
    out = stereo.precompute_depth_hints(u8[0:1], u8[1:2], opt.side == "r", torch.from_numpy(K)[None].to(dev),
                                        torch.from_numpy(inv_K)[None].to(dev))
    hint = out["depth_hint"][0].cpu().numpy()
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    np.save(opt.out, hint)
    print("%s: %dx%d, %.1f %% of the pixels have a hint" % (opt.out, opt.height, opt.width, 100 * float(out["depth_hint_mask"].mean())))


if __name__ == "__main__":
    main()
