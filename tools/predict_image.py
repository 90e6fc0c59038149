"""The picture end of the reference's KITTI/test_simple.py (:130-175), which tools/test_simple.py leaves out: any file PIL
reads -> resized to the network size with kitti_inputs.color_pyramid (Pillow's 8-bit Lanczos, on the GPU) -> encoder +
(dense|sparse) wavelet decoder -> `<name>_disp.npy` (scaled disparity) and `<name>_disp.jpeg`: the disparity at the
picture's own size, min .. 95th percentile through magma (visualize.disparity_image; the bytes handed to PIL are the ones
matplotlib gives the reference).  Needs the MI355X; without --image a synthetic picture of --size is used, without
--weights the networks are randomly initialised.

    python tools/predict_image.py --out /tmp/out [--image FILE ...] [--sparse --threshold 0.05] [--weights DIR]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from PIL import Image

from wavelet_monodepth_amd import kitti_inputs, synth, visualize
from wavelet_monodepth_amd.encoders import ResnetEncoder
from wavelet_monodepth_amd.kitti import make_depth_decoder


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--image", nargs="*", default=[], help="pictures PIL reads")
    ap.add_argument("--size", type=int, nargs=2, default=(375, 1242), metavar=("H", "W"), help="the synthetic picture's size")
    ap.add_argument("--weights", help="folder with encoder.pth / depth.pth")
    ap.add_argument("--num_layers", type=int, default=18)
    ap.add_argument("--sparse", action="store_true")
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--height", type=int, default=192)
    ap.add_argument("--width", type=int, default=640)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(args.out, exist_ok=True)
    enc = ResnetEncoder(args.num_layers)
    dec = make_depth_decoder(enc.num_ch_enc, range(4), use_wavelets=True, use_sparse=args.sparse)
    if args.weights:
        sd = torch.load(os.path.join(args.weights, "encoder.pth"), map_location="cpu")
        enc.load_state_dict({k: v for k, v in sd.items() if k in enc.state_dict()})     # test_simple.py:82-88
        dec.load_state_dict(torch.load(os.path.join(args.weights, "depth.pth"), map_location="cpu"))
    else:
        synth.fill_state_dict(dec, seed=1)
    enc.to(dev).eval()
    dec.to(dev).eval()
    if args.image:
        frames = [(os.path.splitext(os.path.basename(p))[0], np.asarray(Image.open(p).convert("RGB")).copy()) for p in args.image]
    else:
        frames = [("image", (synth.uniform(tuple(args.size) + (3,), "picture", 0, 0.0, 1.0) * 255).astype(np.uint8))]
    for name, frame in frames:
        frame = torch.from_numpy(frame).to(dev)[None]                                   # test_simple.py:131-134
        img = kitti_inputs.color_pyramid(frame, args.height, args.width, num_scales=1)[0][1]
        with torch.no_grad():
            out = dec(enc(img), args.threshold) if args.sparse else dec(enc(img))
        disp = out[("disp", 0)].float()
        np.save(os.path.join(args.out, "%s_disp.npy" % name), (0.01 + (10.0 - 0.01) * disp).cpu().numpy())   # disp_to_depth(., 0.1, 100)
        rgb, rng = visualize.disparity_image(disp, size=tuple(frame.shape[1:3]), return_range=True)       # test_simple.py:144-175
        Image.fromarray(rgb[0].cpu().numpy()).save(os.path.join(args.out, "%s_disp.jpeg" % name))
        print("%s: %d x %d, disparity %.4f .. %.4f (95th percentile) -> %s_disp.jpeg" % ((name,) + tuple(frame.shape[1:3]) + tuple(rng[0].tolist()) + (name,)))


if __name__ == "__main__":
    main()
