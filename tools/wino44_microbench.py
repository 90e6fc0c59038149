"""One trunk layer on the three-pass F(4x4,3x3) kernels (wmd_conv_wino44_fwd) against today's path, in one process.

For the layer: the error of both paths against a float64 direct convolution (max |err| / max |ref|), and their times -- hipEvents
around the whole operator (today: the convolution and its split-K reduce; F(4x4): the three launches), 20 launches after 5 warm-ups,
a 384 MB fill between launches so that every launch starts from cold caches as it does inside a decoder step
(tools/traffic_probe.py) -- plus the library's own per-kernel records of the same launches.  Today's path runs the choice of the
committed tuner cache.
usage: python tools/wino44_microbench.py <layer> [--batch B] [--iters N] [--no-spoil] [--no-ref]
       layer: L1 L2 L3 L4 (KITTI R18 640x192), R1 R3 (R50 1024x320, batch 8)"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from wavelet_monodepth_amd import _lib, ops, tuner

# name: (C1, up1, C2, Cout, H, W, default batch)
LAYERS = {"L1": (256, 2, 256, 256, 12, 40, 12), "L2": (256, 1, 0, 128, 12, 40, 12), "L3": (128, 2, 128, 128, 24, 80, 12),
          "L4": (128, 1, 0, 64, 24, 80, 12), "R1": (256, 2, 1024, 256, 20, 64, 8), "R3": (128, 2, 512, 128, 40, 128, 8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("layer", choices=sorted(LAYERS))
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-spoil", action="store_true", help="no cache-evicting fill between launches")
    ap.add_argument("--no-ref", action="store_true", help="skip the float64 reference (CPU, a few seconds)")
    args = ap.parse_args()
    C1, up, C2, Cout, H, W, B = LAYERS[args.layer]
    B = args.batch or B
    tuner.preload(os.path.join(ROOT, "profiles", "r06_tune_cache.json"))
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(44)
    x1 = torch.randn(B, C1, H // up, W // up, generator=g)
    x2 = torch.randn(B, C2, H, W, generator=g) if C2 else None
    w = torch.randn(Cout, C1 + C2, 3, 3, generator=g) * (2.0 / (9 * (C1 + C2))) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    x1d, x2d, wd, bd = x1.to(dev), None if x2 is None else x2.to(dev), w.to(dev), b.to(dev)

    paths = {"today": lambda: ops.conv2d_fused(x1d, wd, bd, x2=x2d, up1=up, pad="reflect", act="elu"),
             "wino44": lambda: ops.conv3x3_wino44_nograd(x1d, wd, bd, x2=x2d, up1=up, pad="reflect", act="elu")}
    out = {"layer": args.layer, "problem": "conv|%d|%d|%d|%d|%d|%d|%d|3" % (B, H, W, C1, up, C2, Cout), "tiles": B * ((H + 3) // 4) * ((W + 3) // 4)}
    with torch.no_grad():
        ys = {k: f() for k, f in paths.items()}
        torch.cuda.synchronize()
        if not args.no_ref:
            x = x1.double()
            if up == 2:
                x = F.interpolate(x, scale_factor=2, mode="nearest")
            if x2 is not None:
                x = torch.cat([x, x2.double()], 1)
            ref = F.elu(F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w.double(), b.double()))
            for k, y in ys.items():
                out["err_" + k] = float((y.cpu().double() - ref).abs().max() / ref.abs().max())
        out["wino44_vs_today"] = float((ys["wino44"] - ys["today"]).abs().max() / ys["today"].abs().max())
        spoil = None if args.no_spoil else torch.empty(96 * 1024 * 1024, device=dev)   # 384 MB > the 256 MB Infinity Cache
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for k, f in paths.items():
            ts = []
            for it in range(args.warmup + args.iters):
                if spoil is not None:
                    spoil.fill_(float(it))
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                if it >= args.warmup:
                    ts.append(e0.elapsed_time(e1) * 1e3)
            ts.sort()
            _lib.profile_begin()      # the same launches once more under the library's per-kernel events (their own pass: the
            for it in range(args.iters):      # events sit between the launches)
                if spoil is not None:
                    spoil.fill_(float(it))
                f()
            recs = _lib.profile_end()
            out[k] = {"min_us": round(ts[0], 1), "median_us": round(ts[len(ts) // 2], 1),
                      "kernels_us": {r["kernel"]: round(r["ms"] * 1e3 / r["calls"], 1) for r in recs},
                      "kernels_sum_us": round(sum(r["ms"] * 1e3 / args.iters for r in recs), 1)}
    a = ops._conv_args(B, H, W, C1, up, C2, Cout, 3, "reflect", "elu", 0.0)
    l = _lib.lib()
    ntp = -(-out["tiles"] // 32) * 32
    k1, k2, co = -(-C1 // 32) * 32, -(-C2 // 32) * 32, -(-Cout // 32) * 32
    rows = 25 * (k1 + k2) + 11 * k2 if up == 2 else 36 * (k1 + k2)
    out["bytes"] = {"V_written_and_read": 4 * rows * ntp, "M_written_and_read": 4 * 36 * co * ntp, "weights_read": 4 * rows * co,
                    "workspace": 4 * l.wmd_conv_wino44_workspace_floats(C.byref(a))}
    out["gate"] = {"a_error_le_5e-5": out.get("err_wino44", float("nan")) <= 5e-5,
                   "b_faster_than_today": out["wino44"]["median_us"] < out["today"]["median_us"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
