"""Time visualize.disparity_image on the GPU against the reference's chain on this machine's host (profiles/viz.md):
12 decoder maps of 192 x 640 to 375 x 1242 pictures in one call, and one map.

  * call time: device events around repeated calls that end in a synchronise, after a warm-up of the same shapes;
  * per launch: the library's own profile scopes (a device event pair around every launch), in a run of their own, with
    the bytes each launch has to move against the 8 TB/s HBM peak used throughout profiles/;
  * the comparison point: the device-to-host copy of the resized maps, then np.percentile + matplotlib per frame where
    matplotlib imports (tests/viz_ref.py otherwise), as KITTI/test_simple.py:166-172 does it.
No threshold is set on any of it.

    python tools/viz_microbench.py [--json FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from wavelet_monodepth_amd import _lib, ops, synth, visualize as viz

HBM = 8.0e12
h, w, H, W = 192, 640, 375, 1242


def host_chain():
    try:
        import matplotlib as mpl
        import matplotlib.cm as cm

        def one(x):
            vmax = np.percentile(x, 95)
            mapper = cm.ScalarMappable(norm=mpl.colors.Normalize(vmin=x.min(), vmax=vmax), cmap="magma")
            return (mapper.to_rgba(x)[:, :, :3] * 255).astype(np.uint8)
        return "numpy %s + matplotlib %s" % (np.__version__, mpl.__version__), one
    except ImportError:
        import viz_ref

        magma = viz_ref.table("magma")
        return "tests/viz_ref.py (numpy %s)" % np.__version__, lambda x: viz_ref.disparity_image(x, 95, magma)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    host_name, host_one = host_chain()
    result = {"shape": [h, w, H, W], "host_chain": host_name, "runs": []}
    for B in (12, 1):
        u = synth.uniform((B, h, w), "viz_bench", B, 0.0, 1.0)
        disp = torch.from_numpy((1.0 / (1.0 + 30.0 * u)).astype(np.float32)).to(dev)      # heavy-tailed, like a disparity map
        ws = torch.empty(_lib.lib().wmd_viz_workspace_bytes(B, H, W) // 4 + 1, device=dev, dtype=torch.int32)
        for _ in range(20):
            rgb = viz.disparity_image(disp, (H, W), workspace=ws)
        torch.cuda.synchronize()
        reps = 300 if B == 12 else 1000
        windows = []
        for _ in range(5):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                viz.disparity_image(disp, (H, W), workspace=ws)
            t1.record()
            torch.cuda.synchronize()
            windows.append(t0.elapsed_time(t1) / reps)
        _lib.profile_begin()
        for _ in range(20):
            viz.disparity_image(disp, (H, W), workspace=ws)
        recs = _lib.profile_end()
        launches = [{"kernel": r["kernel"], "us": r["ms"] / r["calls"] * 1e3, "bytes": r["bytes"] / r["calls"],
                     "hbm_floor_us": r["bytes"] / r["calls"] / HBM * 1e6, "share_of_hbm_peak": r["bytes"] / (r["ms"] * 1e-3) / HBM}
                    for r in recs]
        # the host chain on the same maps, from device memory: copy, then per frame
        resized = ops.upsample_bilinear(disp[:, None], (H, W))[:, 0].contiguous()
        torch.cuda.synchronize()
        host = []
        for _ in range(3):
            t = time.perf_counter()
            maps = resized.cpu().numpy()
            t_copy = time.perf_counter() - t
            pics = [host_one(m) for m in maps]
            host.append((time.perf_counter() - t, t_copy))
        same = bool(np.array_equal(np.stack(pics), rgb.cpu().numpy()))
        run = {"B": B, "call_ms_windows": windows, "call_ms": float(np.median(windows)), "launches": launches,
               "host_ms": min(t for t, _ in host) * 1e3, "host_copy_ms": min(c for _, c in host) * 1e3, "same_bytes_as_host_chain": same}
        result["runs"].append(run)
        print("B = %d: %.4f ms per call (windows %s), %.2f us per picture; host chain %.1f ms (copy %.2f ms), %.1f ms per picture; same bytes: %s"
              % (B, run["call_ms"], " ".join("%.4f" % v for v in windows), run["call_ms"] * 1e3 / B, run["host_ms"], run["host_copy_ms"],
                 run["host_ms"] / B, same))
        for r in launches:
            print("    %-32s %8.2f us  %9.0f bytes  floor %6.2f us  %5.1f %% of 8 TB/s" % (r["kernel"], r["us"], r["bytes"], r["hbm_floor_us"],
                                                                                           100 * r["share_of_hbm_peak"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
