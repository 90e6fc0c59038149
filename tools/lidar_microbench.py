"""Time the LiDAR depth maps (csrc/wmd_lidar.hip through kitti_utils.project_lidar) with hipEvents beside the float64 numpy
oracle (tests/lidar_ref.py) on this machine's CPU: synthetic 120 000-point ring scans at 375 x 1242.

    python tools/lidar_microbench.py [B ...]      # default: 1 8 64 scans per call

Per batch size: the whole call (workspace allocation, three launches) per scan, the library's own per-kernel times, and the
byte model of DESIGN.md -- per scan 2 x (8 B per pixel + 16 B per sub2ind bucket) for the initialisation and the resolve,
4 B per pixel written, 16 B per point read -- over the measured time.  The CPU column is one oracle call per scan."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import lidar_cases
import lidar_ref
from wavelet_monodepth_amd import _lib, kitti_utils as ku

dev = torch.device("cuda:0")
H, W = 375, 1242


def timed(fn, reps=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0]


def main():
    sizes = [int(v) for v in sys.argv[1:]] or [1, 8, 64]
    case = lidar_cases.build(lidar_cases.FULL)
    P = case["P"]
    scans = [lidar_cases._rings(np.random.default_rng(1000 + i)) for i in range(max(sizes))]
    cpu = []
    for s in scans[:8]:
        for vel in (False, True):
            t0 = time.perf_counter()
            lidar_ref.depth_map(s, P, (H, W), vel)
            cpu.append(time.perf_counter() - t0)
    cpu_ms = 1e3 * float(np.median(cpu))
    print("CPU oracle (numpy, float64): %.2f ms per scan (median of %d calls, min %.2f ms)" % (cpu_ms, len(cpu), 1e3 * min(cpu)))
    for B in sizes:
        pts = torch.from_numpy(np.concatenate(scans[:B])).to(dev)
        offsets = torch.from_numpy(np.arange(B + 1, dtype=np.int64) * len(scans[0])).to(dev)
        Pb = torch.from_numpy(P)[None].repeat(B, 1, 1).to(dev)
        for vel in (False, True):
            fn = lambda: ku.project_lidar(pts, Pb, (H, W), vel, offsets)
            out = fn().cpu().numpy()
            same = all(np.array_equal(out[b], lidar_ref.depth_map(scans[b], P, (H, W), vel).astype(np.float32)) for b in range(min(B, 2)))
            med, best = timed(fn)
            _lib.profile_begin()
            for _ in range(10):
                fn()
            rows = _lib.profile_end()
            kern = ", ".join("%s %.1f us" % (r["kernel"].replace("lidar_", "").replace("_kernel", ""), r["ms"] / r["calls"] * 1e3) for r in rows)
            kern_ms = sum(r["ms"] / r["calls"] for r in rows)
            nk = H * (W - 1) + 1
            model = B * (2.0 * (8 * H * W + 16 * nk) + 4 * H * W + 16 * len(scans[0]))
            print("B=%2d vel_depth=%d: %.3f ms per call (min %.3f) = %.1f us per scan; kernels %.3f ms (%s); model %.1f MB -> %.0f GB/s "
                  "over the kernels; CPU / GPU per scan %.0fx; equals the oracle: %s"
                  % (B, vel, med, best, 1e3 * med / B, kern_ms, kern, model / 1e6, model / kern_ms / 1e6, cpu_ms / (med / B), same))


if __name__ == "__main__":
    main()
