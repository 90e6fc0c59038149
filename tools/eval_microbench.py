"""Time the evaluation chain on a KITTI-sized batch (development aid): 16 images, 192x640 predictions, 375x1242 ground truth;
then the NYUv2 depth-boundary errors on 2 and 32 images of 440x592 (profiles/dbe.md)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from wavelet_monodepth_amd import _lib, evaluation as ev

dev = torch.device("cuda:0")
B = 16
disp = torch.rand(B, 192, 640, device=dev) * 0.3 + 0.01
gt = torch.rand(B, 375, 1242, device=dev) * 90
gt[torch.rand_like(gt) < 0.7] = 0
for _ in range(3):
    ev.kitti_metrics(disp, gt)
torch.cuda.synchronize()
_lib.profile_begin()
for _ in range(10):
    ev.kitti_metrics(disp, gt)
recs = _lib.profile_end()
tot = sum(r["ms"] for r in recs) / 10
print("kitti_metrics batch %d: %.3f ms (%.1f us / image): %s" % (B, tot, tot * 1e3 / B, ", ".join(
    "%s %.1f us %.0f GB/s" % (r["kernel"], r["ms"] / r["calls"] * 1e3, r["bytes"] / r["ms"] / 1e6) for r in recs)))
l, r = torch.rand(B, 192, 640, device=dev), torch.rand(B, 192, 640, device=dev)
for _ in range(3):
    ev.flip_postprocess(l, r)
torch.cuda.synchronize()
_lib.profile_begin()
for _ in range(10):
    ev.flip_postprocess(l, r)
recs = _lib.profile_end()
print(", ".join("%s %.1f us %.0f GB/s" % (r["kernel"], r["ms"] / r["calls"] * 1e3, r["bytes"] / r["ms"] / 1e6) for r in recs))

# dbe: the NYUv2 depth-boundary errors at the Eigen crop of 480 x 640 -- device events around repeated calls (each ends in a
# synchronise), the per-kernel split from the library's own profile, and tests/dbe_ref.py (numpy + scipy, one image at a
# time as the reference works) on this machine's CPU for the same inputs
import time

import numpy as np

sys.path.insert(0, os.path.join(ROOT, "tests"))
import dbe_cases

H, W = dbe_cases.FULL
base_pred, base_gt = dbe_cases.scenes(4, H, W, "bench", 40)
for B in (2, 32):
    pred = torch.from_numpy(np.concatenate([base_pred] * (B // 4 + 1))[:B]).to(dev)
    gt = torch.from_numpy(np.concatenate([base_gt] * (B // 4 + 1))[:B]).to(dev)
    for _ in range(5):
        scores, edges = ev.compute_depth_boundary_error(gt, pred)
    torch.cuda.synchronize()
    reps = 2000 if B == 2 else 400
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        ev.compute_depth_boundary_error(gt, pred)
    t1.record()
    torch.cuda.synchronize()
    call_ms = t0.elapsed_time(t1) / reps
    _lib.profile_begin()
    for _ in range(10):
        ev.compute_depth_boundary_error(gt, pred)
    recs = _lib.profile_end()
    print("dbe batch %d at %dx%d: %.3f ms per call (%.1f us / image, %d calls, %d edge pixels); kernels: %s" % (
        B, H, W, call_ms, call_ms * 1e3 / B, reps, int(edges.sum()),
        ", ".join("%s %.1f us" % (r["kernel"], r["ms"] / r["calls"] * 1e3) for r in recs)))
try:
    import dbe_ref
except ImportError as e:
    print("dbe_ref on the CPU: not measured (%s)" % e)
else:
    t = time.perf_counter()
    for b in range(4):
        dbe_ref.compute_depth_boundary_error(base_gt[b], base_pred[b])
    print("dbe_ref (numpy + scipy.ndimage) on this machine's CPU: %.1f ms / image at %dx%d" % ((time.perf_counter() - t) * 250, H, W))
