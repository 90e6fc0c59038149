"""Time the depth-hint fusion (one launch, csrc/wmd_hints.hip) against the composition of the operators it replaces
(photometric.warp_frame on M-fold expanded inputs, compute_reprojection_loss, torch.argmin, torch.gather) with hipEvents.

    python tools/hints_microbench.py [B M H W ...]      # default: 1 12 320 1024, 1 12 192 640, 8 12 192 640

Bytes are the model of DESIGN.md: fused 4 M + 12 + 8 per pixel (candidates once, base image once, two outputs; the lookup
gathers hit L2); the GB/s column is that model over the measured time."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from wavelet_monodepth_amd import _lib, depth_hints as dh, photometric as ph

dev = torch.device("cuda:0")


def inputs(B, M, H, W):
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + M)
    base = torch.rand(B, 3, H, W, generator=g)
    base = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(base, (1, 1, 1, 1), mode="replicate"), 3, 1)
    lookup = (torch.roll(base, 5, -1) + 0.02 * torch.rand(B, 3, H, W, generator=g)).clamp(0, 1)
    disp = (torch.rand(B, M, H, W, generator=g) * 60 * 16).round() / 16
    disp[torch.rand(B, M, H, W, generator=g) < 0.15] = 0
    K = torch.tensor([[0.58 * W, 0, 0.5 * W, 0], [0, 1.92 * H, 0.5 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1]]).repeat(B, 1, 1)
    T = torch.eye(4).repeat(B, 1, 1)
    T[:, 0, 3] = 0.1
    T[1::2, 0, 3] = -0.1
    return [t.to(dev).contiguous() for t in (disp, base, lookup, K, torch.linalg.inv(K), T)]


def composition(depths, base, lookup, K, inv_K, T):
    B, M, H, W = depths.shape
    rep = lambda t: t[:, None].expand(B, M, *t.shape[1:]).reshape(B * M, *t.shape[1:])
    warped = ph.warp_frame(rep(lookup), depths.reshape(B * M, 1, H, W), rep(K), rep(inv_K), rep(T))
    losses = ph.compute_reprojection_loss(warped, rep(base)).view(B, M, H, W)
    index = torch.argmin(losses, dim=1, keepdim=True)
    return torch.gather(depths, 1, index), index


def timed(fn, reps=100, warm=10):
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
    args = [int(v) for v in sys.argv[1:]]
    shapes = [tuple(args[i:i + 4]) for i in range(0, len(args), 4)] or [(1, 12, 320, 1024), (1, 12, 192, 640), (8, 12, 192, 640)]
    for B, M, H, W in shapes:
        disp, base, lookup, K, inv_K, T = inputs(B, M, H, W)
        fbl = float(K[0, 0, 0]) * 0.1
        depths = dh.disparity_to_depth(disp, float(K[0, 0, 0]))
        fused = lambda: dh.fuse_depth_hints(disp, base, lookup, K, inv_K, T, disparities=True, focal_times_baseline=fbl)
        comp = lambda: composition(depths, base, lookup, K, inv_K, T)
        d1, _ = fused()
        d2, _ = comp()
        same = float((d1 == d2).float().mean())
        tf, tf_min = timed(fused)
        tc, tc_min = timed(comp)
        kern = {}
        for tag, fn in (("fused", fused), ("composition", comp)):   # the library's own per-launch timing: kernels only, no gaps
            _lib.profile_begin()
            for _ in range(10):
                fn()
            kern[tag] = ", ".join("%s %.1f us" % (r["kernel"], r["ms"] / r["calls"] * 1e3) for r in _lib.profile_end())
        print("   library kernels -- fused: %s; composition (argmin and gather are torch's): %s" % (kern["fused"], kern["composition"]))
        model = B * H * W * (4.0 * M + 12 + 8)
        print("B=%d M=%d %dx%d: fused %.3f ms (min %.3f), composition %.3f ms (min %.3f), ratio %.2fx; model %.1f MB -> %.0f GB/s; "
              "hints equal at %.2f %% of the pixels" % (B, M, H, W, tf, tf_min, tc, tc_min, tc / tf, model / 1e6, model / tf / 1e6, 100 * same))


if __name__ == "__main__":
    main()
