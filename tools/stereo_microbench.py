"""Time the semi-global matcher (csrc/wmd_stereo.hip) per stage, for the twelve reference settings.

    python tools/stereo_microbench.py [--json out.json] [--reps 10] [H W B ...]     # default: 320 1024 1, 320 1024 12, 192 640 1, 192 640 12

"call" is the median of `reps` calls of stereo.sgbm between two device events, Python wrapper and workspace allocation
included.  The per-stage times are the library's own per-launch timing (wmd_profile_begin / end) over `reps` further calls:
kernels only.  Bytes are the model of DESIGN.md, computed from the layout (n = H Wv D elements of the uint16 volumes):
cost 2 n written; aggregation 4 n for the first direction (read C, write S) and 6 n for every other (read C, read and write
S); winner 2 n read.  GB/s = model bytes / stage time.  blockSize 2 and 3 are the same window, hence the same work; both
are listed.  The inputs are a smoothed random texture and the same texture displaced by 3..40 pixels, growing down the image,
plus noise; the B images of a batch are rolled copies, and the tool checks that image 0 of the batch equals the B = 1 map."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from wavelet_monodepth_amd import _lib, stereo

dev = torch.device("cuda:0")


def inputs(B, H, W):
    g = torch.Generator(device="cpu").manual_seed(7)
    tex = torch.rand(1, 3, H, W + 64, generator=g)
    tex = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(tex, (1, 1, 1, 1), mode="replicate"), 3, 1)[0]
    left = tex[:, :, :W]
    shift = (3 + 37 * torch.arange(H) // H).tolist()
    right = torch.stack([tex[:, y, s:s + W] for y, s in enumerate(shift)], dim=1)
    right = (right + 0.02 * torch.rand(3, H, W, generator=g)).clamp(0, 1)
    to_u8 = lambda t: (t * 255).round().to(torch.uint8).permute(1, 2, 0)
    l, r = to_u8(left), to_u8(right)
    ls = torch.stack([torch.roll(l, 3 * b, 0) for b in range(B)])
    rs = torch.stack([torch.roll(r, 3 * b, 0) for b in range(B)])
    return ls.contiguous().to(dev), rs.contiguous().to(dev), torch.tensor(shift)


def timed(fn, reps, warm=3):
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


STAGES = (("prep", ("stereo_prep_kernel",)), ("cost", ("stereo_cost_kernel",)), ("paths", ("stereo_path_kernel",)),
          ("winner", ("stereo_winner_kernel",)), ("finish", ("stereo_finish_kernel",)),
          ("speckles", ("speckle_init_kernel", "speckle_merge_kernel", "speckle_count_kernel", "speckle_clear_kernel")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("sizes", nargs="*", type=int)
    opt = ap.parse_args()
    sizes = [tuple(opt.sizes[i:i + 3]) for i in range(0, len(opt.sizes), 3)] or [(320, 1024, 1), (320, 1024, 12), (192, 640, 1), (192, 640, 12)]
    rows, single = [], {}
    for H, W, B in sizes:
        left, right, shift = inputs(B, H, W)
        for s in stereo.reference_settings():
            D = s.numDisparities
            n = B * H * (W - D) * D
            fn = lambda: stereo.sgbm(left, right, s)
            disp = fn()
            call, call_min = timed(fn, opt.reps)
            _lib.profile_begin()
            for _ in range(opt.reps):
                fn()
            prof = {r["kernel"]: r["ms"] / opt.reps for r in _lib.profile_end()}   # ms per call, all launches of that kernel
            stage = {name: sum(prof.get(k, 0.0) for k in kernels) for name, kernels in STAGES}
            model = {"cost": 2.0 * n, "paths": (4.0 + 6.0 * (s.directions - 1)) * n, "winner": 2.0 * n}
            gbs = {k: model[k] / stage[k] / 1e6 for k in model if stage[k] > 0}
            # sanity at the timed size: the valid share and the share of valid pixels within half a pixel of the truth, image 0
            d0 = disp[0].cpu()
            rect = d0[:, D:].to(torch.float32) / 16
            valid = rect >= 0
            near = ((rect - shift[:, None].float()).abs() <= 0.5) & valid
            key = (H, W, s)
            if B == 1:
                single[key] = d0
            same = None if key not in single or B == 1 else bool(torch.equal(single[key], d0))
            row = {"H": H, "W": W, "B": B, "blockSize": s.blockSize, "numDisparities": D, "call_ms": call, "call_min_ms": call_min,
                   "stage_ms": stage, "kernel_ms": prof, "model_MB": {k: v / 1e6 for k, v in model.items()}, "model_GBs": gbs,
                   "valid": float(valid.float().mean()), "near_of_valid": float(near.sum()) / max(int(valid.sum()), 1), "equals_b1": same}
            rows.append(row)
            print("%dx%d B=%d block=%d D=%d: call %.3f ms (min %.3f) | %s | kernels %.3f ms | model GB/s %s | valid %.1f %%, within 0.5 px %.1f %%%s"
                  % (H, W, B, s.blockSize, D, call, call_min, " ".join("%s %.3f" % (k, stage[k]) for k, _ in STAGES), sum(stage.values()),
                     " ".join("%s %.0f" % (k, v) for k, v in gbs.items()), 100 * row["valid"], 100 * row["near_of_valid"],
                     "" if same is None else ", image 0 equals the B=1 map: %s" % same), flush=True)
    if opt.json:
        with open(opt.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
