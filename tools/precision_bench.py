"""Trunk precision modes side by side: fp32 (default), bf16x3 and bf16 (DepthWaveProgressiveDecoder.set_precision).

  python tools/precision_bench.py [--steps 50] [--warmup 10] [--passes 3] [--configs r18,r50]

Per configuration (r18: KITTI ResNet18 640x192 batch 12 = config 2; r50: ResNet50 1024x320 batch 8) one decoder per mode,
graph replay, the protocol of bench.py's headline (set-up forward + 30 replays, `warmup` replays, `steps` timed replays
between synchronisations), the three modes ALTERNATED in one process for `passes` passes.  Then, per mode, the trunk
kernels' per-launch times from the library profiler (eager forwards, launch order = layer order) with mfma_flops / time as
a share of the bf16 (fp32 for the fp32 mode) matrix peak and the layer's fp32 tensor bytes / time as a share of 8 TB/s, and
the parity of frame 0 of the timed mode's output against the CPU oracle.  Needs the GPU; there is no fallback."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from oracle import decoder_ref as R
from wavelet_monodepth_amd import _lib, synth, tuner
from wavelet_monodepth_amd.kitti import DepthWaveProgressiveDecoder

MODES = ("fp32", "bf16x3", "bf16")
CONFIGS = {"r18": ([64, 64, 128, 256, 512], 12, 192, 640), "r50": ([64, 256, 512, 1024, 2048], 8, 320, 1024)}
PEAK_BF16, PEAK_FP32, PEAK_HBM = 2.5e15, 157.3e12, 8.0e12     # dense matrix peaks (FLOP/s) and HBM bytes/s of one MI355X
LAYERS = [("upconv", i, j) for i in (4, 3, 2, 1) for j in (0, 1)]


def is_trunk(name):
    return name.startswith(("conv_bf16_kernel<", "conv_wino")) or (name.startswith("conv_fwd_kernel<") and name.endswith(",9>"))


def timed(dec, feats, steps, warmup):
    with torch.no_grad():
        for _ in range(warmup):
            dec(feats)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            dec(feats)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def per_layer(dec, feats, reps=5):
    """-> [(kernel, us, flops, mfma_flops, bytes)] of the eight trunk launches, best of `reps` profiled eager forwards.  The
    profiler aggregates by kernel name, so each layer is profiled on its own: one forward per layer with a hook pair."""
    out = []
    with torch.no_grad(), dec.eager():
        dec(feats)
        for key in LAYERS:
            mod = dec.convs[key]
            best = None
            for _ in range(reps):
                h0 = mod.register_forward_pre_hook(lambda m, a: _lib.profile_begin())
                got = []
                h1 = mod.register_forward_hook(lambda m, a, o: got.append(_lib.profile_end()))
                dec(feats)
                h0.remove()
                h1.remove()
                recs = got[0]
                ms = sum(r["ms"] for r in recs)
                main = [r for r in recs if is_trunk(r["kernel"])]
                assert len(main) == 1, recs
                if best is None or ms < best[1]:
                    best = (main[0]["kernel"] + ("" if len(recs) == 1 else " + " + " + ".join(r["kernel"] for r in recs if r is not main[0])),
                            ms, main[0]["flops"], main[0]["mfma_flops"], main[0]["bytes"])
            out.append(best)
    return out


def parity(out, feats, sd):
    ref = R.kitti_wave_decoder([f[:1].cpu() for f in feats], sd)
    worst = 0.0
    for k, v in ref.items():
        worst = max(worst, float((out[k][:1].cpu() - v).abs().max() / v.abs().max().clamp_min(1e-30)))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--configs", default="r18,r50")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("precision_bench.py needs the MI355X: there is no CPU or fp32 fallback")
    dev = torch.device("cuda:0")
    _lib.lib()
    tuner.preload(os.path.join(ROOT, "profiles", "r06_tune_cache.json"))     # the fp32 mode as bench.py runs it
    try:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        commit = "unknown"
    print("# trunk precision modes, commit %s, %s, steps %d warmup %d passes %d" % (commit, torch.cuda.get_device_name(0), args.steps, args.warmup, args.passes))
    for cname in args.configs.split(","):
        chans, B, H, W = CONFIGS[cname]
        feats = [torch.from_numpy(f).to(dev) for f in synth.encoder_features(B, H, W, chans, seed=1)]
        decs = {}
        for m in MODES:
            dec = synth.fill_state_dict(DepthWaveProgressiveDecoder(np.array(chans)), seed=1).to(dev).set_precision(m)
            dec.enable_graph(True)
            with torch.no_grad():
                for _ in range(31):
                    dec(feats)
            decs[m] = dec
        sd = {k: v.detach().cpu() for k, v in decs["fp32"].state_dict().items()}
        steps = {m: [] for m in MODES}
        for _ in range(args.passes):
            for m in MODES:
                steps[m].append(timed(decs[m], feats, args.steps, args.warmup))
        print("\n## %s: %s %dx%d batch %d, graph replay" % (cname, chans, W, H, B))
        print("| mode | step ms (passes) | parity of frame 0 vs fp32 oracle (worst plane max_rel) | report |")
        print("|---|---|---|---|")
        layers = {}
        for m in MODES:
            with torch.no_grad():
                out = decs[m](feats)
            rep = sorted(set(decs[m].trunk_precision_report().values()))
            print("| %s | %s | %.3e | %s |" % (m, " / ".join("%.4f" % v for v in steps[m]), parity(out, feats, sd), ",".join(rep)))
            layers[m] = per_layer(decs[m], feats)
        print("\n| layer | " + " | ".join("%s us (kernel)" % m for m in MODES) + " | " +
              " | ".join("%s: %% matrix peak / %% of 8 TB/s -> nearer bound" % m for m in MODES) + " |")
        print("|---|" + "---|" * (2 * len(MODES)))
        for n, key in enumerate(LAYERS):
            cells, shares = [], []
            for m in MODES:
                kern, ms, flops, mfma, nbytes = layers[m][n]
                peak = PEAK_FP32 if m == "fp32" else PEAK_BF16
                pm, pb = mfma / (ms * 1e-3) / peak, nbytes / (ms * 1e-3) / PEAK_HBM
                cells.append("%.1f (%s)" % (ms * 1e3, kern))
                shares.append("%.1f / %.1f -> %s" % (100 * pm, 100 * pb, "matrix" if pm > pb else "memory"))
            print("| %s | " % (key,) + " | ".join(cells) + " | " + " | ".join(shares) + " |")
        tot = {m: sum(l[1] for l in layers[m]) for m in MODES}
        print("| trunk total | " + " | ".join("%.1f" % (tot[m] * 1e3) for m in MODES) + " |" + " |" * len(MODES))
        print(json.dumps({"config": cname, "commit": commit, "step_ms": steps, "trunk_us": {m: round(tot[m] * 1e3, 1) for m in MODES}}))
        del decs


if __name__ == "__main__":
    main()
