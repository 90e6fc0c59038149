"""Time the KITTI training inputs (csrc/wmd_inputs.hip through kitti_inputs.preprocess) with device events beside the chain
they replace -- Pillow's resize / ImageEnhance / HSV hue shift and a float32 ToTensor, as MonoDataset.preprocess runs it --
on this machine's CPU: synthetic 375 x 1242 frames, three frames per sample, flip and jitter on for every sample.

    python tools/inputs_microbench.py [B ...]      # default: 12 1 samples per call

Per batch size and target size (640 x 192, 1024 x 320): the whole call (wrapper, allocations, the stack of the frames, five
launches and a memset) as the median and minimum of 50 calls after 5 warm-ups, the library's own per-launch times, and a byte
model over them: per frame the native image read once, every level written as uint8 and read back twice (by the next level
-- not the last -- and by the finishing launch) and 24 B per pixel of float32 planes.  The CPU rows need Pillow; without it
they are skipped and said so.  The CPU chain jitters and converts the native level too, as the reference does before it
deletes it."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

H0, W0 = 375, 1242
TARGETS = ((192, 640), (320, 1024))
FRAMES = 3


def frame(i):
    """a smooth scene with 5 % noise: what a photograph costs Pillow does not depend on the content, the hue branches do"""
    from wavelet_monodepth_amd import synth
    y, x = np.mgrid[0:H0, 0:W0].astype(np.float32)
    base = np.stack([128 + 100 * np.sin(x / (40 + 3 * i) + c) * np.cos(y / (55 + c)) for c in range(3)], axis=-1)
    return np.clip(base + synth.uniform((H0, W0, 3), "bench%d" % i, 0, -12.0, 12.0), 0, 255).astype(np.uint8)


def pil_chain(args):
    """one frame through the reference's chain: flip, four Lanczos levels, ColorJitter and ToTensor of the native image and of
    every level -> seconds"""
    from PIL import Image, ImageEnhance
    img, (h, w), order, factors, shift = args

    def hue(im):
        hh, s, v = im.convert("HSV").split()
        np_h = np.array(hh, dtype=np.uint8)
        with np.errstate(over="ignore"):
            np_h += np.uint8(shift)
        return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")

    ops = [lambda im: ImageEnhance.Brightness(im).enhance(factors[0]), lambda im: ImageEnhance.Contrast(im).enhance(factors[1]),
           lambda im: ImageEnhance.Color(im).enhance(factors[2]), hue]
    t0 = time.perf_counter()
    levels = [Image.fromarray(img, "RGB").transpose(Image.FLIP_LEFT_RIGHT)]
    for s in range(4):
        levels.append(levels[-1].resize((w >> s, h >> s), Image.LANCZOS))
    for im in levels:
        aug = im
        for op in order:
            aug = ops[op](aug)
        for v in (im, aug):
            np.ascontiguousarray((np.asarray(v).astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1))
    return time.perf_counter() - t0


def cpu_rows(frames, jit):
    try:
        import PIL
    except ImportError:
        print("Pillow is not installed on this machine: no CPU rows (the issue's 87 ms per frame is another machine's figure)")
        return {}
    import multiprocessing as mp
    workers = min(16, len(os.sched_getaffinity(0)))
    out = {}
    for hw in TARGETS:
        jobs = [(frames[i], hw, [int(v) for v in jit["order"][i // FRAMES]], [float(v) for v in jit["factors"][i // FRAMES]],
                 int(jit["hue_shift"][i // FRAMES])) for i in range(len(frames))]
        one = [pil_chain(j) for j in jobs[:12]]
        with mp.get_context("spawn").Pool(workers) as pool:
            pool.map(pil_chain, jobs[:workers])                      # start the workers and their imports
            t0 = time.perf_counter()
            pool.map(pil_chain, jobs, chunksize=1)
            wall = time.perf_counter() - t0
        out[hw] = (1e3 * float(np.median(one)), 1e3 * wall / len(jobs))
        print("CPU, Pillow %s, %dx%d -> %dx%d: %.1f ms per frame on one thread (median of %d frames, min %.1f); %d frames over a pool "
              "of %d processes: %.2f ms per frame of wall time" % (PIL.__version__, W0, H0, hw[1], hw[0], out[hw][0], len(one), 1e3 * min(one),
                                                                    len(jobs), workers, out[hw][1]))
    return out


def timed(fn, torch, reps=50, warm=5):
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
    sizes = [int(v) for v in sys.argv[1:]] or [12, 1]
    import inputs_cases
    n = max(sizes) * FRAMES
    frames = np.stack([frame(i) for i in range(n)])
    jit = inputs_cases.random_jitter("bench", max(sizes), 1)
    cpu = cpu_rows(frames, jit)                                      # before the GPU is opened: the pool's processes never see it
    import torch
    import inputs_ref as R
    from wavelet_monodepth_amd import _lib, kitti_inputs as ki
    dev = torch.device("cuda:0")
    for B in sizes:
        by_id = {f: torch.from_numpy(frames[k:B * FRAMES:FRAMES].copy()).to(dev) for k, f in enumerate((0, -1, 1))}
        flip = torch.ones(B, dtype=torch.uint8, device=dev)
        params = ki.ColorJitterParams(jit["enable"][:B], jit["order"][:B], jit["factors"][:B], jit["hue_shift"][:B]).to(dev)
        for h, w in TARGETS:
            fn = lambda: ki.preprocess(by_id, h, w, range(4), flip, params)
            got = fn()
            want = R.jitter(R.pyramid(frames[0], h, w, 2, True)[1], jit["order"][0], jit["factors"][0], jit["hue_shift"][0])
            same = np.array_equal(got[("color_aug", 0, 1)][0].cpu().numpy(), R.to_tensor(want))
            med, best = timed(fn, torch)
            _lib.profile_begin()
            for _ in range(10):
                fn()
            rows = _lib.profile_end()
            kern_ms = sum(r["ms"] for r in rows) / 10
            kern = ", ".join("%s x%d %.1f us" % (r["kernel"].replace("_kernel", ""), r["calls"] // 10, r["ms"] / 10 * 1e3) for r in rows)
            N = B * FRAMES
            px = [(h >> s) * (w >> s) for s in range(4)]
            model = N * (3.0 * H0 * W0 + 30.0 * sum(px) + 3.0 * sum(px[:3]))
            line = ("B=%2d x %d frames -> %dx%d: %.3f ms per call (min %.3f) = %.1f us per frame; kernels %.3f ms (%s); model %.1f MB -> %.0f GB/s "
                    "over the kernels; equals the oracle: %s" % (B, FRAMES, w, h, med, best, 1e3 * med / N, kern_ms, kern, model / 1e6,
                                                                 model / kern_ms / 1e6, same))
            if (h, w) in cpu:
                line += "; CPU one thread / GPU per frame %.0fx, CPU pool / GPU per frame %.0fx" % (cpu[(h, w)][0] / (med / N), cpu[(h, w)][1] / (med / N))
            print(line)


if __name__ == "__main__":
    main()
