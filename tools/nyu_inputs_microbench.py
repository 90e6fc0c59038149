"""Time the NYUv2 training inputs (csrc/wmd_nyu_inputs.hip through nyu_inputs.train_transform) with device events beside the
chain they replace -- Pillow's transpose / point / crop / two bicubic resizes and the float32 conversions, as
getDefaultTrainTransform runs them -- on this machine's CPU: synthetic 480 x 640 samples, flip, swap and gamma on for every
sample.

    python tools/nyu_inputs_microbench.py [B ...]      # default: 8 1 samples per call (NYUv2/train.py's --bs default is 8)

Per batch size and mode (the default sizes 640 x 480 / 320 x 240, and is_224): the whole call (wrapper, three allocations, one
launch) as the median and minimum of 50 calls after 5 warm-ups, the library's own per-launch time, and a byte model over it:
per sample the crop box of the image and of the depth map read once (4 B per box pixel), 12 B per image pixel and 8 B per depth
pixel (depth and disp_gt) written.  Tile halos re-read from cache are not in the model.  The CPU rows need Pillow; without it
they are skipped and said so."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

H0, W0, CROP = 480, 640, 16
MODES = (("default", (480, 640), (240, 320)), ("is_224", (224, 224), (224, 224)))
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


def sample(i):
    """a smooth scene with 5 % noise and a smooth depth map: what the chain costs does not depend on the content"""
    from wavelet_monodepth_amd import synth
    y, x = np.mgrid[0:H0, 0:W0].astype(np.float32)
    base = np.stack([128 + 100 * np.sin(x / (40 + 3 * i) + c) * np.cos(y / (55 + c)) for c in range(3)], axis=-1)
    image = np.clip(base + synth.uniform((H0, W0, 3), "nyubench%d" % i, 0, -12.0, 12.0), 0, 255).astype(np.uint8)
    depth = np.clip(30 + 200 * (y / H0) * (0.6 + 0.4 * np.cos(x / (90 + i))), 0, 255).astype(np.uint8)
    return image, depth


def pil_chain(args):
    """one sample through the reference's chain -> seconds"""
    from PIL import Image
    image, depth, perm, gamma, (ih, iw), (dh, dw) = args
    t0 = time.perf_counter()
    im, de = Image.fromarray(image, "RGB"), Image.fromarray(depth, "L")
    im, de = im.transpose(Image.FLIP_LEFT_RIGHT), de.transpose(Image.FLIP_LEFT_RIGHT)
    im = Image.fromarray(np.asarray(im)[..., list(PERMS[perm])])
    im = im.point([(255 + 1 - 1e-3) * pow(e / 255., gamma) for e in range(256)] * 3)
    box = (CROP, CROP, W0 - CROP, H0 - CROP)
    im, de = im.crop(box).resize((iw, ih)), de.crop(box).resize((dw, dh))
    np.ascontiguousarray((np.asarray(im).astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1))
    d = np.clip(np.asarray(de).astype(np.float32) / np.float32(255.0) * np.float32(1000.0), 10, 1000)[None]
    np.float32(10.0) / d
    return time.perf_counter() - t0


def cpu_rows(images, depths, perm, gammas):
    try:
        import PIL
    except ImportError:
        print("Pillow is not installed on this machine: no CPU rows")
        return {}
    import multiprocessing as mp
    workers = min(16, len(os.sched_getaffinity(0)))
    out = {}
    for mode, isz, dsz in MODES:
        jobs = [(images[i % len(images)], depths[i % len(images)], int(perm[i % len(images)]), float(gammas[i % len(images)]), isz, dsz)
                for i in range(max(64, len(images)))]
        one = [pil_chain(j) for j in jobs[:16]]
        with mp.get_context("spawn").Pool(workers) as pool:
            pool.map(pil_chain, jobs[:workers])                      # start the workers and their imports
            t0 = time.perf_counter()
            pool.map(pil_chain, jobs, chunksize=1)
            wall = time.perf_counter() - t0
        out[mode] = (1e3 * float(np.median(one)), 1e3 * wall / len(jobs))
        print("CPU, Pillow %s, %s: %.2f ms per sample on one thread (median of %d samples, min %.2f); %d samples over a pool of %d "
              "processes: %.3f ms per sample of wall time" % (PIL.__version__, mode, out[mode][0], len(one), 1e3 * min(one), len(jobs), workers,
                                                              out[mode][1]))
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
    sizes = [int(v) for v in sys.argv[1:]] or [8, 1]
    n = max(sizes)
    pairs = [sample(i) for i in range(n)]
    images, depths = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    perm = 1 + np.arange(n) % 5
    gammas = np.linspace(0.8, 1.25, n) if n > 1 else np.array([0.8])
    cpu = cpu_rows(images, depths, perm, gammas)                     # before the GPU is opened: the pool's processes never see it
    import torch
    import nyu_inputs_ref as R
    from wavelet_monodepth_amd import _lib, nyu_inputs as ni
    dev = torch.device("cuda:0")
    for B in sizes:
        image, depth = torch.from_numpy(images[:B]).to(dev), torch.from_numpy(depths[:B]).to(dev)
        aug = ni.Augmentation(np.ones(B, np.uint8), perm[:B], np.stack([ni.gamma_lut(g) for g in gammas[:B]])).to(dev)
        for mode, isz, dsz in MODES:
            fn = lambda: ni.train_transform(image, depth, aug, image_size=isz, depth_size=dsz, disparity=True)
            got = fn()
            wi, wd = R.item(images[0], depths[0], CROP, isz, dsz, 1, perm[0], R.gamma_lut(gammas[0]))
            same = np.array_equal(got["image"][0].cpu().numpy(), R.image_tensor(wi)) and np.array_equal(got["depth"][0].cpu().numpy(), R.depth_tensor(wd))
            med, best = timed(fn, torch)
            _lib.profile_begin()
            for _ in range(10):
                fn()
            rows = _lib.profile_end()
            kern_ms = sum(r["ms"] for r in rows) / 10
            kern = ", ".join("%s x%d %.1f us" % (r["kernel"].replace("_kernel", ""), r["calls"] // 10, r["ms"] / 10 * 1e3) for r in rows)
            model = B * (4.0 * (H0 - 2 * CROP) * (W0 - 2 * CROP) + 12.0 * isz[0] * isz[1] + 8.0 * dsz[0] * dsz[1])
            line = ("B=%2d %-7s: %.3f ms per call (min %.3f) = %.1f us per sample; kernel %.3f ms (%s); model %.1f MB -> %.0f GB/s over the kernel; "
                    "equals the oracle: %s" % (B, mode, med, best, 1e3 * med / B, kern_ms, kern, model / 1e6, model / kern_ms / 1e6, same))
            if mode in cpu:
                line += "; CPU one thread / GPU per sample %.0fx, CPU pool / GPU per sample %.0fx" % (cpu[mode][0] / (med / B), cpu[mode][1] / (med / B))
            print(line)


if __name__ == "__main__":
    main()
