"""The named cases of the KITTI training inputs (kitti_inputs.color_pyramid / color_jitter).  Everything is drawn from
wavelet_monodepth_amd.synth, so tests/golden/inputs_reference.npz stores outputs only.

    build(name) -> dict(frames uint8 [N,H0,W0,3], height, width, num_scales, flip uint8 [N], jitter None or
                        dict(enable uint8 [N], order uint8 [N,4], factors float32 [N,3], hue_shift int32 [N]))
"""
import itertools

import numpy as np

from wavelet_monodepth_amd import synth

PERMS = [list(p) for p in itertools.permutations(range(4))]   # 24 orders of 0 brightness, 1 contrast, 2 saturation, 3 hue


def image(name, shape, seed=0, binary=False):
    u = synth.uniform(tuple(shape), name, seed, 0.0, 256.0)
    img = np.minimum(np.floor(u), 255).astype(np.uint8)
    return np.where(img >= 128, 255, 0).astype(np.uint8) if binary else img


def random_jitter(name, n, seed=0, enable=None, perms=None):
    """factors in [0.8, 1.2), hue in [-0.1, 0.1) -> shift = int(hue 255) mod 256, orders from `perms` (indices into PERMS)"""
    f = synth.uniform((n, 3), name + ".factors", seed, 0.8, 1.2)
    h = synth.uniform((n,), name + ".hue", seed, -0.1, 0.1)
    if perms is None:
        perms = (synth.uniform((n,), name + ".perm", seed, 0.0, 24.0)).astype(np.int64) % 24
    return dict(enable=np.ones(n, np.uint8) if enable is None else np.asarray(enable, np.uint8),
                order=np.array([PERMS[int(p)] for p in perms], np.uint8), factors=f.astype(np.float32),
                hue_shift=np.array([int(float(v) * 255) % 256 for v in h], np.int32))


def _half_image(h, w):
    """grey mean exactly 10.5: the contrast mean must round to 11 (int(mean + 0.5))"""
    img = np.full((h, w, 3), 10, np.uint8)
    img[h // 2:] = 11
    return img


def _orders(edges):
    """26 items of 12 x 20: the 24 orders, one disabled item between them (5) and the half 10 / half 11 image last"""
    n = 26
    perms = list(range(5)) + [0] + list(range(5, 24)) + [PERMS.index([1, 0, 2, 3])]
    enable = np.ones(n, np.uint8)
    enable[5] = 0
    frames = image("orders", (n, 12, 20, 3), 3)
    frames[25] = _half_image(12, 20)
    j = random_jitter("orders", n, 4, enable, perms)
    if edges:
        vals = np.array([0.8, 1.0, 1.2], np.float32)
        i = np.arange(n)
        j["factors"] = np.stack([vals[i % 3], vals[(i // 3) % 3], vals[(i // 9) % 3]], axis=1)
        j["hue_shift"] = np.array([0, 25, 231], np.int32)[(i + i // 3) % 3]
    j["factors"][25] = (1.0, 0.8, 1.0)
    return dict(frames=frames, height=12, width=20, num_scales=1, flip=np.zeros(n, np.uint8), jitter=j)


def build(name):
    if name == "ratio_47x161":       # non-integer ratios, 483-byte rows, mixed flips, one item without jitter
        n = 5
        return dict(frames=image(name, (n, 47, 161, 3), 1), height=24, width=80, num_scales=4,
                    flip=np.array([0, 1, 1, 0, 1], np.uint8), jitter=random_jitter(name, n, 2, [1, 0, 1, 1, 1]))
    if name == "clip_5x7":           # the window is wider than the image on both axes
        return dict(frames=image(name, (2, 5, 7, 3), 1), height=2, width=3, num_scales=1, flip=np.array([0, 1], np.uint8), jitter=None)
    if name == "upscale_10x14":
        return dict(frames=image(name, (2, 10, 14, 3), 1), height=16, width=24, num_scales=1, flip=np.array([1, 0], np.uint8), jitter=None)
    if name == "saturate_48x64":     # 0 / 255 only, per pixel and in 16 x 16 blocks: the overshoot at the blocks' edges runs into clip8
        frames = image(name, (3, 48, 64, 3), 1, binary=True)
        frames[1:] = np.kron(image(name + ".blocks", (2, 3, 4, 3), 1, binary=True), np.ones((1, 16, 16, 1), np.uint8))
        return dict(frames=frames, height=6, width=8, num_scales=1, flip=np.array([0, 1, 0], np.uint8), jitter=random_jitter(name, 3, 2))
    if name == "same_12x20":
        return dict(frames=image(name, (2, 12, 20, 3), 1), height=12, width=20, num_scales=1, flip=np.array([0, 0], np.uint8), jitter=None)
    if name == "orders_random":
        return _orders(False)
    if name == "orders_edges":
        return _orders(True)
    raise KeyError(name)


CASES = ["ratio_47x161", "clip_5x7", "upscale_10x14", "saturate_48x64", "same_12x20", "orders_random", "orders_edges"]
CUBE_SHIFTS = (0, 37, 231)
TABLE_PAIRS = [(375, 192), (1242, 640), (375, 320), (1242, 1024)]


def table_pairs():
    """every (in, out) pair a case resizes along, plus the KITTI training sizes"""
    pairs = set(TABLE_PAIRS)
    for name in CASES:
        c = build(name)
        h0, w0 = c["frames"].shape[1:3]
        for s in range(c["num_scales"]):
            h, w = c["height"] // 2 ** s, c["width"] // 2 ** s
            pairs.update([(h0, h), (w0, w)])
            h0, w0 = h, w
    return sorted(pairs)
