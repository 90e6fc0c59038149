"""Inputs of the colour-image tests, regenerated from wavelet_monodepth_amd.synth (numpy only): the fixture
tests/golden/viz_reference.npz stores the expected outputs of every case below, the tests rebuild the inputs.

disparity cases: dict(x [B,h,w] float32, size (H, W) or None, q).  With q = 95 the order statistic below the percentile and
the weight g = frac((n - 1) * 0.95f) are: n = 2: k = 0, g = 0.95; n = 3: k = 1, g = 0.9 (0.2 at q = 60); 7 x 13 = 91: 85.5
exactly after the float32 rounding of 85.4999989 -- the first g of the right-hand branch; 37 x 53 = 1961: 1862, g = 0.
"""
import numpy as np

from wavelet_monodepth_amd import synth

F32 = np.float32
FULL = (375, 1242)                    # a KITTI frame: (n - 1) * 0.95f is above 2^18, g a multiple of 1/32


def dist(kind, shape, tag, seed=0):
    u = synth.uniform(shape, "viz_" + tag, seed, 0.0, 1.0)
    if kind == "uniform":
        return (F32(0.01) + F32(0.99) * u).astype(F32)
    if kind == "constant":
        return np.full(shape, 0.37, F32)
    if kind == "quant":               # eight distinct values: s[k] == s[k+1], duplicates on both sides of k
        return (np.floor(u * F32(8)) / F32(8)).astype(F32)
    if kind == "narrow":
        return (F32(0.30) + F32(0.01) * u).astype(F32)
    if kind == "heavy":               # a few pixels far above the percentile
        return (F32(1) / (F32(0.01) + F32(9.99) * u)).astype(F32)
    if kind == "signed":
        return (F32(2) * u - F32(1)).astype(F32)
    raise KeyError(kind)


# name -> (kind(s), (B, h, w), size, q)
DISPARITY = {
    "one": ("uniform", (1, 1, 1), None, 95),
    "two": ("uniform", (1, 1, 2), None, 95),
    "three": ("uniform", (1, 1, 3), None, 95),
    "three_q60": ("uniform", (1, 1, 3), None, 60),
    "q0": ("uniform", (1, 5, 9), None, 0),
    "q100": ("uniform", (1, 5, 9), None, 100),
    "q99_5": ("heavy", (1, 11, 17), None, 99.5),
    "constant": ("constant", (1, 6, 10), None, 95),
    "quant": ("quant", (1, 16, 24), None, 95),
    "narrow": ("narrow", (1, 16, 24), None, 95),
    "heavy": ("heavy", (1, 24, 40), None, 95),
    "signed": ("signed", (1, 16, 24), None, 95),
    "ragged_7x13": ("uniform", (1, 7, 13), None, 95),
    "ragged_37x53": ("heavy", (1, 37, 53), None, 95),
    "batch3": (("heavy", "constant", "signed"), (3, 9, 31), None, 95),
    "resize_6x20_11x37": ("uniform", (1, 6, 20), (11, 37), 95),
    "resize_6x20_same": ("uniform", (1, 6, 20), (6, 20), 95),
    "resize_12x40_47x155": ("heavy", (2, 12, 40), (47, 155), 95),
}
RESIZED = tuple(n for n, c in DISPARITY.items() if c[2] is not None and c[2] != c[1][1:])


def disparity(name):
    if name == "full":
        return dict(x=synth.uniform((1,) + FULL, "viz_full", 0, 0.0, 1.0), size=None, q=95)
    kinds, (B, h, w), size, q = DISPARITY[name]
    if isinstance(kinds, str):
        kinds = (kinds,) * B
    x = np.stack([dist(k, (h, w), name, b) for b, k in enumerate(kinds)])
    return dict(x=x, size=size, q=q)


# colorize: name -> dict(x [B,H,W], vmin, vmax)
def colorize(name):
    if name == "fixed":               # metres: below 0.1, above 10, and a NaN
        u = synth.uniform((2, 9, 14), "viz_colorize_fixed", 0, 0.0, 1.0)
        x = (F32(0.02) * np.exp2(F32(10) * u)).astype(F32)          # 0.02 .. 20.5
        x[0, 3, 4] = np.nan
        x[1, 0, 0], x[1, 0, 1], x[1, 0, 2] = 0.1, 10.0, 10.000001
        return dict(x=x, vmin=0.1, vmax=10)
    if name == "auto":
        return dict(x=np.stack([dist("heavy", (9, 14), name, 0), dist("signed", (9, 14), name, 1)]), vmin=None, vmax=None)
    if name == "auto_constant":
        return dict(x=np.stack([dist("constant", (5, 7), name, 0), dist("uniform", (5, 7), name, 1)]), vmin=None, vmax=None)
    raise KeyError(name)


COLORIZE = ("fixed", "auto", "auto_constant")


# normalize_image: name -> dict(x, per_image)
def normalize(name):
    if name == "plain":
        return dict(x=dist("signed", (2, 3, 5, 7), "norm_plain"), per_image=False)
    if name == "constant":
        return dict(x=np.full((2, 4, 6), -1.25, F32), per_image=False)
    if name == "per_image":
        x = np.stack([dist("heavy", (3, 5, 7), "norm_pi", 0), dist("constant", (3, 5, 7), "norm_pi", 1),
                      dist("narrow", (3, 5, 7), "norm_pi", 2)])
        return dict(x=x, per_image=True)
    raise KeyError(name)


NORMALIZE = ("plain", "constant", "per_image")
