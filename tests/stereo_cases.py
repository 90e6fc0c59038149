"""Inputs of the stereo tests: the matcher's cases (shape, settings, a synthetic pair built for them) and the hand-made maps of
the speckle filter with the answer written next to them.  Shared by tests/test_stereo_oracle.py and tests/test_gpu_stereo.py."""
import numpy as np

import stereo_ref as R

# name -> (H, W, C, D, minDisparity, blockSize, directions, setting overrides, input kind)
SGBM_CASES = {
    "base_20x72_d16_b3_5": (20, 72, 3, 16, 0, 3, 5, {}, "pair"),
    "base_20x72_d16_b1_8": (20, 72, 3, 16, 0, 1, 8, {}, "pair"),
    "eight_columns_7x40_c1_d32": (7, 40, 1, 32, 0, 3, 5, {}, "pair"),
    "one_wave_33x130_d64_b2": (33, 130, 3, 64, 0, 2, 5, {}, "pair"),
    "ragged_9x200_d160": (9, 200, 3, 160, 0, 3, 5, {}, "pair"),
    "d96_9x120_8": (9, 120, 3, 96, 0, 3, 8, {}, "pair"),
    "min_disparity_3_12x50": (12, 50, 3, 16, 3, 3, 8, {}, "pair"),
    "one_row_1x30": (1, 30, 3, 16, 0, 3, 5, {}, "pair"),
    "one_column_6x17": (6, 17, 3, 16, 0, 3, 5, {}, "pair"),
    "uniqueness_0": (20, 72, 3, 16, 0, 3, 5, {"uniquenessRatio": 0}, "pair"),
    "speckles_off": (20, 72, 3, 16, 0, 3, 5, {"speckleWindowSize": 0}, "pair"),
    "speckles_bite": (20, 72, 3, 16, 0, 3, 5, {"speckleWindowSize": 5}, "noise"),
    "p1_equals_p2": (20, 72, 3, 16, 0, 3, 8, {"P1": 288}, "pair"),
    "constant": (9, 40, 3, 16, 0, 3, 8, {}, "constant"),
    "right_view_noise": (14, 60, 3, 32, 0, 3, 5, {"speckleWindowSize": 10, "speckleRange": 1}, "noise"),
}
TABLE = list(SGBM_CASES)[:9]     # the shapes the feature was specified with


def settings(name):
    H, W, C, D, minD, block, dirs, over, _ = SGBM_CASES[name]
    return R.reference_like(D, block, minDisparity=minD, directions=dirs, **over)


def pair(H, W, C, D, minD, seed, kind="pair"):
    """-> left, right uint8 [H,W,C]: two shifts inside [minD, minD + D), the right view with +-6 of noise so that no cost is an
    exact zero; "noise": a right view that has nothing to do with the left; "constant": both 77"""
    if kind == "constant":
        img = np.full((H, W, C), 77, dtype=np.uint8)
        return img, img.copy()
    maxD = minD + D
    left, right, _ = R.synthetic_pair(H, W, C, maxD, (minD + D // 3, minD + (2 * D) // 3), seed)
    rng = np.random.default_rng(1000 + seed)
    if kind == "noise":
        return left, rng.integers(0, 256, left.shape).astype(np.uint8)
    right = np.clip(right.astype(np.int64) + rng.integers(-6, 7, right.shape), 0, 255).astype(np.uint8)
    return left, right


def sgbm_inputs(name, seed=0):
    H, W, C, D, minD, _, _, _, kind = SGBM_CASES[name]
    return pair(H, W, C, D, minD, seed, kind)


# ---------------------------------------------------------------- speckle maps
INVALID = -16
SPECKLE_CASES = ["snake_kept_at_299", "snake_removed_at_300", "exact_sizes", "chain_rule", "diagonal_touch", "all_invalid"]


def _snake(H=40, W=70, n=300):
    """a one-pixel-wide path: even rows in full, alternately left to right and right to left, joined by one pixel of the odd
    row between them at the end where the path turns; cut after n pixels"""
    path, y, forward = [], 0, True
    while len(path) < n and y < H:
        xs = range(W) if forward else range(W - 1, -1, -1)
        path += [(y, x) for x in xs]
        if y + 1 < H:
            path.append((y + 1, W - 1 if forward else 0))
        y, forward = y + 2, not forward
    return path[:n]


def speckle_case(name):
    """-> dict(disp int16 [H,W], invalid, max_size, max_diff, kept bool [H,W]: the pixels that must survive)"""
    H, W = 40, 70
    disp = np.full((H, W), INVALID, dtype=np.int16)
    kept = np.zeros((H, W), dtype=bool)
    max_size, max_diff = 6, 16
    if name.startswith("snake"):
        path = _snake(H, W, 300)
        assert len(path) == 300 and len(set(path)) == 300
        for i, (y, x) in enumerate(path):
            disp[y, x] = 100 + 5 * (i % 4)                   # steps of 5 and 15: inside max_diff everywhere
        max_size = 299 if name == "snake_kept_at_299" else 300
        if max_size == 299:
            kept = disp != INVALID
    elif name == "exact_sizes":
        disp[3:5, 4:7] = 200                                # 2 x 3 = max_size pixels: removed
        disp[10:12, 20:23] = 200
        disp[12, 20] = 210                                  # 7 pixels: kept
        kept[10:12, 20:23] = True
        kept[12, 20] = True
        disp[30, 60] = 50                                   # a single pixel: removed
    elif name == "chain_rule":
        disp[5, 10:20] = np.arange(10, dtype=np.int16) * 16   # ends 144 apart, every step 16: one component of 10
        kept[5, 10:20] = True
        disp[9, 10:20] = np.arange(10, dtype=np.int16) * 17   # every step 17: ten components of one
        disp[20:24, 30] = [0, 16, 33, 49]                     # a vertical chain broken in the middle: 2 + 2
        max_size = 9
    elif name == "diagonal_touch":
        disp[4:6, 4:6] = 300
        disp[6:8, 6:8] = 300                                # touches the first blob at a corner only: 4 + 4, not 8
        disp[20:22, 20:22] = 300
        disp[22, 21] = 300                                  # five pixels joined by an edge: kept
        kept[20:22, 20:22] = True
        kept[22, 21] = True
        max_size = 4
    elif name == "all_invalid":
        pass
    else:
        raise KeyError(name)
    return {"disp": disp, "invalid": INVALID, "max_size": max_size, "max_diff": max_diff, "kept": kept}
