"""numpy restatement of Pillow's 8-bit resample (Resample.c precompute_coeffs + normalize_coeffs_8bpc and the 8bpc passes): the
part that inputs_ref.py (Lanczos) and nyu_inputs_ref.py (bicubic) share.  Anchored to Pillow through their committed goldens.

    ksize(n_in, n_out, filter), table(n_in, n_out, filter) -> (bounds [out,2], k [out,ksize])
    accumulators(img, bounds, coeffs), _pass(img, bounds, coeffs)   one pass along axis 1
    resize(img, h, w, filter)           horizontal pass, uint8 intermediate, vertical pass; img uint8 [H,W,C]
"""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
BICUBIC, LANCZOS = "bicubic", "lanczos"
SUPPORT = {BICUBIC: 2.0, LANCZOS: 3.0}


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _lanczos(t):
    if -3.0 <= t < 3.0:
        if t == 0.0:
            return 1.0
        a, b = t * math.pi, t / 3.0 * math.pi
        return math.sin(a) / a * (math.sin(b) / b)
    return 0.0


FILTERS = {BICUBIC: _bicubic, LANCZOS: _lanczos}


def ksize(n_in, n_out, filter=BICUBIC):
    return int(math.ceil(SUPPORT[filter] * max(n_in / n_out, 1.0))) * 2 + 1


def table(n_in, n_out, filter=BICUBIC):
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[filter] * fs
    f = FILTERS[filter]
    bounds = np.zeros((n_out, 2), np.int32)
    coeffs = np.zeros((n_out, ksize(n_in, n_out, filter)), np.int32)
    ss = 1.0 / fs
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(n)]
        tot = 0.0
        for v in w:
            tot += v
        for x in range(n):
            v = w[x] / tot if tot != 0.0 else w[x]
            coeffs[xx, x] = int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5)
        bounds[xx] = (xmin, n)
    return bounds, coeffs


def accumulators(img, bounds, coeffs):
    """one pass along axis 1 of img [R,n_in,C] uint8 -> int64 [R,n_out,C], shifted down but not yet clipped"""
    n_out = bounds.shape[0]
    out = np.empty((img.shape[0], n_out, img.shape[2]), np.int64)
    src = img.astype(np.int64)
    for xx in range(n_out):
        xmin, n = bounds[xx]
        acc = np.tensordot(src[:, xmin:xmin + n, :], coeffs[xx, :n].astype(np.int64), axes=([1], [0])) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max() < 2 ** 31
        out[:, xx, :] = acc >> PRECISION_BITS
    return out


def _pass(img, bounds, coeffs):
    return np.clip(accumulators(img, bounds, coeffs), 0, 255).astype(np.uint8)


def resize(img, h, w, filter=BICUBIC):
    """img uint8 [H,W,C] -> [h,w,C]; a pass whose size does not change is skipped, as Pillow skips it"""
    H, W = img.shape[:2]
    if W != w:
        img = _pass(img, *table(W, w, filter))
    if H != h:
        img = _pass(img.transpose(1, 0, 2), *table(H, h, filter)).transpose(1, 0, 2)
    return np.ascontiguousarray(img)
