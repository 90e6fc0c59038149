"""numpy restatement of the NYUv2 training inputs (NYUv2/data.py:22-68, :107-140 over Pillow's 8-bit paths, train.py:281): the
oracle of wavelet_monodepth_amd.nyu_inputs.  Integer and float32 arithmetic only, written so that it equals Pillow bit for
bit -- tests/golden/make_golden_nyu_inputs.py asserts that where Pillow is installed.

    table(n_in, n_out, filter)          Resample.c precompute_coeffs + normalize_coeffs_8bpc -> (bounds [out,2], k [out,ksize])
    resize(img, h, w)                   horizontal pass, uint8 intermediate, vertical pass; img uint8 [H,W,C]; bicubic
    gamma_lut(gamma)                    TF.adjust_gamma's table as Image.point applies it
    augment(image, depth, flip, perm, lut), crop_resize(img, crop, h, w)
    item(image, depth, ...)             the whole chain of one sample -> (image u8 [ih,iw,3], depth u8 [dh,dw])
    image_tensor(u8), depth_tensor(u8), disp_of(depth)   the float32 conversions
"""
import itertools
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
F32 = np.float32
PERMS = list(itertools.permutations(range(3)))
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


def gamma_lut(gamma):
    """Image.point([(255 + 1 - 1e-3) * pow(e / 255., gamma) ...]): Python's round on each float, then the C side's clip"""
    return np.array([min(max(round((255 + 1 - 1e-3) * pow(e / 255., gamma)), 0), 255) for e in range(256)], np.uint8)


def augment(image, depth, flip, perm, lut):
    """flip, channel swap, table: data.py's order; lut None = RandomGamma(0)"""
    if flip:
        image, depth = image[:, ::-1], depth[:, ::-1]
    image = image[..., list(PERMS[int(perm)])]
    if lut is not None:
        image = np.asarray(lut, np.uint8)[image]
    return image, depth


def crop_resize(img, crop, h, w):
    H, W = img.shape[:2]
    box = img[crop:H - crop, crop:W - crop]
    return resize(box if box.ndim == 3 else box[..., None], h, w).reshape((h, w) + img.shape[2:])


def item(image, depth, crop, image_size, depth_size, flip=0, perm=0, lut=None):
    image, depth = augment(image, depth, flip, perm, lut)
    return crop_resize(image, crop, *image_size), crop_resize(depth, crop, *depth_size)


def image_tensor(u8):
    """[h,w,3] uint8 -> float32 [3,h,w], u8 / 255 as a float32 division"""
    return np.ascontiguousarray((u8.astype(F32) / F32(255.0)).transpose(2, 0, 1))


def depth_tensor(u8):
    """[h,w] uint8 -> float32 [1,h,w]: clamp((u8 / 255) * 1000, 10, 1000), every operation in float32"""
    return np.clip((u8.astype(F32) / F32(255.0)) * F32(1000.0), F32(10.0), F32(1000.0))[None]


def disp_of(depth):
    return F32(10.0) / depth
