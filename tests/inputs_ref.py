"""numpy restatement of the KITTI training inputs (KITTI/datasets/mono_dataset.py:118-145 over Pillow's 8-bit paths): the
oracle of wavelet_monodepth_amd.kitti_inputs.  Integer and float32 arithmetic only, written so that it equals Pillow bit
for bit -- tests/golden/make_golden_inputs.py asserts that where Pillow is installed.

    lanczos_table(n_in, n_out), resize(img, h, w)   pillow_resample_ref's table and resize with the Lanczos filter
    pyramid(img, height, width, n, flip) -> list of uint8 levels, each resized from the previous one
    brightness / contrast / saturation / hue, jitter(img, order, factors, hue_shift)   uint8 -> uint8
    rgb_to_hsv, hsv_to_rgb              Convert.c rgb2hsv_row / hsv2rgb
    to_tensor(img)                      float32 CHW, u8 / 255 as a float32 division
"""
import numpy as np

import pillow_resample_ref as P
from pillow_resample_ref import _pass   # noqa: F401

F32 = np.float32


def lanczos_ksize(n_in, n_out):
    return P.ksize(n_in, n_out, P.LANCZOS)


def lanczos_table(n_in, n_out):
    return P.table(n_in, n_out, P.LANCZOS)


def resize(img, h, w):
    return P.resize(img, h, w, P.LANCZOS)


def pyramid(img, height, width, num_scales=4, flip=False):
    if flip:
        img = img[:, ::-1]
    levels = []
    for s in range(num_scales):
        img = resize(img, height // 2 ** s, width // 2 ** s)
        levels.append(img)
    return levels


def to_tensor(img):
    return np.ascontiguousarray((img.astype(F32) / F32(255.0)).transpose(2, 0, 1))


# ---------------------------------------------------------------- colour jitter
def grey(img):
    x = img.astype(np.int64)
    return ((19595 * x[..., 0] + 38470 * x[..., 1] + 7471 * x[..., 2] + 0x8000) >> 16).astype(np.uint8)


def blend(deg, img, f):
    """ImagingBlend(deg, img, f): float32, the product and the sum each rounded on their own"""
    f = F32(f)
    d = deg.astype(F32)
    o = d + (f * (img.astype(F32) - d)).astype(F32)
    if not (F32(0.0) <= f <= F32(1.0)):
        o = np.clip(o, F32(0.0), F32(255.0))
    return o.astype(np.int32).astype(np.uint8)   # truncation


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def grey_mean(img):
    g = grey(img).astype(np.int64)
    n = g.size
    return int((2 * int(g.sum()) + n) // (2 * n))


def contrast(img, f):
    return blend(np.full_like(img, grey_mean(img)), img, f)


def saturation(img, f):
    return blend(np.repeat(grey(img)[..., None], 3, axis=-1), img, f)


def rgb_to_hsv(img):
    r, g, b = (img[..., c].astype(np.int32) for c in range(3))
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    flat = mx == mn
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (mx - mn).astype(F32)
        s = cr / mx.astype(F32)
        rc, gc, bc = ((mx - c).astype(F32) / cr for c in (r, g, b))
        rc, gc, bc = rc.astype(np.float64), gc.astype(np.float64), bc.astype(np.float64)
        h = np.where(r == mx, bc - gc, np.where(g == mx, 2.0 + rc - bc, 4.0 + gc - rc)).astype(F32)
        h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(F32)
        H = np.clip((h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
        S = np.clip((s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    H, S = np.where(flat, 0, H), np.where(flat, 0, S)
    return np.stack([H, S, mx], axis=-1).astype(np.uint8)


def hsv_to_rgb(img):
    h, s, v = (img[..., c].astype(F32) for c in range(3))
    one, half = F32(1.0), F32(0.5)
    hf = h * F32(6.0) / F32(255.0)
    i = np.floor(hf)
    f = hf - i
    fs = s / F32(255.0)

    def rnd(x):
        return np.clip(np.floor(x + half).astype(np.int32), 0, 255)

    p = rnd(v * (one - fs))
    q = rnd(v * (one - fs * f))
    t = rnd(v * (one - fs * (one - f)))
    vi = img[..., 2].astype(np.int32)
    k = i.astype(np.int32) % 6
    r = np.choose(k, [vi, q, p, p, t, vi])
    g = np.choose(k, [t, vi, vi, q, p, p])
    b = np.choose(k, [p, p, t, vi, vi, q])
    out = np.stack([r, g, b], axis=-1)
    return np.where((img[..., 1] == 0)[..., None], vi[..., None], out).astype(np.uint8)


def hue(img, shift):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(shift)) & 255
    return hsv_to_rgb(hsv)


OPS = (brightness, contrast, saturation, hue)   # the codes of ColorJitterParams.order


def jitter(img, order, factors, hue_shift):
    """one uint8 image [h,w,3] through the four ops in `order`; the contrast mean is taken where the chain stands"""
    for op in order:
        img = hue(img, hue_shift) if op == 3 else OPS[op](img, factors[op])
    return img


def jitter_batch(imgs, enable, order, factors, hue_shift):
    return np.stack([jitter(imgs[i], order[i], factors[i], hue_shift[i]) if enable[i] else imgs[i] for i in range(len(imgs))])


def hue_shift_of(hue_factor):
    """torchvision 0.8.2: np_h += np.uint8(hue_factor * 255), the cast truncating toward zero and wrapping"""
    return int(hue_factor * 255) % 256


def colour_cube():
    """all 2^24 colours as one uint8 [4096,4096,3] image: pixel (y, x) holds colour index y 4096 + x = r 65536 + g 256 + b"""
    idx = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(idx >> 16) & 255, (idx >> 8) & 255, idx & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)
