"""numpy restatement of the NYUv2 training inputs (NYUv2/data.py:22-68, :107-140 over Pillow's 8-bit paths, train.py:281): the
oracle of wavelet_monodepth_amd.nyu_inputs.  Integer and float32 arithmetic only, written so that it equals Pillow bit for
bit -- tests/golden/make_golden_nyu_inputs.py asserts that where Pillow is installed.

    ksize, table, accumulators, _pass, resize(img, h, w)   pillow_resample_ref's, the bicubic filter by default
    gamma_lut(gamma)                    TF.adjust_gamma's table as Image.point applies it
    augment(image, depth, flip, perm, lut), crop_resize(img, crop, h, w)
    item(image, depth, ...)             the whole chain of one sample -> (image u8 [ih,iw,3], depth u8 [dh,dw])
    image_tensor(u8), depth_tensor(u8), disp_of(depth)   the float32 conversions
"""
import itertools

import numpy as np

from pillow_resample_ref import BICUBIC, LANCZOS, _pass, accumulators, ksize, resize, table   # noqa: F401

F32 = np.float32
PERMS = list(itertools.permutations(range(3)))


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
