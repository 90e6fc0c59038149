"""NYUv2 training inputs on the GPU (csrc/wmd_nyu_inputs.hip): NYUv2/data.py, getDefaultTrainTransform / getNoTransform.

    train_transform(image_u8, depth_u8, aug, is_224, crop, image_size, depth_size, disparity)   :22-68, :107-140   one launch
    PERMS, gamma_lut(gamma)                                          RandomChannelSwap's list, RandomGamma's table over Pillow
    Augmentation(flip, perm, lut), sample_augmentation(B, ...)       :33, :49-51, :66   drawn on the host
    bicubic_table(n_in, n_out), resample_table(filter, n_in, n_out)  Pillow's 8-bit tables, built by the library on the host

The caller unzips and decodes the samples and hands over uint8 images [B,H0,W0,3] and 8-bit depth maps [B,H0,W0]; flip,
channel swap, gamma, the crop, the two bicubic resizes, ToTensor, * 1000, the clamp and (`disparity`) train.py:281's DepthNorm
run on the device in one launch and give, bit for bit, what the reference's chain gives over Pillow 12.2.  No autograd, no CPU
fallback: CPU tensors raise.
"""
import itertools

import numpy as np
import torch

from . import _lib, resample
from ._lib import check, current_stream, ptr
from .resample import FILTER_BICUBIC, FILTER_LANCZOS, resample_table   # noqa: F401

PERMS = list(itertools.permutations(range(3)))   # RandomChannelSwap.indices: index 0 is the identity


def gamma_lut(gamma):
    """uint8 [256]: TF.adjust_gamma(img, gamma, gain=1) on a PIL image is img.point(table) with
    table[e] = (255 + 1 - 1e-3) * pow(e / 255., gamma) as floats; Pillow 12.2's Image.point rounds each entry with Python's
    round (half to even) and its C side clips to 0..255.  gamma_lut(1.0) is not the identity: 254 -> 255."""
    gamma = float(gamma)
    if not gamma > 0.0 or gamma == float("inf"):
        raise _lib.WmdError("gamma_lut: gamma must be positive and finite (got %r)" % (gamma,))
    return np.array([min(max(round((255 + 1 - 1e-3) * pow(e / 255., gamma)), 0), 255) for e in range(256)], np.uint8)


class Augmentation:
    """Per item: flip uint8 [B]; perm uint8 [B], an index into PERMS (image[..., PERMS[perm]]); lut uint8 [B,256] or None,
    applied to every channel of the image (an item without gamma holds np.arange(256)).  Built from host data (arrays, lists or
    CPU tensors) the values are checked; `.to(device)` moves all three.  On the device the kernel reads perm clamped to 5."""

    def __init__(self, flip, perm, lut=None):
        def tensor(v):
            if isinstance(v, torch.Tensor):
                return (v.to(torch.uint8) if v.dtype == torch.bool else v).contiguous()
            return torch.as_tensor(np.asarray(v), dtype=torch.uint8).contiguous()
        self.flip, self.perm, self.lut = tensor(flip), tensor(perm), None if lut is None else tensor(lut)
        n = self.flip.numel()
        want = {"flip": (self.flip, (n,)), "perm": (self.perm, (n,))}
        if self.lut is not None:
            want["lut"] = (self.lut, (n, 256))
        for name, (t, shape) in want.items():
            if tuple(t.shape) != shape or t.dtype != torch.uint8:
                raise _lib.WmdError("Augmentation.%s must be uint8 %s (got %s %s)" % (name, list(shape), t.dtype, list(t.shape)))
        if len({t.device for t, _ in want.values()}) != 1:
            raise _lib.WmdError("Augmentation: the tensors must live on one device")
        if not self.flip.is_cuda and n and int(self.perm.max()) > 5:   # host data: check the values
            raise _lib.WmdError("Augmentation.perm must be in 0..5 (an index into PERMS)")

    def __len__(self):
        return self.flip.numel()

    def to(self, device):
        return Augmentation(self.flip.to(device), self.perm.to(device), None if self.lut is None else self.lut.to(device))


def sample_augmentation(B, generator=None, swap_p=0.1, gamma=0.8):
    """The reference's draw for B samples, on the host: flip with probability 0.5; with probability swap_p a uniform index
    0..5 into PERMS (0 otherwise); a gamma uniform between 1 / gamma and gamma -> gamma_lut.  gamma == 0 gives no table, as
    RandomGamma(0) does nothing.  Python's `random` stream is not reproduced; pass a torch.Generator to fix the draw."""
    u = torch.rand((B, 4), generator=generator, dtype=torch.float64)
    flip = (u[:, 0] < 0.5).to(torch.uint8)
    index = torch.clamp((u[:, 2] * 6).to(torch.int64), max=5)
    perm = torch.where(u[:, 1] < swap_p, index, torch.zeros_like(index)).to(torch.uint8)
    lut = None
    if gamma != 0:
        lo, hi = 1.0 / gamma, float(gamma)
        lut = np.stack([gamma_lut(lo + (hi - lo) * float(v)) for v in u[:, 3]]) if B else np.zeros((0, 256), np.uint8)
    return Augmentation(flip, perm, lut)


def bicubic_table(n_in, n_out):
    return resample_table(FILTER_BICUBIC, n_in, n_out)


def train_transform(image_u8, depth_u8, aug=None, is_224=False, crop=16, image_size=None, depth_size=None, disparity=False, keep_u8=False):
    """image_u8 uint8 [B,H0,W0,3], depth_u8 uint8 [B,H0,W0] on the device -> {"image": float32 [B,3,ih,iw], "depth": float32
    [B,1,dh,dw]}, plus "disp_gt" = 10 / depth with `disparity` and the uint8 resized planes "image_u8" [B,ih,iw,3] and
    "depth_u8" [B,dh,dw] with `keep_u8`.  Sizes are (h, w); the defaults are the reference's, (480, 640) and (240, 320), or
    (224, 224) for both with is_224.  aug: an Augmentation of B items on the same device; None is getNoTransform: no flip, no
    swap and no table."""
    who = "train_transform"
    _lib.require_device(who, image_u8=(image_u8, torch.uint8), depth_u8=(depth_u8, torch.uint8, "16-bit depth maps are not implemented"))
    if image_u8.dim() != 4 or image_u8.shape[3] != 3:
        raise _lib.WmdError("image_u8 must be [B,H0,W0,3] (got %s)" % (tuple(image_u8.shape),))
    B, H0, W0 = (int(v) for v in image_u8.shape[:3])
    if tuple(depth_u8.shape) != (B, H0, W0) or depth_u8.device != image_u8.device:
        raise _lib.WmdError("depth_u8 must be [%d,%d,%d] on %s (got %s on %s)" % (B, H0, W0, image_u8.device, tuple(depth_u8.shape), depth_u8.device))
    dev = image_u8.device
    ih, iw = (int(v) for v in (image_size if image_size is not None else ((224, 224) if is_224 else (480, 640))))
    dh, dw = (int(v) for v in (depth_size if depth_size is not None else ((224, 224) if is_224 else (240, 320))))
    crop = int(crop)
    flip = perm = lut = None
    if aug is not None:
        if not isinstance(aug, Augmentation):
            raise _lib.WmdError("train_transform needs an Augmentation (got %s)" % type(aug).__name__)
        if len(aug) != B or aug.flip.device != dev:
            raise _lib.WmdError("%s: aug holds %d items on %s, the images are %d on %s" % (who, len(aug), aug.flip.device, B, dev))
        flip, perm, lut = aug.flip, aug.perm, aug.lut
    l = _lib.lib()
    n_tab = l.wmd_nyu_inputs_table_ints(H0, W0, crop, ih, iw, dh, dw)
    ok = n_tab > 0 and B > 0
    tables = resample.device_tables("nyu_inputs", (H0, W0, crop, ih, iw, dh, dw), dev) if ok else torch.zeros(1, dtype=torch.int32, device=dev)
    shape_i, shape_d = ((B, 3, ih, iw), (B, 1, dh, dw)) if ok else ((1,), (1,))
    image_u8, depth_u8 = image_u8.contiguous(), depth_u8.contiguous()
    out = {"image": torch.empty(shape_i, device=dev, dtype=torch.float32), "depth": torch.empty(shape_d, device=dev, dtype=torch.float32)}
    if disparity:
        out["disp_gt"] = torch.empty_like(out["depth"])
    if keep_u8:
        out["image_u8"] = torch.empty((B, ih, iw, 3) if ok else (1,), device=dev, dtype=torch.uint8)
        out["depth_u8"] = torch.empty((B, dh, dw) if ok else (1,), device=dev, dtype=torch.uint8)
    check(l.wmd_nyu_inputs(ptr(image_u8), ptr(depth_u8), B, H0, W0, crop, ih, iw, dh, dw, ptr(flip), ptr(perm), ptr(lut), ptr(tables), n_tab,
                           ptr(out["image"]), ptr(out["depth"]), ptr(out.get("disp_gt")), ptr(out.get("image_u8")), ptr(out.get("depth_u8")),
                           current_stream()), "wmd_nyu_inputs")
    return out
