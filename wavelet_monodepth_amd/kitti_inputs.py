"""KITTI training inputs on the GPU (csrc/wmd_inputs.hip): KITTI/datasets/mono_dataset.py, MonoDataset.preprocess / __getitem__.

    color_pyramid(frames, height, width, num_scales, flip, jitter)   :118-145   uint8 [N,H0,W0,3] -> per scale (u8, color, color_aug)
    color_jitter(images_u8, jitter)                                  torchvision 0.8.2's ColorJitter on PIL images, batched
    preprocess(frames_by_id, height, width, scales, do_flip, jitter) -> {("color", f, s), ("color_aug", f, s)}, one call
    ColorJitterParams, sample_color_jitter(B, p, generator)          :99-102, :213-217   drawn on the host
    scaled_intrinsics(K, height, width, scales)                      :202-211   host
    stereo_T(side, do_flip)                                          :228-234   host

The caller decodes the images and hands over uint8 HWC frames; flip, the four-level Lanczos pyramid, ToTensor and the colour
jitter run on the device and give, bit for bit, what the reference's chain gives over Pillow 12.2 (8-bit `resize(...,
LANCZOS)`, `ImageEnhance`, the HSV hue shift).  The depth_gt and depth-hint resizes stay with the caller.  No autograd,
no CPU fallback: CPU tensors raise.
"""
import numpy as np
import torch

from . import _lib, resample
from ._lib import check, current_stream, ptr


class ColorJitterParams:
    """Per item: enable uint8 [N]; order uint8 [N,4], a permutation of 0 brightness, 1 contrast, 2 saturation, 3 hue;
    factors float32 [N,3] for brightness, contrast, saturation; hue_shift int32 [N] in 0..255 (added to the 8-bit H).
    Built from host data (arrays, lists or CPU tensors) the values are checked; `.to(device)` moves all four."""

    def __init__(self, enable, order, factors, hue_shift):
        def tensor(v, dtype):
            if isinstance(v, torch.Tensor):
                return v.to(dtype) if v.dtype == torch.bool else v
            return torch.as_tensor(np.asarray(v), dtype=dtype)
        self.enable, self.order = tensor(enable, torch.uint8).contiguous(), tensor(order, torch.uint8).contiguous()
        self.factors, self.hue_shift = tensor(factors, torch.float32).contiguous(), tensor(hue_shift, torch.int32).contiguous()
        n = self.enable.numel()
        want = {"enable": (self.enable, (n,), torch.uint8), "order": (self.order, (n, 4), torch.uint8),
                "factors": (self.factors, (n, 3), torch.float32), "hue_shift": (self.hue_shift, (n,), torch.int32)}
        for name, (t, shape, dtype) in want.items():
            if tuple(t.shape) != shape or t.dtype != dtype:
                raise _lib.WmdError("ColorJitterParams.%s must be %s %s (got %s %s)" % (name, dtype, list(shape), t.dtype, list(t.shape)))
        if len({t.device for t, _, _ in want.values()}) != 1:
            raise _lib.WmdError("ColorJitterParams: the four tensors must live on one device")
        if not self.enable.is_cuda:   # host data: check the values (on the device the kernels read order & 3, hue_shift & 255)
            if n and not bool((self.order.sort(dim=1).values == torch.arange(4, dtype=torch.uint8)).all()):
                raise _lib.WmdError("ColorJitterParams.order: every row must be a permutation of 0..3")
            if n and (int(self.hue_shift.min()) < 0 or int(self.hue_shift.max()) > 255):
                raise _lib.WmdError("ColorJitterParams.hue_shift must be in 0..255")
            if not bool(torch.isfinite(self.factors).all()):
                raise _lib.WmdError("ColorJitterParams.factors must be finite")

    def __len__(self):
        return self.enable.numel()

    def to(self, device):
        return ColorJitterParams(*(t.to(device) for t in (self.enable, self.order, self.factors, self.hue_shift)))

    def repeat_interleave(self, k):
        """every item k times in a row: the frames of one sample share its jitter"""
        return ColorJitterParams(*(t.repeat_interleave(k, dim=0) for t in (self.enable, self.order, self.factors, self.hue_shift)))

    def _checked(self, who, n, device):
        _lib.require_device(who, enable=(self.enable, torch.uint8))
        if len(self) != n or self.enable.device != device:
            raise _lib.WmdError("%s: jitter holds %d items on %s, the images are %d on %s" % (who, len(self), self.enable.device, n, device))
        return [ptr(t) for t in (self.enable, self.order, self.factors, self.hue_shift)]


def sample_color_jitter(B, p=0.5, generator=None):
    """The reference's draw for B samples, on the host: enabled with probability p, brightness, contrast and saturation
    factors uniform in (0.8, 1.2), hue uniform in (-0.1, 0.1), a uniformly random order.  hue_shift = int(hue * 255) mod 256,
    truncating toward zero: torchvision 0.8.2's `np_h += np.uint8(hue_factor * 255)`.  Python's `random` stream is not
    reproduced; pass a torch.Generator to fix the draw."""
    u = torch.rand((B, 5), generator=generator, dtype=torch.float64)
    factors = (0.8 + 0.4 * u[:, :3]).to(torch.float32)
    hue = -0.1 + 0.2 * u[:, 3]
    shift = torch.tensor([int(float(h) * 255) % 256 for h in hue], dtype=torch.int32)
    order = torch.stack([torch.randperm(4, generator=generator) for _ in range(B)]).to(torch.uint8) if B else torch.zeros((0, 4), dtype=torch.uint8)
    return ColorJitterParams((u[:, 4] < p).to(torch.uint8), order, factors, shift)


def lanczos_table(n_in, n_out):
    """(bounds int32 [out,2] = (xmin, n), coeffs int32 [out,ksize]) of Pillow's 8-bit Lanczos resize, built by the library on the host"""
    return resample.table("lanczos", n_in, n_out)


def color_pyramid(frames, height, width, num_scales=4, flip=None, jitter=None):
    """frames uint8 [N,H0,W0,3] on the device -> [(u8 [N,h,w,3], color float32 [N,3,h,w], color_aug float32 [N,3,h,w])] per
    scale s, h = height // 2**s, w = width // 2**s.  flip: optional uint8 / bool [N]; jitter: optional ColorJitterParams of
    N items.  Without jitter color_aug is color itself."""
    who = "color_pyramid"
    _lib.require_device(who, frames=(frames, torch.uint8))
    if frames.dim() != 4 or frames.shape[3] != 3:
        raise _lib.WmdError("frames must be [N,H0,W0,3] (got %s)" % (tuple(frames.shape),))
    N, H0, W0 = (int(v) for v in frames.shape[:3])
    height, width, num_scales = int(height), int(width), int(num_scales)
    dev = frames.device
    if flip is not None:
        _lib.require_device(who, flip=(flip, (torch.uint8, torch.bool)))
        if tuple(flip.shape) != (N,) or flip.device != dev:
            raise _lib.WmdError("flip must be [%d] on %s (got %s on %s)" % (N, dev, tuple(flip.shape), flip.device))
        flip = flip.to(torch.uint8).contiguous()
    jit = jitter._checked(who, N, dev) if jitter is not None else [None] * 4
    l = _lib.lib()
    n_ws = l.wmd_color_pyramid_workspace_bytes(N, H0, W0, height, width, num_scales)
    sizes = [(height >> s, width >> s) for s in range(max(num_scales, 0))]
    pixels = sum(N * h * w for h, w in sizes) if n_ws else 0
    tables = resample.device_tables("color_pyramid", (H0, W0, height, width, num_scales), dev) if n_ws else torch.zeros(1, dtype=torch.int32, device=dev)
    frames = frames.contiguous()
    ws, _ = _lib.byte_workspace(n_ws, dev)
    levels = torch.empty(max(pixels, 1) * 3, device=dev, dtype=torch.uint8)
    color = torch.empty(max(pixels, 1) * 3, device=dev, dtype=torch.float32)
    aug = torch.empty_like(color) if jitter is not None else None
    check(l.wmd_color_pyramid(ptr(frames), N, H0, W0, height, width, num_scales, ptr(flip), jit[0], jit[1], jit[2], jit[3], ptr(tables),
                              ptr(levels), ptr(color), ptr(aug), ptr(ws), n_ws, current_stream()), "wmd_color_pyramid")
    out, off = [], 0
    for h, w in sizes:
        n = N * h * w * 3
        c = color[off:off + n].view(N, 3, h, w)
        out.append((levels[off:off + n].view(N, h, w, 3), c, aug[off:off + n].view(N, 3, h, w) if aug is not None else c))
        off += n
    return out


def color_jitter(images_u8, jitter):
    """uint8 [N,h,w,3] -> uint8 [N,h,w,3]: torchvision 0.8.2's ColorJitter on PIL images with the given parameters, every
    image on its own (the contrast mean is that image's)."""
    who = "color_jitter"
    _lib.require_device(who, images_u8=(images_u8, torch.uint8))
    if images_u8.dim() != 4 or images_u8.shape[3] != 3:
        raise _lib.WmdError("images_u8 must be [N,h,w,3] (got %s)" % (tuple(images_u8.shape),))
    if not isinstance(jitter, ColorJitterParams):
        raise _lib.WmdError("color_jitter needs ColorJitterParams (got %s)" % type(jitter).__name__)
    N, h, w = (int(v) for v in images_u8.shape[:3])
    jit = jitter._checked(who, N, images_u8.device)
    images_u8 = images_u8.contiguous()
    l = _lib.lib()
    ws, n_ws = _lib.byte_workspace(l.wmd_color_jitter_workspace_bytes(N, h, w), images_u8.device)
    out = torch.empty_like(images_u8)
    check(l.wmd_color_jitter(ptr(images_u8), ptr(out), N, h, w, jit[0], jit[1], jit[2], jit[3], ptr(ws), n_ws, current_stream()), "wmd_color_jitter")
    return out


def preprocess(frames_by_id, height, width, scales=range(4), do_flip=None, jitter=None):
    """{frame_id: uint8 [B,H0,W0,3]} -> {("color", f, s), ("color_aug", f, s): float32 [B,3,h,w]} for s in `scales`.  do_flip
    is uint8 / bool [B], jitter ColorJitterParams of B items: all frames of a sample share its flip and jitter
    (mono_dataset.py:121-124).  All frames go through one color_pyramid call with N = B x frames, sample-major."""
    ids = list(frames_by_id)
    if not ids:
        raise _lib.WmdError("preprocess needs at least one frame")
    scales = [int(s) for s in scales]
    if not scales or min(scales) < 0:
        raise _lib.WmdError("scales must be non-negative (got %s)" % (scales,))
    first = frames_by_id[ids[0]]
    for f in ids:
        t = frames_by_id[f]
        _lib.require_device("preprocess", **{"frames[%r]" % (f,): (t, torch.uint8)})
        if t.shape != first.shape or t.device != first.device or t.dim() != 4:
            raise _lib.WmdError("preprocess: every frame must be uint8 [B,H0,W0,3] of one shape on one device")
    B, F = first.shape[0], len(ids)
    stacked = torch.stack([frames_by_id[f] for f in ids], dim=1).reshape((B * F,) + tuple(first.shape[1:]))
    if do_flip is not None:
        _lib.require_device("preprocess", do_flip=(do_flip, (torch.uint8, torch.bool)))
        do_flip = do_flip.repeat_interleave(F)
    if jitter is not None:
        jitter = jitter.repeat_interleave(F)
    levels = color_pyramid(stacked, height, width, max(scales) + 1, do_flip, jitter)
    out = {}
    for s in scales:
        _, color, aug = levels[s]
        color, aug = color.view((B, F) + tuple(color.shape[1:])), aug.view((B, F) + tuple(aug.shape[1:]))
        for k, f in enumerate(ids):
            out[("color", f, s)] = color[:, k].contiguous()
            out[("color_aug", f, s)] = aug[:, k].contiguous() if jitter is not None else out[("color", f, s)]
    return out


def scaled_intrinsics(K, height, width, scales=range(4)):
    """mono_dataset.py:202-211: the normalised float32 K [4,4] -> {("K", s), ("inv_K", s)} as float32 tensors, rows 0 and 1
    scaled by width // 2**s and height // 2**s, the inverse by numpy's float32 pinv."""
    K = np.asarray(K)
    if K.shape != (4, 4) or K.dtype != np.float32:
        raise _lib.WmdError("K must be float32 [4,4] (got %s %s)" % (K.dtype, K.shape))
    out = {}
    for scale in scales:
        Ks = K.copy()
        Ks[0, :] *= width // (2 ** scale)
        Ks[1, :] *= height // (2 ** scale)
        out[("K", scale)] = torch.from_numpy(Ks)
        out[("inv_K", scale)] = torch.from_numpy(np.linalg.pinv(Ks))
    return out


def stereo_T(side, do_flip):
    """mono_dataset.py:228-234: the float32 [4,4] transform to the other camera of the rig, baseline 0.1, its sign turned by
    the side ("l" / "r") and by the flip."""
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = (-1 if side == "l" else 1) * (-1 if do_flip else 1) * 0.1
    return torch.from_numpy(T)
