"""Semi-global stereo matching on the GPU (csrc/wmd_stereo.hip): the matcher of KITTI/precompute_depth_hints.py:42-63,127-151,
which produces the candidates that depth_hints.fuse_depth_hints selects from.

    SGBMSettings(...)                                   a plain record with OpenCV's StereoSGBM parameter names
    reference_settings()                                the twelve settings of generate_stereo_matchers
    sgbm(left_u8, right_u8, settings, reverse=None)     int16 [B,H,W]: 16 x the pixel disparity
    filter_speckles(disp_i16, invalid, max_size, max_diff)
    depth_hint_candidates(base_u8, lookup_u8, base_is_right)    float32 [B,M,H,W] pixel disparities, ready for fusion
    precompute_depth_hints(base_u8, lookup_u8, base_is_right, K, inv_K)   the whole script: candidates, T, fusion

The contract is the integer specification in DESIGN.md ("Semi-global stereo matching"): it follows StereoSGBM's documented
parameters and stages, tests/stereo_ref.py restates it in numpy and the kernels match that bit for bit.  It is NOT "equal to
cv2": OpenCV is not a dependency and nobody has measured how far its maps are from these.  Fusion takes candidates from any
matcher, so nothing downstream depends on that.  GPU only, no CPU fallback: CPU tensors raise."""
import collections

import torch

from . import _lib, depth_hints
from ._lib import check, current_stream, ptr

_FIELDS = ("minDisparity", "numDisparities", "blockSize", "P1", "P2", "preFilterCap", "uniquenessRatio", "speckleWindowSize",
           "speckleRange", "disp12MaxDiff", "directions")
_DEFAULTS = (0, 16, 3, 0, 0, 0, 0, 0, 0, 0, 5)


class SGBMSettings(collections.namedtuple("SGBMSettings", _FIELDS, defaults=_DEFAULTS)):
    """OpenCV's names and defaults where it has them (mode MODE_SGBM is directions=5, MODE_HH directions=8).
    disp12MaxDiff <= 0 means 1; speckleWindowSize == 0 skips the speckle stage."""
    __slots__ = ()

    @property
    def invalid(self):
        """the int16 value of a pixel without a disparity"""
        return (self.minDisparity - 1) * 16

    @property
    def window(self):
        return 2 * (self.blockSize // 2) + 1


def reference_settings():
    """generate_stereo_matchers (precompute_depth_hints.py:42-63): blockSize 1 / 2 / 3 x numDisparities 64 / 96 / 128 / 160"""
    sad = 3
    return [SGBMSettings(minDisparity=0, numDisparities=nd, blockSize=bs, P1=sad * sad * 4, P2=sad * sad * 32, preFilterCap=63,
                         uniquenessRatio=10, speckleWindowSize=100, speckleRange=16)
            for bs in (1, 2, 3) for nd in (64, 96, 128, 160)]


def _images(who, left, right):
    _lib.require_device(who, left=(left, torch.uint8), right=(right, torch.uint8))
    if left.dim() == 3:
        left, right = left.unsqueeze(-1), right.unsqueeze(-1)
    if left.dim() != 4 or left.shape != right.shape or left.device != right.device:
        raise _lib.WmdError("%s: left and right must be uint8 [B,H,W,C] (or [B,H,W]) of one shape on one device (got %s, %s)"
                            % (who, tuple(left.shape), tuple(right.shape)))
    return left.contiguous(), right.contiguous()


def _reverse(who, reverse, B, dev):
    if reverse is None:
        return None
    if not torch.is_tensor(reverse):
        reverse = torch.tensor([bool(v) for v in reverse], dtype=torch.uint8)
    if tuple(reverse.shape) != (B,):
        raise _lib.WmdError("%s: reverse must have %d entries (got %s)" % (who, B, tuple(reverse.shape)))
    return (reverse != 0).to(device=dev, dtype=torch.uint8).contiguous()


def sgbm(left_u8, right_u8, settings, reverse=None, return_volumes=False):
    """left / right uint8 [B,H,W,C] (C = 1 or 3; [B,H,W] is C = 1) -> int16 [B,H,W], 16 x the disparity of the left image's
    pixels, settings.invalid where there is none.  reverse: optional [B] flags (tensor or sequence); a flagged pair is mirrored
    before matching and its map mirrored back -- the `reverse=True` branch of compute_depths, for a base image that is the
    right view.  return_volumes: also the block costs and the summed path costs, int32 [B,H,Wv,D] over the valid rectangle
    (Wv = W - minDisparity - numDisparities)."""
    who = "sgbm"
    left, right = _images(who, left_u8, right_u8)
    s = settings
    B, H, W, C = (int(v) for v in left.shape)
    dev = left.device
    rev = _reverse(who, reverse, B, dev)
    l = _lib.lib()
    ws, n_ws = _lib.byte_workspace(l.wmd_stereo_sgbm_workspace_bytes(B, H, W, C, s.minDisparity, s.numDisparities, s.blockSize), dev)
    disp = torch.empty((B, H, W), device=dev, dtype=torch.int16)
    cost = vol = None
    if return_volumes:
        shape = (B, H, max(W - s.minDisparity - s.numDisparities, 1), max(s.numDisparities, 1))
        cost, vol = (torch.empty(shape, device=dev, dtype=torch.int16) for _ in range(2))
    check(l.wmd_stereo_sgbm(ptr(left), ptr(right), ptr(rev), ptr(disp), ptr(cost), ptr(vol), B, H, W, C, s.minDisparity, s.numDisparities,
                            s.blockSize, s.P1, s.P2, s.preFilterCap, s.uniquenessRatio, s.speckleWindowSize, s.speckleRange,
                            s.disp12MaxDiff, s.directions, ptr(ws), n_ws, current_stream()), "wmd_stereo_sgbm")
    if return_volumes:
        return disp, cost.to(torch.int32) & 0xFFFF, vol.to(torch.int32) & 0xFFFF   # the volumes are unsigned 16-bit
    return disp


def filter_speckles(disp_i16, invalid, max_size, max_diff):
    """int16 [B,H,W] (or [H,W]) -> a copy in which every 4-connected component of at most max_size pixels is `invalid`;
    neighbours belong together when both differ from `invalid` and from each other by at most max_diff (int16 units)."""
    _lib.require_device("filter_speckles", disp_i16=(disp_i16, torch.int16))
    if disp_i16.dim() not in (2, 3):
        raise _lib.WmdError("filter_speckles: int16 [B,H,W] or [H,W] expected (got %s)" % (tuple(disp_i16.shape),))
    out = disp_i16.contiguous().clone()
    H, W = (int(v) for v in out.shape[-2:])
    B = int(out.shape[0]) if out.dim() == 3 else 1
    l = _lib.lib()
    ws, n_ws = _lib.byte_workspace(l.wmd_stereo_filter_speckles_workspace_bytes(B, H, W), out.device)
    check(l.wmd_stereo_filter_speckles(ptr(out), B, H, W, int(invalid), int(max_size), int(max_diff), ptr(ws), n_ws, current_stream()),
          "wmd_stereo_filter_speckles")
    return out


def _flags(base_is_right, B, dev):
    if isinstance(base_is_right, bool):
        base_is_right = [base_is_right] * B
    return _reverse("depth_hint_candidates", base_is_right, B, dev)


def depth_hint_candidates(base_u8, lookup_u8, base_is_right, settings=None):
    """base / lookup uint8 [B,H,W,C]: a stereo pair per image, the map belongs to `base`.  base_is_right: a bool or [B] flags;
    a right-view base is matched mirrored (compute_depths(..., reverse=True)).  -> float32 [B,M,H,W] pixel disparities (the
    int16 map / 16, exact; below zero where there is none), one plane per setting (default: reference_settings()), ready for
    fuse_depth_hints(..., disparities=True, focal_times_baseline=...).  Settings that differ only in a blockSize of the same
    window (2 and 3) give the same map: it is computed once and copied."""
    settings = reference_settings() if settings is None else list(settings)
    B = int(base_u8.shape[0])
    rev = _flags(base_is_right, B, base_u8.device)
    memo, planes = {}, []
    for s in settings:
        key = s._replace(blockSize=s.window)
        if key not in memo:
            memo[key] = sgbm(base_u8, lookup_u8, s, reverse=rev).to(torch.float32) / 16.0
        planes.append(memo[key])
    return torch.stack(planes, dim=1)


def precompute_depth_hints(base_u8, lookup_u8, base_is_right, K, inv_K, baseline=0.1, settings=None):
    """KITTI/precompute_depth_hints.py for a batch of stereo pairs on the device: the candidates above, T = the identity with
    T[0, 3] = +baseline for a right-view base and -baseline for a left-view one (:159-174), and fuse_depth_hints.  K / inv_K
    float32 [B,4,4] in pixels of the images' size.  -> depth_hint_inputs(best_depth): "depth_hint" [B,1,H,W] and
    "depth_hint_mask"."""
    cand = depth_hint_candidates(base_u8, lookup_u8, base_is_right, settings)
    B = int(cand.shape[0])
    dev = cand.device
    rev = _flags(base_is_right, B, dev)
    T = torch.eye(4, device=dev, dtype=torch.float32).repeat(B, 1, 1)
    T[:, 0, 3] = (rev.to(torch.float32) * 2.0 - 1.0) * float(baseline)
    base, lookup = (t.unsqueeze(-1) if t.dim() == 3 else t for t in (base_u8, lookup_u8))
    base_f, lookup_f = (t.permute(0, 3, 1, 2).to(torch.float32) / 255 for t in (base, lookup))
    fbl = float((K[0, 0, 0].to(torch.float32).cpu() * torch.tensor(float(baseline), dtype=torch.float32)).item())
    best_depth, _ = depth_hints.fuse_depth_hints(cand, base_f.contiguous(), lookup_f.contiguous(), K, inv_K, T, disparities=True,
                                                 focal_times_baseline=fbl)
    return depth_hints.depth_hint_inputs(best_depth)
