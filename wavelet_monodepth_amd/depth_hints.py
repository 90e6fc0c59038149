"""Depth-hint fusion on the GPU (csrc/wmd_hints.hip): the selection step of KITTI/precompute_depth_hints.py.

    disparity_to_depth(disps, focal, baseline=0.1)        precompute_depth_hints.py:149
    fuse_depth_hints(candidates, base, lookup, K, inv_K, T)   :243-249 -- per pixel, the candidate depth whose reprojection
                                                          of the other stereo view has the smallest 0.85 SSIM + 0.15 L1
    depth_hint_inputs(best_depth)                         datasets/mono_dataset.py:264-265 -- what the trainer's loss reads

The candidates come from the caller, from any matcher: stereo.depth_hint_candidates makes them on the GPU with the reference's
twelve settings (the reference uses OpenCV SGBM on the host), and stereo.precompute_depth_hints chains it with this module.
One HIP launch, no autograd, no CPU fallback: CPU tensors raise.
"""
import torch

from . import _lib
from ._lib import check, current_stream, ptr

MAX_CANDIDATES = 64   # WMD_DEPTH_HINTS_MAX_CANDIDATES


def disparity_to_depth(disps, focal, baseline=0.1):
    """Pixel disparities -> depths, "ignoring missing pixels": focal * baseline / (d + 1e-7) * (d > 0).  `focal` is K[0, 0]
    in pixels of the map's width."""
    _lib.require_device("disparity_to_depth", disps=(disps, torch.float32))
    fb = (torch.tensor(float(focal), dtype=torch.float32) * baseline).to(disps.device)   # a float32 product, as in the reference
    return fb / (disps + 1e-7) * (disps > 0).float()   # tensor / tensor: a true division (scalar / tensor multiplies by a reciprocal)


def fuse_depth_hints(candidates, base_image, lookup_image, K, inv_K, T, *, disparities=False, focal_times_baseline=None,
                     return_losses=False, no_ssim=False):
    """candidates [B,M,H,W] (depths; pixel disparities with disparities=True, which needs focal_times_baseline), base_image /
    lookup_image [B,C,H,W] in [0,1], K / inv_K / T [B,4,4] (T per image: the baseline's sign follows the base image's side)
    -> best_depth [B,1,H,W], best_index [B,H,W] int32 (the lowest index among equal losses) and, with return_losses, the
    float32 losses [B,M,H,W] that were compared.
    The reference's single-image layout -- candidates [M,H,W], images [C,H,W], matrices [4,4] -- returns best_depth [1,H,W]
    (what the reference saves), best_index [H,W] and losses [M,H,W]."""
    single = candidates.dim() == 3
    if single:
        candidates, base_image, lookup_image, K, inv_K, T = (t.unsqueeze(0) for t in (candidates, base_image, lookup_image, K, inv_K, T))
    _lib.require_device("fuse_depth_hints", **{k: (v, torch.float32) for k, v in (("candidates", candidates), ("base_image", base_image),
                                                                                   ("lookup_image", lookup_image), ("K", K), ("inv_K", inv_K), ("T", T))})
    if candidates.dim() != 4 or base_image.dim() != 4:
        raise _lib.WmdError("candidates must be [B,M,H,W] or [M,H,W] and the images [B,C,H,W] or [C,H,W]")
    B, M, H, W = candidates.shape
    Cc = base_image.shape[1]
    if tuple(base_image.shape) != (B, Cc, H, W) or lookup_image.shape != base_image.shape:
        raise _lib.WmdError("base and lookup images must be [%d,C,%d,%d] (got %s, %s)" % (B, H, W, tuple(base_image.shape), tuple(lookup_image.shape)))
    for name, m in (("K", K), ("inv_K", inv_K), ("T", T)):
        if tuple(m.shape) != (B, 4, 4):
            raise _lib.WmdError("%s must be [%d,4,4] (got %s)" % (name, B, tuple(m.shape)))
    if disparities and focal_times_baseline is None:
        raise _lib.WmdError("disparities=True needs focal_times_baseline (K[0, 0] * baseline)")
    cand, base, look, K, inv_K, T = (t.detach().contiguous() for t in (candidates, base_image, lookup_image, K, inv_K, T))
    dev = cand.device
    best_depth = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32)
    best_index = torch.empty((B, H, W), device=dev, dtype=torch.int32)
    losses = torch.empty((B, M, H, W), device=dev, dtype=torch.float32) if return_losses else None
    l = _lib.lib()
    n = l.wmd_depth_hints_workspace_floats(B, M, H, W)
    ws = _lib.float_workspace(n, dev)
    w_ssim, w_l1 = (0.0, 1.0) if no_ssim else (0.85, 0.15)
    check(l.wmd_depth_hints_fuse(ptr(cand), 1 if disparities else 0, float(focal_times_baseline or 0.0), ptr(base), ptr(look), ptr(K),
                                 ptr(inv_K), ptr(T), ptr(best_depth), ptr(best_index), ptr(losses), B, M, Cc, H, W, 1e-7, w_ssim, w_l1,
                                 ptr(ws), n, current_stream()), "wmd_depth_hints_fuse")
    if single:
        best_depth, best_index, losses = best_depth[0], best_index[0], None if losses is None else losses[0]
    return (best_depth, best_index, losses) if return_losses else (best_depth, best_index)


def depth_hint_inputs(best_depth):
    """The two entries the trainer's loss reads (photometric.generate_images_pred / compute_losses with use_depth_hints):
    the hint and the mask of the pixels that have one.  Resizing to the training size stays with the caller."""
    return {"depth_hint": best_depth, "depth_hint_mask": (best_depth > 0).float()}
