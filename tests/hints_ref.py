"""float64 restatement of the depth-hint selection (KITTI/precompute_depth_hints.py:149 and :243-249) on top of
oracle/photo_ref.py's warp_frame and compute_reprojection_loss, which the photometric fixtures pin to the reference's own
layers.  TEST INFRASTRUCTURE ONLY: numpy in, numpy out, torch-CPU in between."""
import numpy as np
import torch

from oracle import photo_ref as P


def disparity_to_depth(d, fbl):
    """focal * baseline / (d + 1e-7) * (d > 0), in float64 on the float32 inputs"""
    d = np.asarray(d, np.float64)
    return float(fbl) / (d + 1e-7) * (d > 0)


def losses(case, dtype=torch.float64, use_ssim=True):
    """-> [B,M,H,W] float64: the reprojection loss of every candidate, the M maps of one image as a batch of M like the
    reference's script"""
    cand = case["cand"]
    B, M, H, W = cand.shape
    depth = disparity_to_depth(cand, case["fbl"]) if case["disparities"] else np.asarray(cand, np.float64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    out = np.empty((B, M, H, W))
    for b in range(B):
        rep = lambda a: t(a[b]).unsqueeze(0).expand(M, *a.shape[1:]).contiguous()
        warped = P.warp_frame(rep(case["lookup"]), t(depth[b]).unsqueeze(1), rep(case["K"]), rep(case["inv_K"]), rep(case["T"]))
        out[b] = P.compute_reprojection_loss(warped, rep(case["base"]), use_ssim)[:, 0].double().numpy()
    return out


def first_argmin(l):
    """[B,M,H,W] -> [B,H,W]: the lowest index among the smallest values (numpy's and torch-CPU's argmin)"""
    return np.argmin(l, axis=1)


def gather(depths, index):
    return np.take_along_axis(depths, index[:, None].astype(np.int64), axis=1)[:, 0]


def decisive(l64, depths, tol_loss):
    """[B,H,W] bool: the float64 gap between the best candidate and the best candidate with another depth value exceeds
    2 tol_loss (a pixel all of whose candidates share one depth value is decisive)"""
    best = first_argmin(l64)
    dbest = gather(depths, best)
    other = np.where(depths != dbest[:, None], l64, np.inf).min(1)
    return other - l64.min(1) > 2.0 * tol_loss
