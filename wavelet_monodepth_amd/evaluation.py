"""Evaluation arithmetic on the GPU: what KITTI/evaluate_depth.py and NYUv2/utils.py do per
image in numpy on the host, for whole batches resident in HBM, through libwmd_hip.so (csrc/wmd_eval.hip, csrc/wmd_dbe.hip).

    kitti_metrics(pred_disp, gt_depth, ...)      evaluate_depth.py:268-307 + compute_errors (:50-68)
    flip_postprocess(l_disp, r_disp_raw)         evaluate_depth.py:71-79 with the [:, :, ::-1] of :204 fused
    compute_errors(pred, gt)                     evaluate_depth.py:50-68 on prepared arrays
    compute_errors_nyu(pred, gt)                 NYUv2/utils.py:85-98
    nyu_prediction(pred_y, crop)                 NYUv2/utils.py:213-226,247-250
    compute_depth_boundary_error(edges_gt, pred) NYUv2/utils.py:122-169: the dbe_acc / dbe_com columns of --eval_edges
    canny(image, sigma, low, high)               the edge detector behind it: this project's definition, modelled on
                                                 skimage.feature.canny with mask=None (include/wmd.h states it in full;
                                                 agreement with an actual skimage is not verified)
No CPU fallback: CPU tensors raise.
"""
import ctypes as C

import torch

from . import _lib, ops
from ._lib import check, current_stream, ptr

KITTI_NAMES = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")
NYU_NAMES = ("abs_rel", "rmse", "log_10", "a1", "a2", "a3")
NYU_EDGE_NAMES = ("dbe_acc", "dbe_com")
MIN_DEPTH, MAX_DEPTH, STEREO_SCALE_FACTOR = 1e-3, 80.0, 5.4


def kitti_metrics(pred_disp, gt_depth, eval_split="eigen", eval_stereo=False, disable_median_scaling=False,
                  pred_depth_scale_factor=1.0, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH):
    """pred_disp [B,h,w] (network resolution), gt_depth [B,H,W] -> (errors [B,7] in KITTI_NAMES order, ratios [B] or
    None, n_valid [B]).  Options follow evaluate_depth.py:263-270: stereo evaluation disables median scaling and scales
    by 5.4."""
    _lib.require_device("kitti_metrics", pred_disp=(pred_disp, torch.float32), gt_depth=(gt_depth, torch.float32))
    if eval_stereo:
        disable_median_scaling, pred_depth_scale_factor = True, STEREO_SCALE_FACTOR
    l = _lib.lib()
    pred_disp, gt_depth = pred_disp.contiguous(), gt_depth.contiguous()
    B, h, w = pred_disp.shape
    Bg, H, W = gt_depth.shape
    if B != Bg:
        raise _lib.WmdError("batch mismatch: %d predictions, %d ground-truth maps" % (B, Bg))
    n = l.wmd_eval_workspace_floats(B, H, W)
    ws = _lib.float_workspace(n, pred_disp.device)
    out = torch.empty((B, 9), device=pred_disp.device, dtype=torch.float32)
    a = _lib.EvalKittiArgs(B=B, h=h, w=w, H=H, W=W, min_depth=float(min_depth), max_depth=float(max_depth),
                           mask_mode=1 if eval_split == "eigen" else 0, pred_scale=float(pred_depth_scale_factor),
                           median_scaling=0 if disable_median_scaling else 1, pred_disp=ptr(pred_disp), gt_depth=ptr(gt_depth),
                           out=ptr(out), workspace=ptr(ws), workspace_floats=n)
    check(l.wmd_eval_kitti(C.byref(a), current_stream()), "wmd_eval_kitti")
    ratios = None
    if not disable_median_scaling:
        med = ws[2 * B * H * W + B:2 * B * H * W + 3 * B].view(B, 2)
        ratios = med[:, 1] / med[:, 0]
    return out[:, :7], ratios, out[:, 8].to(torch.int64)


def _errors9(pred, gt):
    _lib.require_device("compute_errors", pred=(pred, torch.float32), gt=(gt, torch.float32))
    if pred.shape != gt.shape:
        raise _lib.WmdError("shape mismatch %s vs %s" % (tuple(pred.shape), tuple(gt.shape)))
    pred, gt = pred.contiguous(), gt.contiguous()
    B = pred.shape[0] if pred.dim() > 1 else 1
    out = torch.empty((B, 9), device=pred.device, dtype=torch.float32)
    check(_lib.lib().wmd_eval_errors(ptr(pred), ptr(gt), B, pred.numel() // B, ptr(out), current_stream()), "wmd_eval_errors")
    return out


def compute_errors(gt, pred):
    """KITTI compute_errors per leading-dimension item: [B,7] (argument order of the reference: gt first).  The reference
    calls it once per image and averages the rows afterwards (evaluate_depth.py:305-313), which is what the rows are for."""
    return _errors9(pred, gt)[:, :7]


def compute_errors_nyu(pred, gt, per_image=False):
    """NYUv2/utils.py:85-98: (abs_rel, rmse, log_10, a1, a2, a3) as a [6] tensor — ONE reduction over every element of the
    arrays handed in, as the reference computes them over its whole concatenated test set (rmse = sqrt of the GLOBAL mean
    squared error: averaging per-image rmse values afterwards gives a different, non-comparable number).
    per_image=True: one row per leading-dimension item, [B,6], for per-frame diagnostics."""
    if per_image:
        o = _errors9(pred, gt)
        return torch.stack([o[:, 0], o[:, 2], o[:, 7], o[:, 4], o[:, 5], o[:, 6]], 1)
    o = _errors9(pred.reshape(1, -1), gt.reshape(1, -1))[0]
    return torch.stack([o[0], o[2], o[7], o[4], o[5], o[6]])


def flip_postprocess(l_disp, r_disp_raw):
    """Monodepth-v1 post-processing; r_disp_raw is the prediction for the mirrored image, not flipped back."""
    _lib.require_device("flip_postprocess", l_disp=(l_disp, torch.float32), r_disp_raw=(r_disp_raw, torch.float32))
    l_disp, r_disp_raw = l_disp.contiguous(), r_disp_raw.contiguous()
    B, h, w = l_disp.shape
    out = torch.empty_like(l_disp)
    check(_lib.lib().wmd_flip_postprocess(ptr(l_disp), ptr(r_disp_raw), ptr(out), B, h, w, current_stream()), "wmd_flip_postprocess")
    return out


def nyu_prediction(pred_y, crop, border_crop_size=16):
    """NYUv2/utils.py:213-226,247-250 on the GPU: pred_y [B,1,H,W] (already / 100) -> [B, crop rows, crop cols]."""
    _lib.require_device("nyu_prediction", pred_y=(pred_y, torch.float32))
    t = ops.upsample_bilinear(pred_y, (240 - border_crop_size, 320 - border_crop_size), align_corners=True)
    t = torch.nn.functional.pad(t, (border_crop_size // 2,) * 4, mode="replicate")
    t = ops.upsample_bilinear(t, (2 * t.shape[2], 2 * t.shape[3]), align_corners=True)
    t = torch.clamp(t, min=0.4, max=10)
    return t[:, 0, crop[0]:crop[1] + 1, crop[2]:crop[3] + 1]


def _u8(t, what, shape):
    """bool / uint8 / float map, nonzero = set -> contiguous uint8 of 0 / 1"""
    _lib.require_device("compute_depth_boundary_error", **{what: (t, None)})   # any dtype: nonzero = set
    if tuple(t.shape) != tuple(shape):
        raise _lib.WmdError("%s has shape %s, expected %s" % (what, tuple(t.shape), tuple(shape)))
    return (t != 0).to(torch.uint8).contiguous()


def canny(image, sigma=1.0, low_threshold=0.1, high_threshold=0.2):
    """image [B,H,W] (or [H,W]) float32 -> bool edge map of the same shape.  Gaussian smoothing with zeros outside the
    image, Sobel gradients, non-maximum suppression against the interpolated neighbours along the gradient, hysteresis over
    8-connected components; thresholds are absolute, all arithmetic float64, NaN pixels spread and never become edges.
    Modelled on skimage.feature.canny(image, sigma, low_threshold, high_threshold) with mask=None; skimage was not at hand
    when this was written, so the agreement is by construction only."""
    _lib.require_device("canny", image=(image, torch.float32))
    img = image.contiguous()
    if img.dim() == 2:
        img = img[None]
    if img.dim() != 3:
        raise _lib.WmdError("canny expects [B,H,W] or [H,W], got %s" % (tuple(image.shape),))
    B, H, W = img.shape
    edges = torch.empty((B, H, W), device=img.device, dtype=torch.uint8)
    ws, n = _lib.byte_workspace(_lib.lib().wmd_eval_dbe_workspace_bytes(B, H, W), img.device)
    check(_lib.lib().wmd_eval_canny(ptr(img), ptr(edges), B, H, W, float(sigma), float(low_threshold), float(high_threshold),
                                    ptr(ws), n, current_stream()), "wmd_eval_canny")
    return edges.bool().view(image.shape)


def compute_depth_boundary_error(edges_gt, pred, mask=None, low_thresh=0.15, high_thresh=0.3):
    """NYUv2/utils.py:122-169 for a batch: pred [B,H,W] float32, edges_gt [B,H,W] (bool, uint8 or float, nonzero = edge),
    mask [B,H,W] binary or None -> (scores [B,2] float32 in NYU_EDGE_NAMES order, edges_est bool [B,H,W]).
    The prediction is normalised to 0..1 over its non-zero pixels (zeros become NaN holes), edges_est = canny(sigma=sqrt 2)
    with the two thresholds, and the scores are the directed (dbe_acc) and the symmetric, truncated (dbe_com) chamfer
    distances between the two edge maps; (10, 10) when no predicted edge lies within 10 pixels of a ground-truth edge.
    An image without ground-truth edges scores (nan, nan) with an empty edge map: the reference assigns those values and
    then fails on an unbound D_est in its return statement (:169).  Deterministic: the same input gives the same bits.
    The reference is called once per image on the host (NYUv2/utils.py:262-266); this is one call per batch."""
    _lib.require_device("compute_depth_boundary_error", pred=(pred, torch.float32))
    if pred.dim() != 3:
        raise _lib.WmdError("compute_depth_boundary_error expects pred [B,H,W], got %s" % (tuple(pred.shape),))
    pred = pred.contiguous()
    B, H, W = pred.shape
    gt = _u8(edges_gt, "edges_gt", pred.shape)
    m = None if mask is None else _u8(mask, "mask", pred.shape)
    scores = torch.empty((B, 2), device=pred.device, dtype=torch.float32)
    edges = torch.empty((B, H, W), device=pred.device, dtype=torch.uint8)
    ws, n = _lib.byte_workspace(_lib.lib().wmd_eval_dbe_workspace_bytes(B, H, W), pred.device)
    check(_lib.lib().wmd_eval_dbe(ptr(pred), ptr(gt), ptr(m), ptr(scores), ptr(edges), B, H, W, float(low_thresh),
                                  float(high_thresh), ptr(ws), n, current_stream()), "wmd_eval_dbe")
    return scores, edges.bool()
