"""CPU restatement of the NYUv2 depth-boundary errors in numpy + scipy.ndimage, float64 throughout: the reference the
depth-boundary tests compare against (everything but the Canny detector is itself pinned to the reference's
compute_depth_boundary_error by tests/golden/dbe_reference.npz, tests/test_dbe_oracle.py).

  canny(image, sigma, low, high)                      this project's definition of the detector, modelled on
                                                      skimage.feature.canny(image, sigma, low, high) with mask=None; no
                                                      skimage was at hand, so agreement with an actual skimage is unverified
  canny_stages(image, sigma, low, high)               the same with every intermediate plane and the decision margin
  normalise(pred)                                     NYUv2/utils.py:130-134 in float64 (the reference keeps float32 there)
  compute_depth_boundary_error(edges_gt, pred, ...)   NYUv2/utils.py:122-169 -> (dbe_acc, dbe_com, edges_est, margin)

The decision margin of an input is the smallest finite |lhs - rhs| over every comparison that decides an edge pixel: the
gradient magnitude against `low`, the two interpolated neighbours against the magnitude, the kept magnitude against
`high`.  An implementation whose arithmetic differs from this one by less than the margin finds the same edge map.
"""
import numpy as np
from scipy import ndimage

EPS = 2.220446049250313e-16
MAX_DIST = 10.0


def smooth(p, sigma):
    """G(p) / (G(ones) + eps) with zeros outside the image: the masked smoothing of the detector with an all-ones mask"""
    g = lambda a: ndimage.gaussian_filter(a, sigma, mode="constant", truncate=4.0)
    return g(p) / (g(np.ones(p.shape)) + EPS)


def canny_stages(image, sigma, low, high):
    p = np.asarray(image, dtype=np.float64)
    H, W = p.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        sm = smooth(p, sigma)
        jsobel = ndimage.sobel(sm, axis=1)
        isobel = ndimage.sobel(sm, axis=0)
        mag = np.hypot(isobel, jsobel)
        inner = np.zeros((H, W), bool)
        inner[1:-1, 1:-1] = True
        examined = inner & (mag >= low)
        ai, aj = np.abs(isobel), np.abs(jsobel)
        c1 = ((isobel >= 0) & (jsobel >= 0)) | ((isobel <= 0) & (jsobel <= 0))
        c2 = ((isobel <= 0) & (jsobel >= 0)) | ((isobel >= 0) & (jsobel <= 0))
        case = [c1 & (ai > aj), c1 & ~(ai > aj), ~c1 & c2 & (ai < aj), ~c1 & c2 & ~(ai < aj)]
        w = np.where(case[0] | case[3], aj / ai, ai / aj)
        pad = np.pad(mag, 1, constant_values=0.0)
        at = lambda di, dj: pad[1 + di:1 + di + H, 1 + dj:1 + dj + W]     # mag[x + di, y + dj]
        # (a, b) on the positive side; the negative side is the point reflection
        nb = [((1, 0), (1, 1)), ((0, 1), (1, 1)), ((0, 1), (-1, 1)), ((-1, 0), (-1, 1))]
        lhs_p = np.full((H, W), np.nan)
        lhs_n = np.full((H, W), np.nan)
        for c, (a, b) in zip(case, nb):
            lhs_p = np.where(c, at(*b) * w + at(*a) * (1 - w), lhs_p)
            lhs_n = np.where(c, at(-b[0], -b[1]) * w + at(-a[0], -a[1]) * (1 - w), lhs_n)
        keep = examined & (lhs_p <= mag) & (lhs_n <= mag)
        out = np.where(keep, mag, 0.0)
    weak = out > 0
    strong = weak & (out >= high)
    labels, n = ndimage.label(weak, structure=np.ones((3, 3)))
    good = np.zeros(n + 1, bool)
    good[np.unique(labels[strong])] = True
    good[0] = False
    edges = good[labels]
    gaps = [np.abs(mag - low)[inner], np.abs(lhs_p - mag)[examined], np.abs(lhs_n - mag)[examined], np.abs(out - high)[weak]]
    gaps = np.concatenate([g.ravel() for g in gaps])
    gaps = gaps[np.isfinite(gaps)]
    margin = float(gaps.min()) if gaps.size else np.inf
    return dict(smoothed=sm, isobel=isobel, jsobel=jsobel, mag=mag, out=out, weak=weak, strong=strong, edges=edges, margin=margin)


def canny(image, sigma=1.0, low_threshold=0.1, high_threshold=0.2):
    return canny_stages(image, sigma, low_threshold, high_threshold)["edges"]


def normalise(pred):
    p = np.array(pred, dtype=np.float64)
    p[p == 0] = np.nan
    with np.errstate(invalid="ignore", divide="ignore"):
        if np.isnan(p).all():
            return p
        p = p - np.nanmin(p)
        return p / np.nanmax(p)


def chamfer_scores(edges_gt, edges_est, mask=None):
    """NYUv2/utils.py:140-167 on two binary maps with at least one ground-truth edge pixel"""
    edges_gt, edges_est = (np.asarray(edges_gt) != 0).astype(np.float64), (np.asarray(edges_est) != 0).astype(np.float64)
    mask = np.ones(edges_gt.shape) if mask is None else (np.asarray(mask) != 0).astype(np.float64)
    d_gt = ndimage.distance_transform_edt(1 - edges_gt)
    f = edges_est * (d_gt < MAX_DIST) * mask
    if f.sum() == 0:
        return MAX_DIST, MAX_DIST
    d_est = ndimage.distance_transform_edt(1 - edges_est)
    acc = (d_gt * mask * f).sum() / f.sum()
    com = (np.minimum(d_gt * mask, MAX_DIST) * edges_est).sum() + (np.minimum(d_est, MAX_DIST) * edges_gt).sum()
    return float(acc), float(com / (edges_est.sum() + edges_gt.sum()))


def compute_depth_boundary_error(edges_gt, pred, mask=None, low_thresh=0.15, high_thresh=0.3):
    """-> (dbe_acc, dbe_com, edges_est bool [H,W], margin).  No ground-truth edge: (nan, nan) and an empty map (the
    reference assigns those and then fails on an unbound D_est, NYUv2/utils.py:169)."""
    edges_gt = np.asarray(edges_gt) != 0
    if not edges_gt.any():
        return np.nan, np.nan, np.zeros(edges_gt.shape, bool), np.inf
    st = canny_stages(normalise(pred), np.sqrt(2), low_thresh, high_thresh)
    acc, com = chamfer_scores(edges_gt, st["edges"], mask)
    return acc, com, st["edges"], st["margin"]
