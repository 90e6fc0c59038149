"""Float64 numpy oracle of generate_depth_map (KITTI/kitti_utils.py:73-104), vectorised, by the six rules of include/wmd.h
(wmd_lidar_depth_maps).  numpy only.

    project(points, P, shape)                   -> the valid points in file order: u, v (int64), x, p_2, the rounding ties among them
    depth_map(points, P, shape, vel_depth)      -> [H,W] float64, the reference's result
    depth_map(..., rule="last_wins")            rule 4 alone: no duplicate handling
    depth_map(..., rule="pixel_min")            the closest point per PIXEL -- what the duplicate step is commonly taken to do
The two variants exist so that the tests can show that a case tells them apart from the reference's bucket rule.
"""
import numpy as np

RULES = ("reference", "last_wins", "pixel_min")


def project(points, P, shape):
    H, W = shape
    P = np.asarray(P, np.float64)
    pts = np.asarray(points, np.float32)
    pts = pts[pts[:, 0] >= 0]                                    # rule 1: keeps -0.0, drops NaN
    x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        p = [((P[r, 0] * x + P[r, 1] * y) + P[r, 2] * z) + P[r, 3] for r in range(3)]   # rule 2: numpy never fuses
        qu, qv = p[0] / p[2], p[1] / p[2]
        u, v = np.rint(qu) - 1, np.rint(qv) - 1
        ok = (u >= 0) & (v >= 0) & (u < W) & (v < H)             # rule 3, in float64
        tie = (np.abs(qu - np.trunc(qu)) == 0.5) | (np.abs(qv - np.trunc(qv)) == 0.5)
    return {"u": u[ok].astype(np.int64), "v": v[ok].astype(np.int64), "x": x[ok], "p2": p[2][ok], "tie": tie[ok],
            "zero_p2": int((p[2] == 0).sum())}                   # kept points with p_2 = 0: inf or NaN, never valid


def depth_map(points, P, shape, vel_depth, rule="reference"):
    assert rule in RULES
    H, W = shape
    g = project(points, P, shape)
    u, v, val = g["u"], g["v"], g["x"] if vel_depth else g["p2"]
    n, order = len(u), np.arange(len(u))
    pixel = v * W + u
    flat = np.zeros(H * W, np.float64)
    if rule == "pixel_min":
        best = np.full(H * W, np.inf)
        np.minimum.at(best, pixel, val)
        flat[np.isfinite(best)] = best[np.isfinite(best)]
    else:
        last = np.full(H * W, -1, np.int64)
        np.maximum.at(last, pixel, order)                        # rule 4: the highest index at the pixel
        flat[last >= 0] = val[last[last >= 0]]
    if rule == "reference" and n:
        key = v * (W - 1) + u                                    # rule 5: sub2ind + 1, 0 .. H (W - 1)
        nk = H * (W - 1) + 1
        count = np.bincount(key, minlength=nk)
        first = np.full(nk, n, np.int64)
        np.minimum.at(first, key, order)
        kmin = np.full(nk, np.inf)
        np.minimum.at(kmin, key, val)
        dup = count > 1
        flat[pixel[first[dup]]] = kmin[dup]
    flat[flat < 0] = 0                                           # rule 6
    return flat.reshape(H, W)


def coverage(points, P, shape):
    """What a case exercises: valid points, rounding ties and negative p_2 among them, kept points with p_2 = 0, pixels hit
    more than once, buckets that join two different pixels (-1: not counted for a large case)."""
    H, W = shape
    g = project(points, P, shape)
    pixel, key = g["v"] * W + g["u"], g["v"] * (W - 1) + g["u"]
    joined = sum(1 for k in np.unique(key) if len(np.unique(pixel[key == k])) > 1) if len(key) < 5000 else -1
    return {"valid": len(pixel), "ties": int(g["tie"].sum()), "negative_p2": int((g["p2"] < 0).sum()), "zero_p2": g["zero_p2"],
            "duplicate_pixels": int((np.bincount(pixel, minlength=1) > 1).sum()), "joined_buckets": joined}
