"""The semi-global matcher's integer specification in numpy ("Semi-global stereo matching"), written from the rules
and not from the kernels: plain loops over pixels and directions, vectors only along the disparity axis (and along a row where
the rule has no dependence inside the row).  Every quantity is an exact integer; nothing saturates.

    sgbm(left, right, s, reverse=False) -> dict(cost [H,Wv,D], S [H,Wv,D], disp2 [H,W], raw [H,W], disp [H,W])

with Wv = W - maxD the width of the valid rectangle, `raw` the map before the speckle stage and `disp` the final int16 map.
`s` is any object with OpenCV's StereoSGBM parameter names as attributes (wavelet_monodepth_amd.stereo.SGBMSettings)."""
import collections

import numpy as np

PATHS5 = [(-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0)]          # predecessor offsets (dx, dy)
PATHS8 = PATHS5 + [(1, 1), (0, 1), (-1, 1)]

Settings = collections.namedtuple("Settings", "minDisparity numDisparities blockSize P1 P2 preFilterCap uniquenessRatio "
                                              "speckleWindowSize speckleRange disp12MaxDiff directions")


def reference_like(numDisparities=16, blockSize=3, minDisparity=0, directions=5, **kw):
    """the reference's settings (KITTI/precompute_depth_hints.py:49-59) with the given overrides"""
    base = dict(minDisparity=minDisparity, numDisparities=numDisparities, blockSize=blockSize, P1=36, P2=288, preFilterCap=63,
                uniquenessRatio=10, speckleWindowSize=100, speckleRange=16, disp12MaxDiff=0, directions=directions)
    base.update(kw)
    return Settings(**base)


def s_bound(s, C):
    win = 2 * (s.blockSize // 2) + 1
    return s.directions * (win * win * C * (2 * s.preFilterCap + 63) + s.P2)


def prefilter(img, cap):
    """img int [H,W,C] -> G: the clamped horizontal Sobel response, coordinates clamped to the image"""
    H, W, _ = img.shape
    p = np.pad(img, ((1, 1), (1, 1), (0, 0)), mode="edge")
    g = (p[0:H, 2:] - p[0:H, :W]) + 2 * (p[1:H + 1, 2:] - p[1:H + 1, :W]) + (p[2:, 2:] - p[2:, :W])
    return np.clip(g, -cap, cap) + cap


def interval(A):
    """[H,W,C] -> (lo, hi): the half-pixel interval along the row"""
    p = np.pad(A, ((0, 0), (1, 1), (0, 0)), mode="edge")
    a, b = (A + p[:, :-2]) >> 1, (A + p[:, 2:]) >> 1
    return np.minimum(A, np.minimum(a, b)), np.maximum(A, np.maximum(a, b))


def bt(v, v0, v1, u, u0, u1):
    zero = np.zeros_like(v)
    return np.minimum(np.maximum(zero, np.maximum(v - u1, u0 - v)), np.maximum(zero, np.maximum(u - v1, v0 - u)))


def pixel_cost(left, right, s):
    """-> pc [H,W,D]; columns left of x0 stay 0 and are never read"""
    H, W, _ = left.shape
    D, minD = s.numDisparities, s.minDisparity
    x0 = minD + D
    pc = np.zeros((H, W, D), dtype=np.int64)
    GL, GR = prefilter(left, s.preFilterCap), prefilter(right, s.preFilterCap)
    (gl0, gl1), (gr0, gr1) = interval(GL), interval(GR)
    (il0, il1), (ir0, ir1) = interval(left), interval(right)
    xs = np.arange(x0, W)
    for d in range(D):
        xr = xs - (d + minD)
        g = bt(GL[:, xs], gl0[:, xs], gl1[:, xs], GR[:, xr], gr0[:, xr], gr1[:, xr])
        i = bt(left[:, xs], il0[:, xs], il1[:, xs], right[:, xr], ir0[:, xr], ir1[:, xr]) >> 2
        pc[:, xs, d] = g.sum(-1) + i.sum(-1)
    return pc


def block_cost(pc, s):
    """-> C [H,Wv,D]: window rows clamped to the image, window columns to the valid rectangle"""
    H, W, D = pc.shape
    x0 = s.minDisparity + D
    r = s.blockSize // 2
    C = np.zeros((H, W - x0, D), dtype=np.int64)
    for y in range(H):
        for x in range(x0, W):
            acc = np.zeros(D, dtype=np.int64)
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    acc += pc[min(max(y + dy, 0), H - 1), min(max(x + dx, x0), W - 1)]
            C[y, x - x0] = acc
    return C


INF = 1 << 40


def path_cost(C, dx, dy, P1, P2):
    """L of one path; the predecessor of (x, y) is (x + dx, y + dy) inside the valid rectangle"""
    H, Wv, D = C.shape
    L = np.zeros_like(C)
    ys = range(H) if dy <= 0 else range(H - 1, -1, -1)
    xs = range(Wv) if dx <= 0 else range(Wv - 1, -1, -1)
    for y in ys:
        for x in xs:
            px, py = x + dx, y + dy
            if not (0 <= px < Wv and 0 <= py < H):
                L[y, x] = C[y, x]
                continue
            Lp = L[py, px]
            m = Lp.min()
            lo = np.concatenate(([INF], Lp[:-1])) + P1
            hi = np.concatenate((Lp[1:], [INF])) + P1
            L[y, x] = C[y, x] + np.minimum(np.minimum(Lp, lo), np.minimum(hi, m + P2)) - m
    return L


def aggregate(C, s):
    S = np.zeros_like(C)
    for dx, dy in (PATHS8 if s.directions == 8 else PATHS5):
        S += path_cost(C, dx, dy, s.P1, s.P2)
    return S


def trunc_div(a, b):
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def winners(S, W, s):
    """-> raw map before the left-right check [H,W], disp2 [H,W] (unset: minDisparity - 1)"""
    H, Wv, D = S.shape
    minD = s.minDisparity
    x0 = minD + D
    invalid = (minD - 1) * 16
    disp = np.full((H, W), invalid, dtype=np.int64)
    disp2 = np.full((H, W), minD - 1, dtype=np.int64)
    best2 = {}
    for y in range(H):
        for x in range(x0, W):
            Sp = [int(v) for v in S[y, x - x0]]
            minS = min(Sp)
            d = Sp.index(minS)
            x2 = x - (d + minD)
            if (y, x2) not in best2 or (minS, x) < best2[(y, x2)]:
                best2[(y, x2)] = (minS, x)
                disp2[y, x2] = d + minD
            if any(abs(k - d) > 1 and Sp[k] * (100 - s.uniquenessRatio) < minS * 100 for k in range(D)):
                continue
            val = (d + minD) * 16
            if 0 < d < D - 1:
                den = max(Sp[d - 1] + Sp[d + 1] - 2 * Sp[d], 1)
                val += trunc_div((Sp[d - 1] - Sp[d + 1]) * 16 + den, 2 * den)
            disp[y, x] = val
    return disp, disp2


def left_right_check(disp, disp2, s):
    H, W = disp.shape
    minD = s.minDisparity
    invalid = (minD - 1) * 16
    tol = s.disp12MaxDiff if s.disp12MaxDiff > 0 else 1
    out = disp.copy()
    for y in range(H):
        for x in range(W):
            d1 = int(disp[y, x])
            if d1 == invalid:
                continue
            a, b = d1 >> 4, (d1 + 15) >> 4

            def off(xx, dd):
                return 0 <= xx < W and disp2[y, xx] >= minD and abs(int(disp2[y, xx]) - dd) > tol
            if off(x - a, a) and off(x - b, b):
                out[y, x] = invalid
    return out


def filter_speckles(disp, invalid, max_size, max_diff):
    """[H,W] -> copy with every 4-connected component (neighbours both valid, |difference| <= max_diff) of at most max_size
    pixels set to `invalid`"""
    H, W = disp.shape
    out = disp.copy()
    seen = np.zeros((H, W), dtype=bool)
    for y in range(H):
        for x in range(W):
            if seen[y, x] or disp[y, x] == invalid:
                continue
            comp, todo = [], [(y, x)]
            seen[y, x] = True
            while todo:
                cy, cx = todo.pop()
                comp.append((cy, cx))
                for ny, nx in ((cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)):
                    if 0 <= ny < H and 0 <= nx < W and not seen[ny, nx] and disp[ny, nx] != invalid \
                            and abs(int(disp[ny, nx]) - int(disp[cy, cx])) <= max_diff:
                        seen[ny, nx] = True
                        todo.append((ny, nx))
            if len(comp) <= max_size:
                for cy, cx in comp:
                    out[cy, cx] = invalid
    return out


def sgbm(left, right, s, reverse=False):
    left, right = np.asarray(left).astype(np.int64), np.asarray(right).astype(np.int64)
    if left.ndim == 2:
        left, right = left[:, :, None], right[:, :, None]
    if reverse:
        left, right = left[:, ::-1], right[:, ::-1]
    H, W, C = left.shape
    assert W > s.minDisparity + s.numDisparities and s_bound(s, C) <= 65535
    cost = block_cost(pixel_cost(left, right, s), s)
    S = aggregate(cost, s)
    first, disp2 = winners(S, W, s)
    raw = left_right_check(first, disp2, s)
    invalid = (s.minDisparity - 1) * 16
    disp = filter_speckles(raw, invalid, s.speckleWindowSize, 16 * s.speckleRange) if s.speckleWindowSize > 0 else raw
    if reverse:
        disp2, raw, disp = disp2[:, ::-1], raw[:, ::-1], disp[:, ::-1]
    return {"cost": cost, "S": S, "disp2": disp2, "raw": raw.astype(np.int16), "disp": disp.astype(np.int16)}


def synthetic_pair(H=20, W=72, C=3, maxD=16, shifts=(5, 9), seed=0):
    """A random texture seen from two places: rows of the upper half are displaced by shifts[0], the others by shifts[1].
    -> left, right uint8 [H,W,C] and the true disparity per row; right[y, x] = left[y, x + shift]."""
    tex = np.random.default_rng(seed).integers(0, 256, (H, W + 2 * maxD, C)).astype(np.uint8)
    left = tex[:, maxD:maxD + W]
    right = np.empty_like(left)
    true = np.empty(H, dtype=np.int64)
    for y in range(H):
        sh = shifts[0] if y < H // 2 else shifts[1]
        right[y] = tex[y, maxD + sh:maxD + sh + W]
        true[y] = sh
    return np.ascontiguousarray(left), right, true
