"""The contract of the three-pass Winograd F(4x4,3x3) convolution (wmd_conv_wino44_fwd) as numpy, in float64: the transform
matrices, the 5-term map of an upsampled line, tile and border folding.  The tests hold the kernels to this statement, and this
statement to a direct convolution."""
import numpy as np

# points 0, +-1, +-2, inf
BT = np.array([[4, 0, -5, 0, 1, 0],
               [0, -4, -4, 1, 1, 0],
               [0, 4, -4, -1, 1, 0],
               [0, -2, -1, 2, 1, 0],
               [0, 2, -1, -2, 1, 0],
               [0, 4, 0, -5, 0, 1]], dtype=np.float64)
G = np.array([[1 / 4, 0, 0],
              [-1 / 6, -1 / 6, -1 / 6],
              [-1 / 6, 1 / 6, -1 / 6],
              [1 / 24, 1 / 12, 1 / 6],
              [1 / 24, -1 / 12, 1 / 6],
              [0, 0, 1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 1, 1, 0],
               [0, 1, -1, 2, -2, 0],
               [0, 1, 1, 4, 4, 0],
               [0, 1, -1, 8, -8, 1]], dtype=np.float64)

UP_POS = (0, 1, 3, 4, 5)     # 1-D positions a replicated line (a, b, b, c, c, e) reaches: B^T d is identically 0 at position 2
# (a, b, c, e) -> (4a - 5b + c, -8b + 2c, -3 (b - c), b - c, 4b - 5c + e)
BT_UP = np.array([[4, -5, 1, 0],
                  [0, -8, 2, 0],
                  [0, -3, 3, 0],
                  [0, 1, -1, 0],
                  [0, 4, -5, 1]], dtype=np.float64)
G_UP = G[list(UP_POS)]       # the weight rows that go with them


def fold(g, n, pad):
    """Padded coordinate g (-1 .. n + 3) of an n-sample line -> source index, or -1 for "reads 0": beyond n only the discarded
    outputs of a ragged tile are reached."""
    if g > n:
        return -1
    if 0 <= g < n:
        return g
    if pad == "zero":
        return -1
    if pad == "reflect":
        return -g if g < 0 else 2 * n - 2 - g
    return 0 if g < 0 else n - 1


def fold_low(s, n1, pad):
    """Sample s (2t-1 .. 2t+2) of the low-resolution line behind an upsampled one -> source index or -1: clamped into the line
    (the reflected and the replicated border sample of the upsampled line are both its edge sample), 0 under zero padding."""
    if 0 <= s < n1:
        return s
    return -1 if pad == "zero" else min(max(s, 0), n1 - 1)


def gather(x, rows, cols):
    """x [..., H, W] at the index grids rows x cols, 0 where an index is -1."""
    r, c = np.asarray(rows), np.asarray(cols)
    out = x[..., np.maximum(r, 0)[:, None], np.maximum(c, 0)[None, :]]
    return out * ((r >= 0)[:, None] & (c >= 0)[None, :])


def direct(x1, w, bias=None, x2=None, up1=1, pad="reflect"):
    """float64 direct form of the operator: conv3x3(pad(cat[nearest_up(x1), x2])) + bias."""
    x = np.asarray(x1, np.float64)
    if up1 == 2:
        x = x.repeat(2, axis=2).repeat(2, axis=3)
    if x2 is not None:
        x = np.concatenate([x, np.asarray(x2, np.float64)], axis=1)
    w = np.asarray(w, np.float64)
    H, W = x.shape[2:]
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)), mode={"zero": "constant", "reflect": "reflect", "replicate": "edge"}[pad])
    y = np.zeros((x.shape[0], w.shape[0], H, W))
    for i in range(3):
        for j in range(3):
            y += np.einsum("bchw,oc->bohw", xp[:, :, i:i + H, j:j + W], w[:, :, i, j])
    return y if bias is None else y + np.asarray(bias, np.float64)[None, :, None, None]


def weights_full(w):
    """[Cout, C, 3, 3] -> U [6, 6, C, Cout]"""
    return np.einsum("ai,ocij,bj->abco", G, np.asarray(w, np.float64), G)


def weights_up(w):
    """[Cout, C, 3, 3] -> the 25 positions [5, 5, C, Cout] an upsampled operand reaches"""
    return np.einsum("ai,ocij,bj->abco", G_UP, np.asarray(w, np.float64), G_UP)


def wino44(x1, w, bias=None, x2=None, up1=1, pad="reflect", structured=True):
    """The three passes in float64.  structured: the upsampled operand is read at its own resolution (25 positions); False:
    it is upsampled first and takes the full 36-position path."""
    x1 = np.asarray(x1, np.float64)
    w = np.asarray(w, np.float64)
    C1 = x1.shape[1]
    if up1 == 2 and not structured:
        x1 = x1.repeat(2, axis=2).repeat(2, axis=3)
    low = up1 == 2 and structured
    B = x1.shape[0]
    H, W = (x1.shape[2] * 2, x1.shape[3] * 2) if low else x1.shape[2:]
    th, tw = -(-H // 4), -(-W // 4)
    Uf1, Uu1 = weights_full(w[:, :C1]), weights_up(w[:, :C1])
    U2 = weights_full(w[:, C1:]) if x2 is not None else None
    y = np.zeros((B, w.shape[0], 4 * th, 4 * tw))
    for ty in range(th):
        for tx in range(tw):
            M = np.zeros((B, 6, 6, w.shape[0]))
            if low:
                rows = [fold_low(2 * ty - 1 + i, x1.shape[2], pad) for i in range(4)]
                cols = [fold_low(2 * tx - 1 + i, x1.shape[3], pad) for i in range(4)]
                V = np.einsum("ai,bcij,dj->badc", BT_UP, gather(x1, rows, cols), BT_UP)
                M[:, np.ix_(UP_POS, UP_POS)[0], np.ix_(UP_POS, UP_POS)[1]] += np.einsum("badc,adco->bado", V, Uu1)
            else:
                rows = [fold(4 * ty - 1 + i, H, pad) for i in range(6)]
                cols = [fold(4 * tx - 1 + i, W, pad) for i in range(6)]
                M += np.einsum("badc,adco->bado", np.einsum("ai,bcij,dj->badc", BT, gather(x1, rows, cols), BT), Uf1)
            if x2 is not None:
                rows = [fold(4 * ty - 1 + i, H, pad) for i in range(6)]
                cols = [fold(4 * tx - 1 + i, W, pad) for i in range(6)]
                V2 = np.einsum("ai,bcij,dj->badc", BT, gather(np.asarray(x2, np.float64), rows, cols), BT)
                M += np.einsum("badc,adco->bado", V2, U2)
            y[:, :, 4 * ty:4 * ty + 4, 4 * tx:4 * tx + 4] = np.einsum("ia,bado,jd->boij", AT, M, AT)
    y = y[:, :, :H, :W]
    return y if bias is None else y + np.asarray(bias, np.float64)[None, :, None, None]


def tiles(B, H, W):
    return B * (-(-H // 4)) * (-(-W // 4))


def round_up(v, m):
    return -(-v // m) * m


def workspace_floats(B, H, W, C1, C2, Cout):
    """V [36][C1p + C2p][NTp] + M [36][Coutp][NTp]: channels rounded up to 32 each, Cout to 32, tiles to 32"""
    ntp = round_up(tiles(B, H, W), 32)
    return 36 * ntp * (round_up(C1, 32) + round_up(C2, 32) + round_up(Cout, 32))


def weight_floats(C1, C2, Cout):
    return 36 * (round_up(C1, 32) + round_up(C2, 32)) * round_up(Cout, 32)
