"""The contract of the three-pass Winograd F(4x4,3x3) convolution (wmd_conv_wino44_fwd) as numpy, in float64: the transform
matrices, the 5-term map of an upsampled line, tile and border folding.  The tests hold the kernels to this statement, and this
statement to a direct convolution.  Below the contract: the three images a launch leaves behind (U, V, M) in the kernels' own
layouts, pass by pass, in float64 and in float32 (tests/test_gpu_wino44_pins.py holds each pass to them)."""
import collections

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


# ---- the three images of a launch, in the kernels' own layouts (header of wmd_conv_wino44.hip) --------------------------------------
Dims = collections.namedtuple("Dims", "C1p C2p Ktot Coutp th tw NT NTp u_floats v_floats m_floats")
KC, BM = 32, 64                                              # channels per staged chunk of the GEMM, out channels per GEMM block
LONG = tuple(6 * i + j for i in UP_POS for j in UP_POS)      # the 25 positions an upsampled operand reaches
SHORT = tuple(p for p in range(36) if p not in LONG)         # ... and the 11 it does not


def dims(B, H, W, C1, C2, Cout):
    """w44_dims: channels padded to 32 each, Cout to 32, tiles to 32; the workspace is V then M"""
    C1p, C2p, Coutp = round_up(C1, KC), round_up(C2, KC), round_up(Cout, 32)
    th, tw = -(-H // 4), -(-W // 4)
    NT = B * th * tw
    NTp = round_up(NT, 32)
    Ktot = C1p + C2p
    return Dims(C1p, C2p, Ktot, Coutp, th, tw, NT, NTp, 36 * Ktot * Coutp, 36 * Ktot * NTp, 36 * Coutp * NTp)


def blocks(d, up1):
    """The GEMM's grid and reduction of a layer with dims d: out-channel blocks, tile blocks and chunks of the positions that
    reduce over every channel (blocks of 64 tiles when the layer is split, of 128 otherwise) and of the 11 short ones."""
    split = up1 == 2
    return dict(split=split, nbm=-(-d.Coutp // BM), nbn_long=-(-d.NTp // 64), nbn_short=-(-d.NTp // 128),
                chunks_full=d.Ktot // KC, chunks_short=d.C2p // KC if split else None)


def kbeg(p, up1, C1p):
    """first channel of position p's reduction: the short positions of a split layer skip x1's channels"""
    return C1p if up1 == 2 and p in SHORT else 0


def pack4(img):
    """[36][K][R] -> [36][K / 4][R][4]: four consecutive channels innermost"""
    n, K, R = img.shape
    return np.ascontiguousarray(img.reshape(n, K // 4, 4, R).transpose(0, 1, 3, 2))


def unpack4(img):
    """[36][K / 4][R][4] -> [36][K][R]"""
    n, K4, R, _ = img.shape
    return np.ascontiguousarray(img.transpose(0, 1, 3, 2).reshape(n, K4 * 4, R))


def activate(y, act, slope=0.0):
    """in y's own precision"""
    if act == "elu":
        return np.where(y > 0, y, np.expm1(np.minimum(y, 0)))
    if act == "leaky":
        return np.where(y > 0, y, y * y.dtype.type(slope))
    if act == "sigmoid":
        return 1 / (1 + np.exp(-y))
    assert act == "none", act
    return y


def weight_image(w, C1, up1):
    """U = G g G^T in float64, [36][Ktot][Coutp] (channel-major: pack4 gives the kernel's layout): zero in every padded row and
    column and, for an upsampled x1, in its channels at the 11 positions it does not reach."""
    w = np.asarray(w, np.float64)
    Cout, C = w.shape[:2]
    d = dims(1, 4, 4, C1, C - C1, Cout)
    U = np.zeros((36, d.Ktot, d.Coutp))
    full = weights_full(w).reshape(36, C, Cout)
    U[:, :C1, :Cout] = full[:, :C1]
    U[:, d.C1p:d.C1p + C - C1, :Cout] = full[:, C1:]
    if up1 == 2:
        U[list(SHORT), :d.C1p] = 0.0
    return U


def _patches(x, rows, cols):
    """x [B, C, H, W] at the per-tile index lists rows [th][n], cols [tw][n] (-1: reads 0) -> [B, C, th, n, tw, n]"""
    r, c = np.asarray(rows), np.asarray(cols)
    out = x[:, :, np.maximum(r, 0)[:, :, None, None], np.maximum(c, 0)[None, None, :, :]]
    return out * ((r >= 0)[:, :, None, None] & (c >= 0)[None, None, :, :])


def _transform(T, patches, dtype):
    """T d T^T per tile, the column pass rounded to dtype before the row pass: [B, C, th, n, tw, n] -> [len(T)^2][C][B th tw]"""
    T = T.astype(dtype)
    t = np.einsum("ai,bcyixj->bcyaxj", T, patches.astype(dtype)).astype(dtype)
    v = np.einsum("bcyaxj,dj->adcbyx", t, T).astype(dtype)
    return v.reshape(T.shape[0] ** 2, v.shape[2], -1)


def input_image(x1, x2, up1, pad, dtype=np.float64, absolute=False):
    """V = B^T d B [36][Ktot][NTp] (channel-major) and the mask of the entries the input pass leaves untouched: the structured
    25-position form for an upsampled x1, the full form otherwise; dead channels and dead tiles are 0.  absolute: |B^T| |d| |B|
    instead, the scale that bounds the rounding error of a position whatever cancels in it."""
    x1 = np.asarray(x1)
    B, C1 = x1.shape[:2]
    H, W = x1.shape[2] * up1, x1.shape[3] * up1
    C2 = 0 if x2 is None else x2.shape[1]
    d = dims(B, H, W, C1, C2, 1)
    prep = (lambda a: np.abs(np.asarray(a, np.float64))) if absolute else (lambda a: np.asarray(a, np.float64))
    mat = (lambda m: np.abs(m)) if absolute else (lambda m: m)
    V = np.zeros((36, d.Ktot, d.NTp), dtype)
    untouched = np.zeros((36, d.Ktot, d.NTp), bool)
    rows = [[fold(4 * ty - 1 + i, H, pad) for i in range(6)] for ty in range(d.th)]
    cols = [[fold(4 * tx - 1 + i, W, pad) for i in range(6)] for tx in range(d.tw)]
    if up1 == 2:
        lrows = [[fold_low(2 * ty - 1 + i, H // 2, pad) for i in range(4)] for ty in range(d.th)]
        lcols = [[fold_low(2 * tx - 1 + i, W // 2, pad) for i in range(4)] for tx in range(d.tw)]
        V[list(LONG), :C1, :d.NT] = _transform(mat(BT_UP), _patches(prep(x1), lrows, lcols), dtype)
        untouched[list(SHORT), :d.C1p] = True
    else:
        V[:, :C1, :d.NT] = _transform(mat(BT), _patches(prep(x1), rows, cols), dtype)
    if C2:
        V[:, d.C1p:d.C1p + C2, :d.NT] = _transform(mat(BT), _patches(prep(x2), rows, cols), dtype)
    return V, untouched


def product(U, V, up1, C1p, untouched=None, dtype=np.float64):
    """M[p][co][tile] = sum_c U[p][c][co] V[p][c][tile] over the kernel's reduction range of position p: every channel, or
    c >= C1p at the 11 short positions of a split layer.  U, V channel-major; untouched entries of V count as 0."""
    U, V = np.asarray(U, dtype), np.asarray(V, dtype)
    if untouched is not None:
        V = np.where(untouched, dtype(0), V)
    M = np.zeros((36, U.shape[2], V.shape[2]), dtype)
    for p in range(36):
        k = kbeg(p, up1, C1p)
        if k < U.shape[1]:
            M[p] = U[p, k:].T @ V[p, k:]
    return M


def output_image(M, bias, B, H, W, Cout, act="none", slope=0.0, dtype=np.float64):
    """y = act(A^T M A + bias) [B, Cout, H, W] from M [36][Coutp][NTp], the row pass rounded to dtype before the column pass"""
    d = dims(B, H, W, 1, 0, Cout)
    A = AT.astype(dtype)
    m = np.asarray(M, dtype)[:, :Cout, :d.NT].reshape(6, 6, Cout, B, d.th, d.tw)
    t = np.einsum("ia,adobyx->idobyx", A, m).astype(dtype)
    y = np.einsum("idobyx,jd->boyixj", t, A).astype(dtype).reshape(B, Cout, 4 * d.th, 4 * d.tw)[:, :, :H, :W]
    if bias is not None:
        y = y + np.asarray(bias, dtype)[None, :, None, None]
    return activate(y, act, slope).astype(dtype)


def images(x1, w, bias=None, x2=None, up1=1, pad="reflect"):
    """The float64 statements of the three images of one launch, in the kernels' layouts: U [36][Ktot/4][Coutp][4],
    V [36][Ktot/4][NTp][4], M [36][Coutp][NTp], and the boolean mask (V's layout) of the V entries the contract leaves untouched.
    (bias enters after M: it is accepted so that a case's operands pass whole, and ignored.)"""
    x1 = np.asarray(x1)
    Uc = weight_image(w, x1.shape[1], up1)
    Vc, un = input_image(x1, x2, up1, pad)
    M = product(Uc, Vc, up1, round_up(x1.shape[1], KC), un)
    return pack4(Uc), pack4(Vc), M, pack4(un)


def three_pass_f32(x1, w, bias=None, x2=None, up1=1, pad="reflect", act="none", slope=0.0):
    """The same three passes with every intermediate rounded to float32: weights float32(G g G^T), then input transform, product
    and output transform in float32.  The oracle32 of the end-to-end comparison: unlike a float32 direct convolution it carries
    the algorithm's own amplification."""
    x1 = np.asarray(x1, np.float32)
    B, C1 = x1.shape[:2]
    H, W = x1.shape[2] * up1, x1.shape[3] * up1
    U = weight_image(w, C1, up1).astype(np.float32)
    V, un = input_image(x1, None if x2 is None else np.asarray(x2, np.float32), up1, pad, np.float32)
    M = product(U, V, up1, round_up(C1, KC), un, np.float32)
    return output_image(M, bias, B, H, W, np.asarray(w).shape[0], act, slope, np.float32)
