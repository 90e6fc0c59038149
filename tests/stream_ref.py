"""Plain torch-CPU oracles of the streaming kernels (wmd_dwconv.hip, wmd_wavelet.hip, wmd_resample.hip and
flip_postprocess_kernel of wmd_eval.hip), each runnable in float32 and in float64 -- TEST INFRASTRUCTURE ONLY.

Nothing here imports the product.  Every function takes `dtype` last, casts its operands to it and computes in it; the float64
result is the reference, the float32 result measures what float32 arithmetic of the same operation costs.
Every backward takes its gate from a tensor the C entry point is given (`y`, `out`, `depth`), and the gates are evaluated on those
float32 values exactly as the kernels evaluate them, so no pixel is ambiguous between the two dtypes.
tests/test_stream_ref_oracle.py holds the float64 forms to torch autograd, oracle/decoder_ref.py, PyWavelets vectors and
oracle/eval_ref.py."""
import numpy as np
import torch
import torch.nn.functional as Fn

_PAD = {"zero": "constant", "reflect": "reflect", "replicate": "replicate"}
ACT_NONE, ACT_ELU, ACT_LEAKY, ACT_SIGMOID = 0, 1, 2, 3      # wmd_act of include/wmd.h, act_deriv of wmd_internal.h


def cast(v, dtype):
    return None if v is None else torch.as_tensor(v).to(dtype)


# ---- depthwise 3x3 + ReLU over [nearest-upsampled x1 | x2], padded by one ----------------------------------------------------------
def _virtual(x1, x2, up1):
    u = x1 if up1 == 1 else x1.repeat_interleave(up1, 2).repeat_interleave(up1, 3)
    return u if x2 is None else torch.cat([u, x2], 1)


def _padded(x1, x2, up1, pad):
    return Fn.pad(_virtual(x1, x2, up1), (1, 1, 1, 1), mode=_PAD[pad])


def dwconv_fwd(x1, x2, w, up1, pad, dtype):
    """x1 [B,C1,H/up1,W/up1], x2 [B,C2,H,W] or None, w [C,1,3,3] -> y [B,C,H,W] = relu(sum_t w[c,t] P[b,c,y+ky,x+kx])"""
    x1, x2, w = cast(x1, dtype), cast(x2, dtype), cast(w, dtype)
    P = _padded(x1, x2, up1, pad)
    B, C, Hp, Wp = P.shape
    H, W = Hp - 2, Wp - 2
    w = w.reshape(C, 3, 3)
    s = torch.zeros((B, C, H, W), dtype=dtype)
    for t in range(9):
        ky, kx = t // 3, t % 3
        s = s + w[:, ky, kx].view(1, C, 1, 1) * P[:, :, ky:ky + H, kx:kx + W]
    return torch.relu(s)


def _pad_source(n, pad):
    """source coordinate of padded coordinate 0 .. n+1 (-1: reads zero)"""
    src = []
    for g in range(-1, n + 1):
        if 0 <= g < n:
            src.append(g)
        elif pad == "zero":
            src.append(-1)
        elif pad == "replicate":
            src.append(0 if g < 0 else n - 1)
        else:
            src.append(-g if g < 0 else 2 * n - 2 - g)
    return src


def _unpad(gP, pad):
    """adjoint of the one-pixel padding: every padded position adds into its source"""
    B, C, Hp, Wp = gP.shape
    H, W = Hp - 2, Wp - 2
    sy, sx = _pad_source(H, pad), _pad_source(W, pad)
    rows = torch.zeros((B, C, H, Wp), dtype=gP.dtype)
    for Y, y in enumerate(sy):
        if y >= 0:
            rows[:, :, y] += gP[:, :, Y]
    out = torch.zeros((B, C, H, W), dtype=gP.dtype)
    for X, x in enumerate(sx):
        if x >= 0:
            out[:, :, :, x] += rows[:, :, :, X]
    return out


def dwconv_bwd(x1, x2, w, y, dy, up1, pad, dtype, dw_sequential=False):
    """-> (dx1, dx2 or None, dw [C,1,3,3]); dz = dy where the GIVEN y > 0.  dw_sequential: the B*H*W terms of every dw[c,t] are
    added one by one in `dtype` (numpy cumsum) instead of by torch.sum's blocked order."""
    gate = torch.as_tensor(y) > 0
    x1, x2, w, dy = cast(x1, dtype), cast(x2, dtype), cast(w, dtype), cast(dy, dtype)
    dz = torch.where(gate, dy, torch.zeros((), dtype=dtype))
    B, C, H, W = dz.shape
    C1 = x1.shape[1]
    w = w.reshape(C, 3, 3)
    P = _padded(x1, x2, up1, pad)
    gP = torch.zeros((B, C, H + 2, W + 2), dtype=dtype)
    dw = torch.zeros((C, 3, 3), dtype=dtype)
    for t in range(9):
        ky, kx = t // 3, t % 3
        gP[:, :, ky:ky + H, kx:kx + W] += w[:, ky, kx].view(1, C, 1, 1) * dz
        prod = (dz * P[:, :, ky:ky + H, kx:kx + W]).permute(1, 0, 2, 3).reshape(C, -1)
        if dw_sequential:
            dw[:, ky, kx] = torch.from_numpy(np.cumsum(prod.numpy(), axis=1, dtype=prod.numpy().dtype)[:, -1].copy())
        else:
            dw[:, ky, kx] = prod.sum(1)
    dv = _unpad(gP, pad)
    d1 = dv[:, :C1]
    if up1 != 1:
        d1 = d1.reshape(B, C1, H // up1, up1, W // up1, up1).sum((3, 5))
    return d1.contiguous(), (dv[:, C1:].contiguous() if x2 is not None else None), dw.view(C, 1, 3, 3)


# ---- Haar synthesis / analysis -----------------------------------------------------------------------------------------------------
def idwt(yl, yh, disp_scale, clamp01, dtype):
    """yl [N,h,w], yh [N,3,h,w] (LH, HL, HH) -> out [N,2h,2w], disp = out * disp_scale (clamped to [0,1] when clamp01)"""
    a, yh = cast(yl, dtype), cast(yh, dtype)
    b, c, d = yh[:, 0], yh[:, 1], yh[:, 2]
    N, h, w = a.shape
    out = torch.zeros((N, 2 * h, 2 * w), dtype=dtype)
    out[:, 0::2, 0::2] = (a + b + c + d) * 0.5
    out[:, 0::2, 1::2] = (a + b - c - d) * 0.5
    out[:, 1::2, 0::2] = (a - b + c - d) * 0.5
    out[:, 1::2, 1::2] = (a - b - c + d) * 0.5
    disp = out * float(np.float32(disp_scale))
    if clamp01:
        disp = disp.clamp(0, 1)
    return out, disp


def _analysis(g):
    tx, ty, ux, uy = g[:, 0::2, 0::2], g[:, 0::2, 1::2], g[:, 1::2, 0::2], g[:, 1::2, 1::2]
    yl = (tx + ty + ux + uy) * 0.5
    yh = torch.stack([(tx + ty - ux - uy) * 0.5, (tx - ty + ux - uy) * 0.5, (tx - ty - ux + uy) * 0.5], 1)
    return yl, yh


def clamp_gate(out, disp_scale):
    """[0 <= out * disp_scale <= 1] on float32(out) * float32(disp_scale), the product rounded to float32, both ends inclusive"""
    s = torch.as_tensor(out).to(torch.float32) * torch.tensor(float(disp_scale), dtype=torch.float32)
    return (s >= 0) & (s <= 1)


def idwt_bwd(d_out, d_disp, out, disp_scale, clamp01, dtype):
    """-> (d_yl [N,h,w], d_yh [N,3,h,w]) of g = d_out + d_disp * disp_scale * gate; either gradient may be None"""
    ref = d_out if d_out is not None else d_disp
    g = torch.zeros(tuple(ref.shape), dtype=dtype)
    if d_out is not None:
        g = g + cast(d_out, dtype)
    if d_disp is not None:
        dd = cast(d_disp, dtype)
        if clamp01:
            dd = torch.where(clamp_gate(out, disp_scale), dd, torch.zeros((), dtype=dtype))
        g = g + dd * float(np.float32(disp_scale))
    return _analysis(g)


def dwt(x, dtype):
    """x [N,2h,2w] -> (yl [N,h,w], yh [N,3,h,w])"""
    return _analysis(cast(x, dtype))


def dwt_reflect(x, dtype):
    """any H, W: an odd axis gets one reflected sample on the right / bottom (x[n] = x[n-2]) first"""
    x = cast(x, dtype)
    if x.shape[1] % 2:
        x = torch.cat([x, x[:, -2:-1]], 1)
    if x.shape[2] % 2:
        x = torch.cat([x, x[:, :, -2:-1]], 2)
    return _analysis(x)


def act_deriv(y, act, slope, dtype):
    """f'(x) in terms of the activation OUTPUT y; the kinks are decided on the given y"""
    yy = cast(y, dtype)
    one = torch.ones((), dtype=dtype)
    if act == ACT_ELU:
        return torch.where(yy > 0, one, yy + 1)
    if act == ACT_LEAKY:
        return torch.where(yy > 0, one, one * float(np.float32(slope)))
    if act == ACT_SIGMOID:
        return yy * (1 - yy)
    return torch.ones_like(yy)


def act_bwd(dy, y, act, slope, dtype):
    return cast(dy, dtype) * act_deriv(y, act, slope, dtype)


# ---- bilinear resize (+ disp_to_depth) ---------------------------------------------------------------------------------------------
def _axis(n_in, n_out, align_corners, dtype):
    """ATen's upsample_bilinear2d index rule along one axis -> (i0, i1, lambda) per output index"""
    o = torch.arange(n_out, dtype=dtype)
    if align_corners:
        scale = torch.tensor((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0, dtype=dtype)
        src = scale * o
    else:
        scale = torch.tensor(n_in, dtype=dtype) / torch.tensor(n_out, dtype=dtype)
        src = (scale * (o + 0.5) - 0.5).clamp(min=0)
    i0 = src.floor().long().clamp(max=n_in - 1)
    i1 = i0 + (i0 < n_in - 1).long()
    return i0, i1, src - i0.to(dtype)


def _disp_range(depth_range, dtype):
    lo, hi = depth_range        # (min_depth, max_depth) -> min_disp = 1 / max_depth, max_disp = 1 / min_depth
    return torch.tensor(1.0, dtype=dtype) / hi, torch.tensor(1.0, dtype=dtype) / lo


def bilinear(x, size, align_corners, depth_range, dtype):
    """x [N,h,w] -> (y [N,H,W], depth = 1 / (min_disp + (max_disp - min_disp) y) or None)"""
    x = cast(x, dtype)
    N, h, w = x.shape
    H, W = size
    y0, y1, ly = _axis(h, H, align_corners, dtype)
    x0, x1, lx = _axis(w, W, align_corners, dtype)
    ly, lx = ly.view(1, H, 1), lx.view(1, 1, W)
    top = (1 - lx) * x[:, y0][:, :, x0] + lx * x[:, y0][:, :, x1]
    bot = (1 - lx) * x[:, y1][:, :, x0] + lx * x[:, y1][:, :, x1]
    y = (1 - ly) * top + ly * bot
    if depth_range is None:
        return y, None
    lo, hi = _disp_range(depth_range, dtype)
    return y, 1 / (lo + (hi - lo) * y)


def bilinear_bwd(dy, ddepth, depth, in_size, align_corners, depth_range, dtype):
    """dy, ddepth [N,H,W] (either may be None), depth = the forward's depth (given) -> dx [N,h,w]: every output pixel scatters
    its gradient to its four sources with the forward's weights"""
    ref = dy if dy is not None else ddepth
    N, H, W = ref.shape
    h, w = in_size
    g = torch.zeros((N, H, W), dtype=dtype)
    if dy is not None:
        g = g + cast(dy, dtype)
    if ddepth is not None:
        lo, hi = _disp_range(depth_range, dtype)
        d = cast(depth, dtype)
        g = g - cast(ddepth, dtype) * (hi - lo) * d * d
    y0, y1, ly = _axis(h, H, align_corners, dtype)
    x0, x1, lx = _axis(w, W, align_corners, dtype)
    dx = torch.zeros((N, h * w), dtype=dtype)
    for yi, wy in ((y0, 1 - ly), (y1, ly)):
        for xi, wx in ((x0, 1 - lx), (x1, lx)):
            idx = (yi.view(H, 1) * w + xi.view(1, W)).reshape(-1)
            dx.index_add_(1, idx, (wy.view(1, H, 1) * wx.view(1, 1, W) * g).reshape(N, -1))
    return dx.view(N, h, w)


# ---- Monodepth flip post-processing ------------------------------------------------------------------------------------------------
def flip_postprocess(l, r, dtype):
    """l, r [B,h,w]; r is the prediction for the flipped image, NOT flipped back.  The linspace masks are float64 whatever `dtype`
    is, as in oracle/eval_ref.batch_post_process_disparity: `dtype` decides the mean and the result's rounding."""
    l, r = cast(l, dtype), cast(r, dtype).flip(-1)
    w = l.shape[-1]
    m = (0.5 * (l + r)).double()
    lin = torch.from_numpy(np.linspace(0, 1, w))
    lm = (1.0 - (20 * (lin - 0.05)).clamp(0, 1)).view(1, 1, w)
    rm = lm.flip(-1)
    return (rm * l.double() + lm * r.double() + (1.0 - lm - rm) * m).to(dtype)
