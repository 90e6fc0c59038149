"""The wavelet heads' forward restated on oracle.decoder_ref, generic in the dtype of its operands (the float64 oracle is the same
function on .double() operands, the float32 one measures the reference's own rounding), and the case generator of
test_gpu_head_fwd.py: operands from seeded torch.Generators, masks, and the host rules of the head launches re-derived in Python
(head_plan, the `wide` rule, the C = 256 cost rule), so that a table shape that no longer reaches its form fails the test."""
import os
import zlib

import torch

from oracle import decoder_ref as R

SLOPE = 0.1
NUM_CU = 256                       # kNumCU (wmd_internal.h)
HT_H, HT_W, H_CK = 16, 32, 8       # head3x3_kernel's tile and channel chunk (wmd_head.hip)
HL_TH, HL_TW = 4, 40               # head_level_kernel's tile (wmd_head_level.hip)
CHAIN_PXB = {64: 128, 128: 64}     # pixels of a head_chain_kernel block (C = 256: 32 or 48, chain_pg256)


def gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()))


def randn(g, *shape):
    return torch.randn(shape, generator=g)


# ---- operands -----------------------------------------------------------------------------------------------------------------
def head_params(g, C, cout=3, cin=None):
    """(w1 [C,cin,1,1], b1 [C], w3 [cout,C,3,3], b3 [cout]) of one head: pre-activations of unit scale for unit-scale inputs"""
    cin = C if cin is None else cin
    return [randn(g, C, cin, 1, 1) / cin ** 0.5, randn(g, C) * 0.3, randn(g, cout, C, 3, 3) / (1.5 * C ** 0.5), randn(g, cout) * 0.3]


def level_case(tag, B, C, H, W, with_ll=False):
    """x, yl and the heads (+, -, and the low-pass head C -> C/4 -> 1 when asked for) of one level"""
    g = gen(tag)
    c = dict(B=B, C=C, H=H, W=W, x=randn(g, B, C, H, W), yl=randn(g, B, 1, H, W) * 0.6 + 0.5, hp=head_params(g, C), hn=head_params(g, C))
    if with_ll:
        c["hl"] = head_params(g, C // 4, 1, C)
    return c


def tile_mask(tag, B, H, W, th, tw):
    """uint8 [B,H,W]: the th x tw tiles in turn empty, partly set (30 %), one pixel -- at least one empty and one partly set tile
    whenever there are two tiles"""
    g = gen(tag)
    m = torch.zeros((B, H, W), dtype=torch.uint8)
    kinds, i = [], 0
    for b in range(B):
        for y0 in range(0, H, th):
            for x0 in range(0, W, tw):
                blk = m[b, y0:y0 + th, x0:x0 + tw]
                if i % 3 == 1:
                    blk.copy_((torch.rand(blk.shape, generator=g) < 0.3).to(torch.uint8))
                    blk[0, 0] = 1
                elif i % 3 == 2:
                    blk[-1, -1] = 1
                kinds.append((b, y0, x0, i % 3))
                i += 1
    return m, kinds


def run_mask(tag, B, plane, run):
    """uint8 [B,plane]: runs of `run` pixels in turn empty, one pixel, full -> (mask, bool [B,plane] of the pixels in listed runs)"""
    m = torch.zeros((B, plane), dtype=torch.uint8)
    listed = torch.zeros((B, plane), dtype=torch.bool)
    i = 1
    for b in range(B):
        for p0 in range(0, plane, run):
            if i % 3 == 1:
                m[b, min(p0 + run, plane) - 1] = 1
            elif i % 3 == 2:
                m[b, p0:p0 + run] = 1
            if i % 3:
                listed[b, p0:p0 + run] = True
            i += 1
    return m, listed


def dilate3(m):
    """the 3x3 dilation of a [B,H,W] mask (zero beyond the border)"""
    return torch.nn.functional.max_pool2d(m.float().unsqueeze(1), 3, 1, 1).squeeze(1) > 0


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def cast(v, dt):
    if isinstance(v, (list, tuple)):
        return [cast(e, dt) for e in v]
    return None if v is None else v.to(dt)


def mid_of(x, head, bias1=True):
    return R.leaky(R.conv1x1(x, head[0], head[1] if bias1 else None), SLOPE)


def tap_partials(mid, w3):
    """[B, cout*9, H, W]: plane co*9 + ky*3 + kx = sum_c w3[co,c,ky,kx] * mid[c]"""
    co, c = w3.shape[:2]
    return R.conv1x1(mid, w3.permute(0, 2, 3, 1).reshape(co * 9, c, 1, 1), None)


def gather9(tp, pad):
    """nine-tap shift-sum of [B, n*9, H, W] tap-partial planes -> [B, n, H, W]: plane co*9 + ky*3 + kx read at (y + ky - 1, x + kx - 1)"""
    B, n9, H, W = tp.shape
    p = R.pad1(tp, pad).view(B, n9 // 9, 3, 3, H + 2, W + 2)
    return sum(p[:, :, ky, kx, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3))


def complete(t, b3p, b3n, scale, pad, yl=None, ll=False, b3l=None, scale_ll=1.0, mask=None, disp_scale=1.0, clamp01=False):
    """what the shift-sum does with t [B,54|81,H,W] -> dict(sig_p, sig_n, yh [B,3,H,W], and with a low-pass input or head: sig_ll,
    yl [B,1,H,W], out, disp)"""
    bias = lambda b: 0 if b is None else b.view(1, -1, 1, 1)
    o = {"sig_p": torch.sigmoid(gather9(t[:, :27], pad) + bias(b3p)), "sig_n": torch.sigmoid(gather9(t[:, 27:54], pad) + bias(b3n))}
    o["yh"] = scale * o["sig_p"] - scale * o["sig_n"]
    if mask is not None:
        o["yh"] = torch.where(mask.unsqueeze(1) != 0, o["yh"], torch.zeros_like(o["yh"]))
    if ll:     # the low-pass head completed from planes 54..62; it is the synthesis input
        o["sig_ll"] = torch.sigmoid(gather9(t[:, 54:63], pad) + bias(b3l))
        yl = o["yl"] = scale_ll * o["sig_ll"]
    if yl is not None:
        o["out"] = R.haar_idwt(yl, o["yh"].unsqueeze(1))
        o["pre_disp"] = o["out"] * disp_scale
        o["disp"] = o["pre_disp"].clamp(0, 1) if clamp01 else o["pre_disp"]
    return o


def first_stage(c, dt, bias1=True, with_ll=False):
    """mid_p, mid_n (, mid_ll) and t [B,54|81,H,W] (planes 63..80 of an 81-plane t are NaN: never written) in dtype dt"""
    x, hp, hn = cast(c["x"], dt), cast(c["hp"], dt), cast(c["hn"], dt)
    o = {"mid_p": mid_of(x, hp, bias1), "mid_n": mid_of(x, hn, bias1)}
    planes = [tap_partials(o["mid_p"], hp[2]), tap_partials(o["mid_n"], hn[2])]
    if with_ll:
        hl = cast(c["hl"], dt)
        o["mid_ll"] = mid_of(x, hl)
        planes += [tap_partials(o["mid_ll"], hl[2]), torch.full((c["B"], 18, c["H"], c["W"]), float("nan"), dtype=dt)]
    o["t"] = torch.cat(planes, 1)
    return o


def level(c, dt, scale, pad="reflect", bias1=True, b3=True, with_yl=True, mask=None, disp_scale=1.0, clamp01=False):
    """the whole level: first_stage + complete"""
    o = first_stage(c, dt, bias1)
    hp, hn = cast(c["hp"], dt), cast(c["hn"], dt)
    o.update(complete(o["t"], hp[3] if b3 else None, hn[3] if b3 else None, scale, pad, cast(c["yl"], dt) if with_yl else None,
                      mask=mask, disp_scale=disp_scale, clamp01=clamp01))
    return o


def head3x3(xp, wp, bp, xn, wn, bn, pad, mode, scale):
    """wmd_head_args: -> dict(y, sig_p, sig_n)"""
    o = {}
    hp = R.conv3x3(xp, wp, bp, pad)
    if mode == 0:
        o["y"] = scale * hp
        return o
    o["sig_p"] = torch.sigmoid(hp)
    if mode == 1:
        o["y"] = scale * o["sig_p"]
        return o
    o["sig_n"] = torch.sigmoid(R.conv3x3(xn, wn, bn, pad))
    o["y"] = scale * o["sig_p"] - scale * o["sig_n"]
    return o


def clamp_health(pre_disp64, what):
    """a disp compared under clamp01 must exercise both the clamp and the pass-through: >= 1 % of the pixels each"""
    outside = float(((pre_disp64 < 0) | (pre_disp64 > 1)).double().mean())
    assert outside >= 0.01 and 1.0 - outside >= 0.01, "%s: %.1f %% of out * disp_scale outside [0, 1]" % (what, 100 * outside)


# ---- the host rules, re-derived ------------------------------------------------------------------------------------------------
def _switch(name):
    v = os.environ.get(name)
    return None if v is None else int(v)


def head3x3_plan(B, C, H, W, workspace=True):
    """head_plan + the `wide` rule of wmd_head3x3_fwd -> (csplit, channels per slice, NG)"""
    tiles = B * ((W + HT_W - 1) // HT_W) * ((H + HT_H - 1) // HT_H)
    cs = min((3 * NUM_CU + tiles - 1) // tiles, max(1, C // 16))
    if _switch("WMD_HEAD_CSPLIT") is not None:
        cs = max(1, _switch("WMD_HEAD_CSPLIT"))
    cs = max(1, min(cs, (C + H_CK - 1) // H_CK))
    per = ((((C + cs - 1) // cs) + H_CK - 1) // H_CK) * H_CK
    cs = (C + per - 1) // per
    if not workspace:
        cs, per = 1, ((C + H_CK - 1) // H_CK) * H_CK
    ng = 4 if tiles * cs < 2 * NUM_CU else 2
    if _switch("WMD_HEAD_NG") is not None:
        ng = 4 if _switch("WMD_HEAD_NG") == 4 else 2
    return cs, per, ng


def chain_pixels(B, C, plane):
    """pixels per head_chain_kernel block; C = 256: the cost rule of head_chain_launch (48 when that saves a round of blocks)"""
    if C != 256:
        return CHAIN_PXB[C]
    force = _switch("WMD_HEAD_CHAIN_PG256") or 0
    b32, b48 = B * ((plane + 31) // 32) * 2, B * ((plane + 47) // 48) * 2
    cost32, cost48 = ((b32 + NUM_CU - 1) // NUM_CU) * 2, ((b48 + NUM_CU - 1) // NUM_CU) * 3
    return 48 if force == 3 or (force == 0 and cost48 < cost32) else 32


def key_of(f):
    """order-preserving uint32 key of float32 values (wmd_head_shiftsum_args.range_keys), as int64"""
    bits = f.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return torch.where(bits >= 0x80000000, bits ^ 0xFFFFFFFF, bits | 0x80000000)
