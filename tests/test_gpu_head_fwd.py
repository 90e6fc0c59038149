"""The wavelet heads' forward kernels (wmd_head.hip, wmd_head_level.hip, wmd_head_chain.hip, wmd_head_stream.hip and the FUSE forms
of conv_fwd_kernel) held against the float64 oracle, instantiation by instantiation.

The argument blocks are built directly (no ops.*_nograd wrapper allocates an output): every output is a view inside a NaN-filled
buffer with a guard band on each side, so a store outside an output shows in the bands and an element never written in the
output; planes the contract leaves alone must still be NaN.  wmd_head3x3_fwd gets exactly wmd_head3x3_workspace_floats(a) floats.
The launch profile names the kernels that ran, and the host rules that pick an instantiation are re-derived in head_ref.py, so a
table shape that stops reaching its form fails here.

Tolerances are measured, not chosen: for every compared tensor, on the same inputs,
    e_ref = max |oracle32 - oracle64| / max |oracle64|     the torch-CPU oracle in float32 against itself in float64
    e_hip = max |hip      - oracle64| / max |oracle64|
(yh: divided by `scale` instead, a difference of sigmoids cancels) and the assertion is e_hip <= F[kind] * e_ref + 4 * 2^-23.
No pixel is excluded: LeakyReLU, the clamp and the mask select are continuous or exact."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import head_ref as H
import pin_harness as P
from pin_harness import GUARD, NAN, Bufs, untouched, written

pytestmark = pytest.mark.gpu

# per tensor kind, the smallest power of two >= twice the largest e_hip / e_ref measured on the MI355X among the comparisons whose
# e_hip exceeds the floor (profiles/head_fwd_pins.md; the table and the kernel that set each entry are in DESIGN.md §4.6.1); 1 where
# no comparison of the kind exceeds the floor: the bound is then the reference's own error plus the floor
F = {"t": 4, "mid": 4, "sig": 8, "yh": 1, "yl": 1, "out": 1, "disp": 4, "head3x3_y": 8}
assert max(F.values()) <= 64
SWITCHES = ("WMD_HEAD_CHAIN", "WMD_HEAD_CHAIN_MULTI", "WMD_HEAD_CHAIN_PG256", "WMD_HEAD_STREAM", "WMD_HEAD_STREAM_TH", "WMD_HEAD_STREAM_MIN_PIXELS",
            "WMD_SHIFTSUM_CHAIN_SQUARE", "WMD_HEAD_CSPLIT", "WMD_HEAD_NG", "WMD_HEAD_BWD_FUSED")    # test_host_logic._HEAD_SWITCH_NAMES
DEFAULT_SWITCHES = not any(k in os.environ for k in SWITCHES)
UNSUPPORTED = -3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


# ---- harness ---------------------------------------------------------------------------------------------------------------------
class Checks(P.Checks):
    """pin_harness.Checks on this module's F table"""

    def __init__(self, case):
        super().__init__(case, F)


def ptr(v):
    return None if v is None else v.data_ptr()


def spare(v, dev, tail):
    """v on the device, contiguous, as the head of a larger allocation (`tail` more floats, zero)"""
    buf = torch.zeros((v.numel() + tail,), device=dev)
    buf[:v.numel()] = v.reshape(-1).to(dev)
    return buf[:v.numel()].view(v.shape)


def launch(fn, a, what, *extra):
    """-> (status, kernel names in launch order); every kernel of an accepted launch ran once, a refused one launched nothing"""
    from wavelet_monodepth_amd import _lib
    _lib.profile_begin()
    st = fn(a if isinstance(a, C.Array) else C.byref(a), *extra, torch.cuda.current_stream().cuda_stream)
    prof = _lib.profile_end()
    if st != 0:
        return st, [r["kernel"] for r in prof]
    assert all(r["calls"] == 1 for r in prof), "%s: %s" % (what, prof)
    return st, [r["kernel"] for r in prof]


def packs(dev, c, bias1=True):
    """the weight images of a level's heads on the device (ops.stacked_pack, ops._tap_partial_pack, ops._ll_chain_pack), memoised on the case"""
    from wavelet_monodepth_amd import ops
    if "dev" not in c:
        d = lambda v: [e.to(dev) for e in v]
        c["dev"] = dict(x=c["x"].to(dev).contiguous(), yl=c["yl"].to(dev).contiguous(), hp=d(c["hp"]), hn=d(c["hn"]), hl=d(c["hl"]) if "hl" in c else None)
        k = c["dev"]
        k["wp1"], k["bias1"] = ops.stacked_pack([k["hp"][0], k["hn"][0]], [k["hp"][1], k["hn"][1]])
        k["wp2"] = ops._tap_partial_pack(k["hp"][2], k["hn"][2])
        if k["hl"] is not None:
            k["ll_wp1"], k["ll_wp2"] = ops._ll_chain_pack(k["hl"][0], k["hl"][2])
        torch.cuda.synchronize()
    return c["dev"]


_ORACLES = {}


def oracle(key, fn):
    """(float32, float64) oracle results, computed once per key and left unchanged"""
    if key not in _ORACLES:
        _ORACLES[key] = (fn(torch.float32), fn(torch.float64))
    return _ORACLES[key]


# ---- A. wmd_head3x3_fwd: head3x3_kernel<CO,NG> + head_finalize_kernel --------------------------------------------------------------
A_SHAPES = {   # form -> (B, C, H, W, channel split, NG) under head_plan and the `wide` rule (tiles of 16 x 32, 256 CUs)
    "ng4_2x2": (1, 7, 2, 2, False, 4),
    "ng4_12x40": (2, 20, 12, 40, False, 4),
    "ng4_split_ragged": (1, 40, 9, 35, True, 4),        # slices of 24 + 16 channels
    "ng2_unsplit": (64, 8, 128, 2, False, 2),           # 512 tiles
    "ng2_split": (16, 128, 64, 2, True, 2),             # 64 tiles x 8 slices
}
A_MODE_PAD = [(m, p) for m in (0, 1, 2) for p in ("zero", "reflect", "replicate")]


def head3x3_variant(dev, form, i, chk, workspace="exact"):
    """variant i of a shape: (mode, pad) = A_MODE_PAD[i], Cout = i % 4 + 1, bias NULL for i % 3 == 1, sig_* written for even i,
    xp / xn channel slices of one wider tensor for odd i"""
    from wavelet_monodepth_amd import _lib
    l = _lib.lib()
    B, Cc, Hh, W, split, ng = A_SHAPES[form]
    (mode, pad), cout, bias, sig, sliced = A_MODE_PAD[i], i % 4 + 1, i % 3 != 1, i % 2 == 0, i % 2 == 1
    what = "%s mode %d %s Cout %d%s%s%s ws=%s" % (form, mode, pad, cout, "" if bias else " no-bias", " sig" if sig else "", " sliced" if sliced else "", workspace)
    g = H.gen("A%s%d" % (form, i))
    Ct = 2 * Cc + 12
    xw = H.randn(g, B, Ct, Hh, W)
    xp, xn = xw[:, 1:1 + Cc], xw[:, Cc + 2:2 * Cc + 2]
    wp, wn = (H.randn(g, cout, Cc, 3, 3) / (1.5 * Cc ** 0.5) for _ in range(2))
    bp, bn = (H.randn(g, cout) * 0.3 if bias else None for _ in range(2))
    scale = 2.0
    o32, o64 = oracle(("A", form, i), lambda dt: H.head3x3(*H.cast([xp, wp, bp, xn, wn, bn], dt), pad, mode, scale))
    plane = Hh * W
    if sliced:
        xd = xw.to(dev).contiguous()
        xp_ptr, xn_ptr, bstride = xd.data_ptr() + 4 * plane, xd.data_ptr() + 4 * (Cc + 2) * plane, Ct * plane
    else:   # (a spare tail behind every operand: a kernel that walks past the last channel reads zeros of this test, nothing else)
        xpd, xnd = spare(xp, dev, 16 * plane), spare(xn, dev, 16 * plane)
        xp_ptr, xn_ptr, bstride = xpd.data_ptr(), xnd.data_ptr(), 0
    wpd, wnd = spare(wp, dev, 16 * 9), spare(wn, dev, 16 * 9)
    bpd, bnd = (None if b is None else b.to(dev) for b in (bp, bn))
    bufs = Bufs(dev)
    y = bufs.new("y", B, cout, Hh, W)
    sp = bufs.new("sig_p", B, cout, Hh, W) if sig else None
    sn = bufs.new("sig_n", B, cout, Hh, W) if sig else None
    a = _lib.HeadArgs(B=B, H=Hh, W=W, C=Cc, Cout=cout, pad_mode=_lib.PAD[pad], mode=mode, scale=scale, xp=xp_ptr, wgt_p=ptr(wpd), bias_p=ptr(bpd),
                      xn=xn_ptr if mode == 2 else None, wgt_n=ptr(wnd) if mode == 2 else None, bias_n=ptr(bnd) if mode == 2 else None, y=ptr(y),
                      sig_p=ptr(sp), sig_n=ptr(sn), xp_bstride=bstride, xn_bstride=bstride, workspace=None, workspace_floats=0)
    n = l.wmd_head3x3_workspace_floats(C.byref(a))
    cs, per, _ng = H.head3x3_plan(B, Cc, Hh, W)
    assert n == (cs * B * 2 * cout * plane if cs > 1 else 0), "%s: %d workspace floats for %d slices" % (what, n, cs)
    if DEFAULT_SWITCHES:
        assert (n > 0) == split and _ng == ng, "%s: the shape no longer reaches its form (workspace %d, NG %d)" % (what, n, _ng)
        if form == "ng4_split_ragged":
            assert (cs, per) == (2, 24), (cs, per)
    ws = None
    if workspace != "null" and n > 0:
        have = n - 1 if workspace == "short" else n
        ws = torch.full((have + max(n, GUARD),), NAN, device=dev)
        a.workspace, a.workspace_floats = ws.data_ptr(), have
    st, kernels = launch(l.wmd_head3x3_fwd, a, what)
    assert st == 0, "%s: status %d" % (what, st)
    splits = n > 0 and workspace == "exact"
    assert kernels == ["head3x3_kernel"], "%s: %s" % (what, kernels)     # (one profiler scope covers the kernel and its finalize pass)
    bufs.bands(what)
    written(y, what + ": y")
    if ws is not None:
        untouched(ws[a.workspace_floats:], what + ": past the workspace")
        if splits:      # [slice][b][side][co][H*W]: the - side holds sums in mode 2 only
            part = ws[:n].view(cs, B, 2, cout, plane)
            written(part[:, :, 0], what + ": the slices' partial sums")
            (written if mode == 2 else untouched)(part[:, :, 1], what + ": the - side of the slices' partial sums")
        else:
            untouched(ws, what + ": an unsplit launch's workspace")
    chk.add("head3x3_y", what, y, o32["y"], o64["y"])
    if sig and mode >= 1:
        written(sp, what + ": sig_p")
        chk.add("sig", what + " sig_p", sp, o32["sig_p"], o64["sig_p"])
    elif sp is not None:
        untouched(sp, what + ": sig_p")
    if sig and mode == 2:
        written(sn, what + ": sig_n")
        chk.add("sig", what + " sig_n", sn, o32["sig_n"], o64["sig_n"])
    elif sn is not None:
        untouched(sn, what + ": sig_n")


def run_head3x3(dev, form):
    chk = Checks("A " + form)
    for i in range(len(A_MODE_PAD)):
        head3x3_variant(dev, form, i, chk)
    if A_SHAPES[form][4]:     # a NULL workspace and one a float too small: the launch runs unsplit and still meets the oracle
        for i, wsp in ((8, "null"), (5, "short"), (2, "null"), (7, "short")):
            head3x3_variant(dev, form, i, chk, wsp)
    chk.done()


@pytest.mark.parametrize("form", list(A_SHAPES))
def test_head3x3_every_form_vs_oracle(dev, form):
    """Every (mode, pad) pair, every Cout, bias NULL, sig_* outputs and channel-slice operands on each of the five forms: NG = 4 and 2,
    unsplit and split (a ragged last slice among them), and the unsplit fall-back of a missing or short workspace."""
    run_head3x3(dev, form)


# ---- B. wmd_head_level_fwd: head_level_kernel<32,4> and head_stream_kernel ------------------------------------------------------
B_SHAPES = [(2, 2, 2), (2, 5, 7), (2, 10, 84), (1, 2060, 2)]     # (1, 2060, 2): 515 tiles of 4 x 40, the persistent loop wraps, 515 % 8 = 3
_LEVELS = {}


def level_case(B, Cc, Hh, W, with_ll=False):
    key = (B, Cc, Hh, W, with_ll)
    if key not in _LEVELS:
        _LEVELS[key] = H.level_case("L%dx%dx%dx%d" % (B, Cc, Hh, W), B, Cc, Hh, W, with_ll)
    return _LEVELS[key]


def level_launch(dev, c, chk, tag, kernel, pad="reflect", mask=None, ones=False, with_yl=True, disp=True, clamp01=True, train=False, bias1=True,
                 mask_kinds=None):
    """one wmd_head_level_fwd launch against the oracle; mask: uint8 [B,H,W] (ones: an all-ones mask, the oracle is the unmasked one);
    train: mid_out at non-zero offsets inside a wider tensor + sig_p / sig_n"""
    from wavelet_monodepth_amd import _lib
    l = _lib.lib()
    B, Cc, Hh, W = c["B"], c["C"], c["H"], c["W"]
    what = "%dx%dx%d %s %s" % (B, Hh, W, pad, tag)
    scale, disp_scale = 2.0, 1.0
    k = packs(dev, c)
    m = torch.ones((B, Hh, W), dtype=torch.uint8) if ones else mask
    o32, o64 = oracle(("B", B, Hh, W, pad, tag), lambda dt: H.level(c, dt, scale, pad, bias1, True, with_yl, mask, disp_scale, clamp01))
    if with_yl and disp and clamp01:
        H.clamp_health(o64["pre_disp"], what)
    bufs = Bufs(dev)
    yh = bufs.new("yh", B, 3, Hh, W)
    out = bufs.new("out", B, 1, 2 * Hh, 2 * W) if with_yl else None
    dsp = bufs.new("disp", B, 1, 2 * Hh, 2 * W) if with_yl and disp else None
    a = _lib.HeadLevelArgs(B=B, H=Hh, W=W, C=Cc, pad_mode=_lib.PAD[pad], slope=H.SLOPE, scale=scale, x=ptr(k["x"]), wp1=ptr(k["wp1"]),
                           bias1=ptr(k["bias1"]) if bias1 else None, wp2=ptr(k["wp2"]), bias_p=ptr(k["hp"][3]), bias_n=ptr(k["hn"][3]), yh=ptr(yh),
                           yl=ptr(k["yl"]) if with_yl else None, out=ptr(out), disp=ptr(dsp), disp_scale=disp_scale, clamp01=int(clamp01),
                           yh_mask=None)
    md = m.to(dev) if m is not None else None
    a.yh_mask = ptr(md)
    mid = sp = sn = None
    if train:
        ct, off_p, off_n = 2 * Cc + 7, 3, Cc + 5
        mid, sp, sn = bufs.new("mid_out", B, ct, Hh, W), bufs.new("sig_p", B, 3, Hh, W), bufs.new("sig_n", B, 3, Hh, W)
        a.mid_out, a.mid_ct, a.mid_off_p, a.mid_off_n, a.sig_p, a.sig_n = ptr(mid), ct, off_p, off_n, ptr(sp), ptr(sn)
    st, kernels = launch(l.wmd_head_level_fwd, a, what)
    assert st == 0, "%s: status %d" % (what, st)
    assert kernels == [kernel], "%s: the profile shows %s, expected %s" % (what, kernels, kernel)
    bufs.bands(what)
    for name, v in (("yh", yh), ("out", out), ("disp", dsp), ("sig_p", sp), ("sig_n", sn)):
        if v is not None:
            written(v, "%s: %s" % (what, name))
    chk.add("yh", what, yh, o32["yh"], o64["yh"], denom=scale)
    if with_yl:
        chk.add("out", what, out, o32["out"], o64["out"])
        if disp:
            chk.add("disp", what, dsp, o32["disp"], o64["disp"])
    if train:
        written(mid[:, off_p:off_p + Cc], what + ": mid +")
        written(mid[:, off_n:off_n + Cc], what + ": mid -")
        for lo, hi in ((0, off_p), (off_p + Cc, off_n), (off_n + Cc, ct)):
            untouched(mid[:, lo:hi], "%s: mid_out channels %d..%d" % (what, lo, hi - 1))
        chk.add("mid", what + " +", mid[:, off_p:off_p + Cc], o32["mid_p"], o64["mid_p"])
        chk.add("mid", what + " -", mid[:, off_n:off_n + Cc], o32["mid_n"], o64["mid_n"])
        chk.add("sig", what + " sig_p", sp, o32["sig_p"], o64["sig_p"])
        chk.add("sig", what + " sig_n", sn, o32["sig_n"], o64["sig_n"])
    if mask_kinds is not None:    # a tile without a mask pixel: yh = 0 exactly, out = the four copies of yl / 2 exactly
        empty = 0
        for b, y0, x0, kind in mask_kinds:
            if kind != 0:
                continue
            empty += 1
            ys, xs = slice(y0, y0 + H.HL_TH), slice(x0, x0 + H.HL_TW)
            assert bool((yh[b, :, ys, xs] == 0).all()), "%s: yh of the empty tile at (%d, %d, %d)" % (what, b, y0, x0)
            if with_yl:
                half = (k["yl"][b, 0, ys, xs] * 0.5).repeat_interleave(2, 0).repeat_interleave(2, 1)
                got = out[b, 0, 2 * y0:2 * (y0 + H.HL_TH), 2 * x0:2 * (x0 + H.HL_TW)]
                assert torch.equal(got, half), "%s: out of the empty tile at (%d, %d, %d) is not yl / 2" % (what, b, y0, x0)
        assert empty > 0, what
    return yh, out, dsp


@pytest.mark.parametrize("shape", B_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_head_level_kernel_vs_oracle(dev, shape):
    """head_level_kernel<32,4> through each of its three doors -- a yh_mask (all ones == the unmasked oracle; whole tiles empty and
    others partly set: yh == 0 and out == yl / 2 exactly there), the training outputs (mid at non-zero offsets of a wider tensor,
    sig_*), zero / replicate padding -- with yl NULL, out without disp, clamp01 on and off, bias1 NULL."""
    B, Hh, W = shape
    c = level_case(B, 32, Hh, W)
    chk = Checks("B level %dx%dx%d" % shape)
    K = "head_level_kernel"
    m, kinds = H.tile_mask("M%dx%dx%d" % shape, B, Hh, W, H.HL_TH, H.HL_TW)
    level_launch(dev, c, chk, "mask=ones", K, ones=True)
    level_launch(dev, c, chk, "mask=tiles out", K, mask=m, mask_kinds=kinds, disp=False)
    level_launch(dev, c, chk, "mask=tiles disp", K, mask=m, mask_kinds=kinds, clamp01=False)
    level_launch(dev, c, chk, "mask=tiles yh-only", K, mask=m, mask_kinds=kinds, with_yl=False)
    level_launch(dev, c, chk, "mask=tiles zero-pad", K, pad="zero", mask=m, mask_kinds=kinds)
    level_launch(dev, c, chk, "train", K, train=True, clamp01=False)
    level_launch(dev, c, chk, "train no-bias1 yh-only", K, train=True, bias1=False, with_yl=False)
    for pad in ("zero", "replicate"):
        level_launch(dev, c, chk, "plain", K, pad=pad)
        level_launch(dev, c, chk, "train", K, pad=pad, train=True, disp=False)
    level_launch(dev, c, chk, "plain no-bias1", K, pad="zero", bias1=False)
    chk.done()


def run_level_plain(dev, shape, kernel):
    B, Hh, W = shape
    c = level_case(B, 32, Hh, W)
    chk = Checks("B %s %dx%dx%d" % ((kernel.split("_")[1],) + tuple(shape)))
    yh, _, _ = level_launch(dev, c, chk, "plain", kernel)
    level_launch(dev, c, chk, "plain out no-clamp", kernel, clamp01=False)
    level_launch(dev, c, chk, "plain no-bias1 out", kernel, bias1=False, disp=False)
    yh2, _, _ = level_launch(dev, c, chk, "plain yh-only", kernel, with_yl=False)
    assert torch.equal(yh, yh2), "yh depends on the synthesis outputs"
    chk.done()


@pytest.mark.parametrize("shape", B_SHAPES + [(520, 2, 2)], ids=lambda s: "x".join(map(str, s)))
def test_head_stream_kernel_vs_oracle(dev, shape):
    """head_stream_kernel takes every plain C = 32 reflect launch (WMD_HEAD_STREAM_MIN_PIXELS defaults to 0): the same shapes, and
    520 frames of 2 x 2 -- more units than the grid cap of head_stream_launch (2 * 256 blocks at most), so the persistent loop wraps."""
    if os.environ.get("WMD_HEAD_STREAM", "1") == "0" or "WMD_HEAD_STREAM_MIN_PIXELS" in os.environ:
        pytest.skip("the streaming kernel is switched off")
    run_level_plain(dev, shape, "head_stream_kernel")


# ---- C. wmd_head_fused_fwd: head_chain_kernel and the FUSE forms of conv_fwd_kernel ------------------------------------------------
C_SHAPES = {   # form -> (C, B, H, W, pixels of a block)
    "c64_9x28": (64, 2, 9, 28, 128),             # 128 + 124 pixels
    "c128_6x20": (128, 2, 6, 20, 64),            # 64 + 56
    "c256_pg2_6x10": (256, 2, 6, 10, 32),        # 32 + 28
    "c256_pg2_12x40": (256, 1, 12, 40, 32),      # exact
    "c256_pg3_8x12": (256, 43, 8, 12, 48),       # cost48 = 3 < cost32 = 4; exact 48s
    "c256_pg3_10x10": (256, 33, 10, 10, 48),     # 48 + 48 + 4
}
CHAIN, FUSE, FUSE_LL = "head_chain_kernel", "conv_fwd_kernel<fused head>", "conv_fwd_kernel<fused LL head>"


def fused_launch(dev, c, chk, tag, kernels_want, bias1=True, ll=False, mid=False, rmask=None, listed=None, chain=0, planes=None, status=0):
    """one wmd_head_fused_fwd launch: the t planes themselves against the float64 tap partials (mid_out too).  rmask / listed: a
    run_mask and the pixels of the runs it lists (the others stay NaN in planes 0..53); chain = 1: the low-pass chain alone"""
    from wavelet_monodepth_amd import _lib
    l = _lib.lib()
    B, Cc, Hh, W = c["B"], c["C"], c["H"], c["W"]
    what = "C%d %dx%dx%d %s" % (Cc, B, Hh, W, tag)
    k = packs(dev, c)
    planes = planes or (81 if (ll or chain) else 54)
    o32, o64 = oracle(("C", Cc, B, Hh, W, bias1, "hl" in c), lambda dt: H.first_stage(c, dt, bias1, "hl" in c))
    bufs = Bufs(dev)
    t = bufs.new("t", B, planes, Hh, W)
    a = _lib.HeadFusedArgs(B=B, H=Hh, W=W, C=Cc, slope=H.SLOPE, x=ptr(k["x"]), wp1=ptr(k["wp1"]), bias1=ptr(k["bias1"]) if bias1 else None,
                           wp2=ptr(k["wp2"]), t=ptr(t), chain=chain, t_planes=planes)
    if chain:
        a.wp1, a.bias1, a.wp2 = ptr(k["ll_wp1"]), ptr(k["hl"][1]), ptr(k["ll_wp2"])
    rm = None
    if rmask is not None:
        rm = rmask.to(dev)
        a.run_mask = ptr(rm)
    if ll:
        a.ll_wp1, a.ll_bias1, a.ll_wp2 = ptr(k["ll_wp1"]), ptr(k["hl"][1]), ptr(k["ll_wp2"])
    mo = None
    if mid:
        ct, offs = 2 * Cc + Cc // 4 + 9, (Cc // 4 + 5, Cc + Cc // 4 + 7, 2)
        mo = bufs.new("mid_out", B, ct, Hh, W)
        a.mid_out, a.mid_ct, a.mid_off_p, a.mid_off_n, a.mid_off_ll = ptr(mo), ct, offs[0], offs[1], offs[2]
    st, kernels = launch(l.wmd_head_fused_fwd, a, what)
    assert st == status, "%s: status %d" % (what, st)
    assert kernels == kernels_want, "%s: the profile shows %s, expected %s" % (what, kernels, kernels_want)
    if status:
        untouched(t, what + ": t of a refused launch")
        return
    bufs.bands(what)
    keep = None if listed is None else listed.view(B, 1, Hh, W)
    if chain:
        untouched(t[:, :54], what + ": planes 0..53")
    elif keep is None:
        written(t[:, :54], what + ": planes 0..53")
        chk.add("t", what, t[:, :54], o32["t"][:, :54], o64["t"][:, :54])
    else:
        kd = keep.to(dev).expand(B, 54, Hh, W)
        written(t[:, :54][kd], what + ": the listed runs")
        untouched(t[:, :54][~kd], what + ": the skipped runs")
        chk.add("t", what, t[:, :54], o32["t"][:, :54], o64["t"][:, :54], keep=keep)
    if planes == 81:
        untouched(t[:, 63:], what + ": planes 63..80")
        if ll or chain:
            written(t[:, 54:63], what + ": planes 54..62")
            chk.add("t", what + " LL", t[:, 54:63], o32["t"][:, 54:63], o64["t"][:, 54:63])
        else:
            untouched(t[:, 54:63], what + ": planes 54..62")
    if mid:
        spans = [(offs[0], Cc, "mid_p"), (offs[1], Cc, "mid_n")] + ([(offs[2], Cc // 4, "mid_ll")] if ll else [])
        own = torch.zeros(ct, dtype=torch.bool)
        for off, n, name in spans:
            own[off:off + n] = True
            v = mo[:, off:off + n]
            if keep is None:
                written(v, "%s: %s" % (what, name))
            else:
                kd = keep.to(dev).expand(B, n, Hh, W)
                written(v[kd], "%s: %s of the listed runs" % (what, name))
                untouched(v[~kd], "%s: %s of the skipped runs" % (what, name))
            chk.add("mid", "%s %s" % (what, name), v, o32[name], o64[name], keep=keep)
        untouched(mo[:, (~own).to(dev)], what + ": mid_out channels outside the heads' offsets")


def run_chain(dev, form):
    Cc, B, Hh, W, pxb = C_SHAPES[form]
    assert H.chain_pixels(B, Cc, Hh * W) == pxb or not DEFAULT_SWITCHES, "%s: the shape no longer reaches its %d-pixel form" % (form, pxb)
    pxb = H.chain_pixels(B, Cc, Hh * W)
    c = level_case(B, Cc, Hh, W, Cc == 256)
    chk = Checks("C " + form)
    wide = Cc == 256
    fused_launch(dev, c, chk, "mid" + (" +LL" if wide else ""), [CHAIN], mid=True, ll=wide)
    fused_launch(dev, c, chk, "no-bias1", [CHAIN], bias1=False)
    fused_launch(dev, c, chk, "plain", [CHAIN])
    rm, listed = H.run_mask("R" + form, B, Hh * W, pxb)
    assert bool(listed.any()) and not bool(listed.all())
    fused_launch(dev, c, chk, "run_mask mid", [CHAIN], mid=True, rmask=rm, listed=listed)
    if wide:
        fused_launch(dev, c, chk, "+LL", [CHAIN], ll=True)
        fused_launch(dev, c, chk, "mid", [CHAIN], mid=True, planes=81)
        # with a run_mask the chained kernel leaves the low-pass chain to a launch of its own, over every pixel
        fused_launch(dev, c, chk, "run_mask +LL", [CHAIN, FUSE_LL], ll=True, rmask=rm, listed=listed)
    chk.done()


@pytest.mark.parametrize("form", list(C_SHAPES))
def test_head_chain_kernel_vs_oracle(dev, form):
    """head_chain_kernel at every width, ragged and exact last blocks, the 8-wave and the 12-wave C = 256 block (picked by the cost
    rule): mid_out at non-zero offsets, bias1 NULL, a run_mask with partly empty runs (skipped runs stay NaN), and at C = 256 the
    low-pass chain riding along (81 planes, 63..80 never written) or left to a launch of its own."""
    if os.environ.get("WMD_HEAD_CHAIN", "1") == "0":
        pytest.skip("the chained kernel is switched off")
    run_chain(dev, form)


def run_fuse(dev, shapes):
    """the FUSE forms of conv_fwd_kernel on the given (C, B, H, W)"""
    for Cc, B, Hh, W in shapes:
        c = level_case(B, Cc, Hh, W, Cc == 256)
        chk = Checks("C fuse C%d %dx%dx%d" % (Cc, B, Hh, W))
        fused_launch(dev, c, chk, "fuse", [FUSE])
        fused_launch(dev, c, chk, "fuse no-bias1", [FUSE], bias1=False)
        if Cc == 256:
            fused_launch(dev, c, chk, "fuse +LL", [FUSE_LL, FUSE], ll=True)
            fused_launch(dev, c, chk, "chain=1", [FUSE_LL], chain=1)
        chk.done()


def test_fuse_forms_vs_oracle(dev):
    """conv_fwd_kernel<fused head> where the chained kernel does not admit the level -- planes that are no multiple of 4 pixels at
    C = 64, 128, 256 (3 x 5), C = 32 at any plane -- and chain = 1, the low-pass chain alone (planes 54..62 of 81)."""
    run_fuse(dev, [(64, 2, 3, 5), (128, 2, 3, 5), (256, 2, 3, 5), (32, 2, 3, 5), (32, 2, 12, 40)])
    c = level_case(1, 256, 12, 40, True)
    chk = Checks("C chain=1 12x40")
    fused_launch(dev, c, chk, "chain=1", [FUSE_LL], chain=1)
    chk.done()


def test_mid_out_needs_the_chained_kernel(dev):
    """mid_out on a level the chained kernel does not admit: WMD_ERR_UNSUPPORTED, nothing launched, nothing written"""
    for Cc, Hh, W in ((64, 3, 5), (32, 12, 40)):
        fused_launch(dev, level_case(2, Cc, Hh, W), None, "mid refused", [], mid=True, status=UNSUPPORTED)


# ---- D. wmd_head_shiftsum_fwd and wmd_head_shiftsum_chain_fwd on a synthetic t ------------------------------------------------------
def shiftsum_case(tag, B, Hh, W, planes):
    g = H.gen(tag)
    return dict(B=B, H=Hh, W=W, t=H.randn(g, B, planes, Hh, W) * 0.5, yl=H.randn(g, B, 1, Hh, W) * 0.6 + 0.5, b3p=H.randn(g, 3) * 0.3,
                b3n=H.randn(g, 3) * 0.3, b3l=H.randn(g, 1) * 0.3)


def shiftsum_args(dev, s, bufs, pad, low, scale, disp_scale=1.0, clamp01=True, sig=False, mask=None, keys=None, t_dev=None, scale_ll=1.5):
    """low: "yl" (low-pass input), "ll" (81 planes: yl_out + bias_ll) or None (yh alone) -> (HeadShiftsumArgs, outputs by name, what to keep alive)"""
    from wavelet_monodepth_amd import _lib
    B, Hh, W = s["B"], s["H"], s["W"]
    o = {"yh": bufs.new("yh", B, 3, Hh, W)}
    keep = [t_dev if t_dev is not None else s["t"].to(dev), s["b3p"].to(dev), s["b3n"].to(dev), s["b3l"].to(dev), s["yl"].to(dev).contiguous(),
            None if mask is None else mask.to(dev)]
    if low:
        o["out"], o["disp"] = bufs.new("out", B, 1, 2 * Hh, 2 * W), bufs.new("disp", B, 1, 2 * Hh, 2 * W)
    if low == "ll":
        o["yl"] = bufs.new("yl_out", B, 1, Hh, W)
    if sig:
        o["sig_p"], o["sig_n"] = bufs.new("sig_p", B, 3, Hh, W), bufs.new("sig_n", B, 3, Hh, W)
        if low == "ll":
            o["sig_ll"] = bufs.new("sig_ll", B, 1, Hh, W)
    a = _lib.HeadShiftsumArgs(B=B, H=Hh, W=W, pad_mode=_lib.PAD[pad], scale=scale, t=ptr(keep[0]), bias_p=ptr(keep[1]), bias_n=ptr(keep[2]),
                              yh=ptr(o["yh"]), yl=ptr(keep[4]) if low == "yl" else None, out=ptr(o.get("out")), disp=ptr(o.get("disp")),
                              disp_scale=disp_scale, clamp01=int(clamp01), bias_ll=ptr(keep[3]) if low == "ll" else None, scale_ll=scale_ll,
                              yl_out=ptr(o.get("yl")), yh_mask=ptr(keep[5]), range_keys=ptr(keys), sig_p=ptr(o.get("sig_p")),
                              sig_n=ptr(o.get("sig_n")), sig_ll=ptr(o.get("sig_ll")))
    return a, o, keep


KIND = {"yh": "yh", "out": "out", "disp": "disp", "yl": "yl", "sig_p": "sig", "sig_n": "sig", "sig_ll": "sig"}


def compare_outputs(chk, what, o, o32, o64, scale):
    for name, v in o.items():
        written(v, "%s: %s" % (what, name))
        shape = o64[name].shape if name != "yh" else v.shape
        chk.add(KIND[name], "%s %s" % (what, name), v.view(shape), o32[name], o64[name], denom=scale if name == "yh" else None)


def shiftsum_launch(dev, s, chk, tag, pad="reflect", low="yl", sig=False, mask=None, clamp01=True, poison=False, keys=None):
    from wavelet_monodepth_amd import _lib
    B, Hh, W = s["B"], s["H"], s["W"]
    what = "%dx%dx%d %s %s %s" % (B, Hh, W, pad, low, tag)
    scale = 2.0
    assert (s["t"].shape[1] == 81) == (low == "ll")
    ref = lambda dt: H.complete(H.cast(s["t"], dt), H.cast(s["b3p"], dt), H.cast(s["b3n"], dt), scale, pad, H.cast(s["yl"], dt) if low == "yl" else None,
                                low == "ll", H.cast(s["b3l"], dt), 1.5, mask, 1.0, clamp01)
    o32, o64 = oracle(("D", B, Hh, W, s["t"].shape[1], pad, low, clamp01, tag if mask is not None else ""), ref)
    if low and clamp01:
        H.clamp_health(o64["pre_disp"], what)
    t_dev = None
    if poison:   # the tap planes of every pixel further than one pixel from the mask: NaN (never written under a run_mask)
        t_dev = torch.where(H.dilate3(mask).unsqueeze(1), s["t"], torch.full_like(s["t"], NAN)).to(dev)
    bufs = Bufs(dev)
    a, o, keep = shiftsum_args(dev, s, bufs, pad, low, scale, clamp01=clamp01, sig=sig, mask=mask, keys=keys, t_dev=t_dev)
    st, kernels = launch(_lib.lib().wmd_head_shiftsum_fwd, a, what)
    assert st == 0, "%s: status %d" % (what, st)
    assert kernels == ["head_shiftsum_kernel"], "%s: %s" % (what, kernels)
    bufs.bands(what)
    compare_outputs(chk, what, o, o32, o64, scale)
    return o


D_SHAPES = [(3, 5, 7), (2, 128, 256)]     # 64-thread blocks (a wavefront straddles frames, dead tail lanes) and 256-thread blocks (65536 pixels)


@pytest.mark.parametrize("shape", D_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shiftsum_vs_oracle(dev, shape):
    """head_shiftsum_kernel on tap planes drawn from a seeded generator: all three pad modes, the low-pass input given, completed
    from planes 54..62 (yl_out + bias_ll) or absent, sig_* written, clamp01 on and off."""
    B, Hh, W = shape
    s54, s81 = shiftsum_case("D54%dx%dx%d" % shape, B, Hh, W, 54), shiftsum_case("D81%dx%dx%d" % shape, B, Hh, W, 81)
    chk = Checks("D shiftsum %dx%dx%d" % shape)
    for pad in ("zero", "reflect", "replicate"):
        shiftsum_launch(dev, s54, chk, "", pad, "yl", sig=pad != "reflect")
        shiftsum_launch(dev, s81, chk, "", pad, "ll", sig=pad != "zero", clamp01=pad != "replicate")
        shiftsum_launch(dev, s54, chk, "", pad, None, sig=pad == "zero")
    chk.done()


def blob_mask(tag, B, Hh, W):
    """uint8 [B,H,W]: a few pixels and short runs, borders and corners among them; most of the map stays empty"""
    g = H.gen(tag)
    m = (torch.rand((B, Hh, W), generator=g) < (0.08 if Hh * W < 1000 else 0.002)).to(torch.uint8)
    m[0, 0, 0] = m[-1, -1, -1] = 1
    if Hh * W > 4:
        m[0, 0, W // 2] = m[-1, Hh // 2, 0] = 1
    else:
        m[0, 0, 1] = m[0, 1, 0] = 0
    return m


@pytest.mark.parametrize("shape", D_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shiftsum_yh_mask_over_poisoned_planes(dev, shape):
    """A yh_mask over tap planes that hold NaN further than one pixel from the mask (what a run_mask leaves behind): the outputs
    are finite and meet the oracle -- under reflect padding, and under zero padding, where the tap weight of a pixel beyond the
    border is 0 and must not meet a NaN."""
    B, Hh, W = shape
    s = shiftsum_case("D54%dx%dx%d" % shape, B, Hh, W, 54)
    m = blob_mask("DM%dx%dx%d" % shape, B, Hh, W)
    chk = Checks("D masked %dx%dx%d" % shape)
    shiftsum_launch(dev, s, chk, "mask", "reflect", "yl", mask=m)
    shiftsum_launch(dev, s, chk, "mask poisoned", "reflect", "yl", mask=m, poison=True)
    shiftsum_launch(dev, s, chk, "mask poisoned", "zero", "yl", mask=m, poison=True)
    shiftsum_launch(dev, s, chk, "mask poisoned", "replicate", None, mask=m, poison=True)
    chk.done()


@pytest.mark.parametrize("masked", [False, True], ids=["dense", "yh_mask"])
@pytest.mark.parametrize("shape", [(3, 5, 7), (1, 2, 2), (2, 128, 256)], ids=lambda s: "x".join(map(str, s)))
def test_shiftsum_range_keys(dev, shape, masked):
    """range_keys armed as wmd_sparse.hip arms them (0xFFFFFFFF, 0): afterwards the keys of every frame decode to the min and max of
    the kernel's own `out` plane of that frame, bit for bit; keys pre-armed with a wider range stay as they are (a fold, not a store)."""
    B, Hh, W = shape
    s = shiftsum_case("D54%dx%dx%d" % shape, B, Hh, W, 54)
    m = blob_mask("DM%dx%dx%d" % shape, B, Hh, W) if masked else None
    chk = Checks("D keys %dx%dx%d%s" % (shape + (" masked" if masked else "",)))
    keys = torch.tensor([[-1, 0]] * B, dtype=torch.int32, device=dev)         # (0xFFFFFFFF, 0)
    o = shiftsum_launch(dev, s, chk, "keys" + (" mask" if masked else ""), "reflect", "yl", mask=m, keys=keys)
    out = o["out"].view(B, -1)
    want = torch.stack([H.key_of(out.min(1).values), H.key_of(out.max(1).values)], 1).cpu()
    got = keys.cpu().to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(got, want), "keys %s, min / max of out %s" % (got.tolist(), want.tolist())
    wide = torch.stack([H.key_of(torch.full((B,), -1e30)), H.key_of(torch.full((B,), 1e30))], 1)
    keys2 = torch.where(wide >= 2 ** 31, wide - 2 ** 32, wide).to(torch.int32).to(dev)
    shiftsum_launch(dev, s, chk, "keys" + (" mask" if masked else ""), "reflect", "yl", mask=m, keys=keys2)
    assert torch.equal(keys2.cpu().to(torch.int64) & 0xFFFFFFFF, wide), "a wider pre-armed range was overwritten"
    chk.done()


def run_shiftsum_chain(dev, B, H0, W0):
    from wavelet_monodepth_amd import _lib
    chk = Checks("D chain %dx%dx%d" % (B, H0, W0))
    scale = [4.0, 2.0, 1.0]
    for low in ("yl", "ll"):
        lv = [shiftsum_case("DC%s%d" % (low, k), B, H0 << k, W0 << k, 81 if (low == "ll" and k == 0) else 54) for k in range(3)]

        def ref(dt, n):
            res, yl = [], H.cast(lv[0]["yl"], dt) if low == "yl" else None
            for k in range(n):
                s = lv[k]
                r = H.complete(H.cast(s["t"], dt), H.cast(s["b3p"], dt), H.cast(s["b3n"], dt), scale[k], "reflect", yl, low == "ll" and k == 0,
                               H.cast(s["b3l"], dt), 1.5, None, 1.0 / scale[k], True)
                res.append(r)
                yl = r["out"]
            return res
        for n in (1, 2, 3):
            what = "%d levels from %dx%dx%d %s" % (n, B, H0, W0, low)
            o32, o64 = oracle(("Dchain", B, H0, W0, low, n), lambda dt: ref(dt, n))
            bufs = Bufs(dev)
            arr, outs, keep = (_lib.HeadShiftsumArgs * n)(), [], []
            for k in range(n):
                a, o, kp = shiftsum_args(dev, lv[k], bufs, "reflect", (low if k == 0 else "chain"), scale[k], disp_scale=1.0 / scale[k])
                arr[k] = a
                outs.append(o)
                keep.append(kp)
            st, kernels = launch(_lib.lib().wmd_head_shiftsum_chain_fwd, arr, what, n)
            assert st == 0, "%s: status %d" % (what, st)
            assert kernels == ["head_shiftsum_chain_kernel"], "%s: %s" % (what, kernels)
            bufs.bands(what)
            for k in range(n):
                H.clamp_health(o64[k]["pre_disp"], "%s level %d" % (what, k))
                compare_outputs(chk, "%s level %d" % (what, k), outs[k], o32[k], o64[k], scale[k])
    chk.done()


@pytest.mark.parametrize("shape", [(2, 3, 5), (1, 6, 20)], ids=lambda s: "x".join(map(str, s)))
def test_shiftsum_chain_vs_oracle(dev, shape):
    """head_shiftsum_chain_kernel: 1, 2 and 3 levels, the first taking yl or completing the low-pass head (yl_out); every level's
    yh, out, disp (and yl_out) against the oracle run through the same chain."""
    run_shiftsum_chain(dev, *shape)


# ---- E. forced switches, in fresh child processes (head_switches() is read once per process) -------------------------------------
def child_A(dev):
    for form in A_SHAPES:
        run_head3x3(dev, form)


def child_C256(dev):
    for form in C_SHAPES:
        if C_SHAPES[form][0] == 256:
            run_chain(dev, form)


def child_fuse(dev):   # WMD_HEAD_CHAIN=0: the FUSE form on planes the chained kernel would take
    run_fuse(dev, [v[:4] for v in C_SHAPES.values() if v[1] <= 2])


def child_level(dev):  # WMD_HEAD_STREAM=0: plain inference on head_level_kernel
    for shape in B_SHAPES:
        run_level_plain(dev, shape, "head_level_kernel")


def child_shiftsum_chain(dev):
    for shape in ((2, 3, 5), (1, 6, 20)):
        run_shiftsum_chain(dev, *shape)


FORCED = [("WMD_HEAD_NG", "2", "child_A"), ("WMD_HEAD_NG", "4", "child_A"), ("WMD_HEAD_CSPLIT", "3", "child_A"),
          ("WMD_HEAD_CHAIN_PG256", "2", "child_C256"), ("WMD_HEAD_CHAIN_PG256", "3", "child_C256"), ("WMD_HEAD_CHAIN", "0", "child_fuse"),
          ("WMD_HEAD_STREAM", "0", "child_level"), ("WMD_SHIFTSUM_CHAIN_SQUARE", "1", "child_shiftsum_chain")]
_CHILD = "import sys, torch, test_gpu_head_fwd as T; getattr(T, sys.argv[1])(torch.device('cuda:0'))"


def test_forced_switches_in_child_processes():
    """Each switch that forces an instantiation, in a process of its own, one after another (stopping at the first that fails):
    the named sections rerun against the oracle, with the host rules of head_ref.py following the switch."""
    here = os.path.dirname(os.path.abspath(__file__))
    for name, value, fn in FORCED:
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env[name] = value
        env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(here), here, env.get("PYTHONPATH", "")])
        r = subprocess.run([sys.executable, "-c", _CHILD, fn], env=env, capture_output=True, text=True, timeout=120)
        print("".join("%s=%s %s\n" % (name, value, line) for line in r.stdout.splitlines() if line.startswith("EDGE")), end="")
        assert r.returncode == 0, "%s=%s %s: exit status %d\n%s\n%s" % (name, value, fn, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
