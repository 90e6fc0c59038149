"""GPU parity: the HIP path (through the C ABI) against the CPU oracle on identical inputs.
Tolerance: north_star asks for <= 1e-4 relative on depth maps; single operators are held to 2e-5
(fp32 accumulation-order noise only)."""
import os

import numpy as np
import pytest
import torch

from oracle import decoder_ref as R
from wavelet_monodepth_amd import synth
from util import quarter_family_declines, R18, assert_close, assert_depth_close, key_str, kitti_feats, load_golden, max_rel, t

pytestmark = pytest.mark.gpu

OP_TOL = 2e-5
NET_TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def test_library_loads_and_reports_version():
    from wavelet_monodepth_amd import _lib
    assert _lib.lib().wmd_version() >= 100


@pytest.mark.parametrize("shape", [(1, 1, 1, 2), (2, 1, 6, 20), (3, 2, 12, 40), (12, 1, 96, 320), (1, 1, 5, 7)])
def test_idwt_forward(dev, shape):
    from wavelet_monodepth_amd import ops
    B, C, h, w = shape
    yl = t(synth.normal((B, C, h, w), "iyl", 1))
    yh = t(synth.normal((B, C, 3, h, w), "iyh", 1))
    ref = R.haar_idwt(yl, yh)
    out, disp = ops.idwt_haar(yl.to(dev), yh.to(dev), disp_scale=0.25, clamp01=True)
    assert_close(out, ref, 1e-6, "idwt")
    assert_close(disp, torch.clamp(ref * 0.25, 0, 1), 1e-6, "disp")
    out2, none = ops.idwt_haar(yl.to(dev), yh.to(dev))
    assert none is None and torch.equal(out2, out)


def test_idwt_vs_pywavelets_golden(dev):
    from wavelet_monodepth_amd import ops
    g = load_golden("pywt_haar.npz")
    for name, (h, w) in {"a": (4, 6), "b": (12, 40), "c": (7, 5), "d": (24, 80)}.items():
        yl = t(synth.normal((h, w), "pywt_yl_" + name, 11)).reshape(1, 1, h, w)
        yh = t(synth.normal((3, h, w), "pywt_yh_" + name, 11)).reshape(1, 1, 3, h, w)
        out, _ = ops.idwt_haar(yl.to(dev), yh.to(dev))
        assert_close(out[0, 0], g["idwt_" + name], 1e-6, "idwt_" + name)


def test_dwt_vs_pywavelets_golden_and_roundtrip(dev):
    from wavelet_monodepth_amd import ops
    g = load_golden("pywt_haar.npz")
    # o1..o3: odd sizes (an odd axis gets one reflected sample: mode="reflect" of DWTForward / pywt.dwt2)
    for name, (h, w, J) in {"a": (8, 12, 1), "b": (48, 160, 4), "c": (240, 320, 4), "o1": (7, 9, 1), "o2": (15, 22, 3),
                            "o3": (30, 45, 4)}.items():
        x = t(synth.normal((h, w), "pywt_x_" + name, 12)).reshape(1, 1, h, w).to(dev)
        yl, yh = ops.dwt_haar(x, J)
        assert_close(yl[0, 0], g["dwt_%s_yl" % name], 2e-6, "yl")
        for j in range(J):
            k = "dwt_%s_yh%d" % (name, j)
            if k in g:
                assert_close(yh[j][0, 0], g[k], 2e-6, k)
        rec = yl
        for j in reversed(range(J)):
            rec, _ = ops.idwt_haar(rec, yh[j])
            fh, fw = (yh[j - 1].shape[-2:] if j else (h, w))      # crop the reflected sample of an odd level again
            rec = rec[:, :, :fh, :fw].contiguous()
        assert_close(rec, x, 2e-6, "idwt(dwt(x))")


def test_idwt_backward(dev):
    from wavelet_monodepth_amd import ops
    yl = t(synth.normal((2, 1, 6, 10), "byl", 2)).requires_grad_(True)
    yh = t(synth.normal((2, 1, 3, 6, 10), "byh", 2)).requires_grad_(True)
    gw = t(synth.normal((2, 1, 12, 20), "bgw", 2))
    gd = t(synth.normal((2, 1, 12, 20), "bgd", 2))
    ref = R.haar_idwt(yl, yh)
    ((ref * gw).sum() + (torch.clamp(ref * 0.5, 0, 1) * gd).sum()).backward()
    yl_g = yl.detach().to(dev).requires_grad_(True)
    yh_g = yh.detach().to(dev).requires_grad_(True)
    out, disp = ops.idwt_haar(yl_g, yh_g, disp_scale=0.5, clamp01=True)
    ((out * gw.to(dev)).sum() + (disp * gd.to(dev)).sum()).backward()
    assert_close(yl_g.grad, yl.grad, 1e-5, "d_yl")
    assert_close(yh_g.grad, yh.grad, 1e-5, "d_yh")


CONV_CASES = [
    # B, C1, C2, up, Cout, H, W, k, pad, act
    (2, 3, 0, 1, 5, 6, 10, 3, "reflect", "none"),
    (2, 19, 0, 1, 7, 5, 8, 3, "zero", "elu"),
    (1, 37, 0, 1, 32, 8, 12, 3, "reflect", "elu"),
    (2, 16, 8, 2, 19, 4, 6, 3, "reflect", "elu"),        # fused upsample + concat, ragged Cout
    (2, 32, 64, 2, 32, 12, 40, 3, "reflect", "elu"),     # upconv(1,1) structure
    (1, 64, 0, 1, 32, 48, 160, 3, "reflect", "elu"),     # 32-wide tiles
    (2, 512, 0, 1, 256, 6, 20, 3, "reflect", "elu"),     # coarsest level, split-K territory
    (1, 256, 256, 2, 256, 12, 40, 3, "reflect", "elu"),
    (1, 40, 0, 1, 24, 15, 20, 3, "replicate", "none"),   # NYUv2 conv2-like (odd H)
    (1, 23, 10, 2, 13, 30, 40, 3, "reflect", "leaky"),   # NYUv2 UpSampleBlock-like, odd channels
    (2, 21, 0, 1, 9, 5, 7, 1, "zero", "none"),           # 1x1
    (2, 256, 0, 1, 256, 12, 40, 1, "zero", "leaky"),     # head 1x1
    (1, 32, 0, 1, 32, 96, 320, 1, "zero", "leaky"),
    (1, 138, 0, 1, 3, 9, 11, 3, "zero", "none"),         # tiny Cout through the MFMA path
    (3, 8, 0, 1, 16, 2, 2, 3, "reflect", "sigmoid"),     # smallest legal reflect size
    (1, 5, 0, 1, 4, 1, 9, 3, "zero", "none"),            # H = 1
    # upsampled operand under every pad mode, whole chunks of 8 channels (the low-resolution Winograd path of
    # conv_wino32_kernel: the pad ring maps onto the border source pixel / onto zero), tile overhang in both directions
    (2, 16, 16, 2, 20, 12, 24, 3, "zero", "elu"),
    (1, 8, 24, 2, 33, 10, 20, 3, "replicate", "leaky"),
    (1, 16, 16, 2, 40, 18, 44, 3, "reflect", "none"),
    (2, 24, 0, 2, 32, 8, 16, 3, "reflect", "elu"),       # upsample without a skip tensor
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_conv_forward(dev, case):
    from wavelet_monodepth_amd import ops
    B, C1, C2, up, Cout, H, W, k, pad, act = case
    x1 = t(synth.normal((B, C1, H // up, W // up), "cx1", 3))
    x2 = t(synth.normal((B, C2, H, W), "cx2", 3)) if C2 else None
    w, b = synth.conv_params("cw", Cout, C1 + C2, k, 3)
    w, b = t(w), t(b)
    xin = R.up2(x1) if up == 2 else x1
    if x2 is not None:
        xin = torch.cat([xin, x2], 1)
    ref = R.conv3x3(xin, w, b, pad) if k == 3 else R.conv1x1(xin, w, b)
    slope = 0.1
    ref = {"none": lambda v: v, "elu": torch.nn.functional.elu, "leaky": lambda v: torch.nn.functional.leaky_relu(v, slope),
           "sigmoid": torch.sigmoid}[act](ref)
    y = ops.conv2d_fused(x1.to(dev), w.to(dev), b.to(dev), x2=None if x2 is None else x2.to(dev), up1=up, pad=pad,
                         act=act, slope=slope)
    assert_close(y, ref, OP_TOL, "conv")


def test_conv_every_tile_configuration_and_split(dev):
    """Force each entry of the library's configuration table (and several K splits) on one ragged problem."""
    import ctypes as C
    from wavelet_monodepth_amd import _lib, ops, tuner
    B, C1, C2, Cout, H, W = 2, 40, 24, 70, 24, 40
    x1 = t(synth.normal((B, C1, H // 2, W // 2), "tx1", 9))
    x2 = t(synth.normal((B, C2, H, W), "tx2", 9))
    names = tuner.config_names()
    assert len(names) >= 10
    for k in (3, 1):
        w, b = [t(a) for a in synth.conv_params("tw%d" % k, Cout, C1 + C2 if k == 3 else C2, k, 9)]
        if k == 3:
            ref = torch.nn.functional.elu(R.conv3x3(torch.cat([R.up2(x1), x2], 1), w, b, "reflect"))
        else:
            ref = torch.nn.functional.elu(R.conv1x1(x2, w, b))
        wp = ops.pack_weights(w.to(dev))
        ww = ops.pack_weights_wino(w.to(dev))
        xa, xb = (x1.to(dev), x2.to(dev)) if k == 3 else (x2.to(dev), None)
        l = _lib.lib()
        tested = 0
        for i, name in enumerate(names):
            if name.startswith("conv_wino") and ww is None:   # family switched off (WMD_WINOGRAD=0)
                continue
            if not (name.endswith(",%d>" % (9 if k == 3 else 1)) or (k == 3 and name.startswith("conv_wino"))):
                continue
            for ks in (1, 2, 3):
                y = torch.full((B, Cout, H, W), float("nan"), device=dev)
                a = _lib.ConvArgs(B=B, H=H, W=W, C1=xa.shape[1], up1=2 if k == 3 else 1, C2=0 if xb is None else C2, Cout=Cout,
                                  ksize=k, pad_mode=1, act=1, slope=0.0, x1=xa.data_ptr(), x2=None if xb is None else xb.data_ptr(),
                                  wp=wp.data_ptr(), bias=b.to(dev).data_ptr(), y=y.data_ptr(), workspace=None,
                                  workspace_floats=0, tune_cfg=i + 1, tune_ksplit=ks, wp_wino=None if ww is None else ww.data_ptr())
                n = l.wmd_conv_fwd_workspace_floats(C.byref(a))
                ws = torch.empty(max(n, 1), device=dev)
                a.workspace, a.workspace_floats = ws.data_ptr(), n
                st = l.wmd_conv_fwd(C.byref(a), torch.cuda.current_stream().cuda_stream)
                if st == -3 and ks > 1:
                    continue  # this tile's channel chunk leaves fewer than ks chunks to split
                if quarter_family_declines(name, xa.shape[1], 0 if xb is None else C2):
                    assert st == -3, name
                    continue
                _lib.check(st, name)
                assert_close(y, ref, OP_TOL, "%s ksplit %d" % (name, ks))
                tested += 1
        assert tested >= (12 if k == 3 else 4)


@pytest.mark.skipif(os.environ.get("WMD_WINOGRAD", "1") == "0", reason="Winograd family switched off (WMD_WINOGRAD=0)")
@pytest.mark.parametrize("case", [c for c in CONV_CASES if c[7] == 3], ids=lambda c: "x".join(str(v) for v in c))
def test_conv_winograd_configurations(dev, case):
    """Every Winograd F(2x2,3x3) configuration, forced, on every 3x3 case (pads, upsample + concat, odd sizes, ragged
    channels, H = 1) against the oracle; the transform costs a little rounding: 5e-5 relative instead of 2e-5."""
    import ctypes as C
    from wavelet_monodepth_amd import _lib, ops, tuner
    B, C1, C2, up, Cout, H, W, k, pad, act = case
    x1 = t(synth.normal((B, C1, H // up, W // up), "cx1", 3))
    x2 = t(synth.normal((B, C2, H, W), "cx2", 3)) if C2 else None
    w, b = [t(a) for a in synth.conv_params("cw", Cout, C1 + C2, k, 3)]
    xin = R.up2(x1) if up == 2 else x1
    if x2 is not None:
        xin = torch.cat([xin, x2], 1)
    slope = 0.1
    ref = {"none": lambda v: v, "elu": torch.nn.functional.elu, "leaky": lambda v: torch.nn.functional.leaky_relu(v, slope),
           "sigmoid": torch.sigmoid}[act](R.conv3x3(xin, w, b, pad))
    wd, bd = w.to(dev), b.to(dev)
    wp, ww = ops.pack_weights(wd), ops.pack_weights_wino(wd)
    x1d, x2d = x1.to(dev), None if x2 is None else x2.to(dev)
    l = _lib.lib()
    tested = 0
    for i, name in enumerate(tuner.config_names()):
        if not name.startswith("conv_wino"):
            continue
        got = {}
        for ks in (1, 2, -2):     # (round 6) 2: finished inside the convolution where the kernel can; -2: by the second-stage kernel
            y = torch.full((B, Cout, H, W), float("nan"), device=dev)
            a = _lib.ConvArgs(B=B, H=H, W=W, C1=C1, up1=up, C2=C2, Cout=Cout, ksize=3, pad_mode=ops.PAD[pad], act=ops.ACT[act],
                              slope=slope, x1=x1d.data_ptr(), x2=None if x2d is None else x2d.data_ptr(), wp=wp.data_ptr(),
                              bias=bd.data_ptr(), y=y.data_ptr(), workspace=None, workspace_floats=0, tune_cfg=i + 1,
                              tune_ksplit=ks, wp_wino=ww.data_ptr())
            n = l.wmd_conv_fwd_workspace_floats(C.byref(a))
            ws = torch.empty(max(n, 1), device=dev)
            a.workspace, a.workspace_floats = ws.data_ptr(), n
            st = l.wmd_conv_fwd(C.byref(a), torch.cuda.current_stream().cuda_stream)
            if st == -3 and ks != 1:
                continue      # fewer than two chunks to split / a kernel without the in-kernel finish refuses "-k"
            if quarter_family_declines(name, C1, C2):
                assert st == -3, name
                continue
            _lib.check(st, name)
            assert_close(y, ref, 5e-5, "%s ksplit %d" % (name, ks))
            got[ks] = y
            tested += 1
        if 2 in got and -2 in got:    # same partial planes, same summation order: the two finishes differ by the activation's arithmetic only
            assert name.startswith("conv_wino32"), name
            if act in ("none", "leaky"):
                assert torch.equal(got[2], got[-2]), "%s: in-kernel finish != second-stage sum" % name
            else:
                assert_close(got[2], got[-2], 2e-6, "%s in-kernel finish vs second-stage sum" % name)
    assert tested >= 2


@pytest.mark.skipif(os.environ.get("WMD_WINOGRAD", "1") == "0", reason="Winograd family switched off (WMD_WINOGRAD=0)")
@pytest.mark.parametrize("name,ks,shape", [("conv_wino32_kernel<6,40,2,8>", 4, (12, 12, 40, 256, 2, 256, 256)),
                                           ("conv_wino32q_kernel<4,32,8>", 4, (12, 6, 20, 512, 1, 0, 256)),
                                           ("conv_wino32_kernel<12,40,4,8>", 8, (12, 12, 40, 256, 1, 0, 128)),
                                           ("conv_wino32q_kernel<8,16,8>", 6, (1, 48, 160, 64, 2, 64, 64))])
def test_splitk_in_kernel_finish_is_coherent_across_xcds(dev, name, ks, shape):
    """Round 6 (VERDICT r5 #2a): the K-slice blocks of a tile run on different XCDs, whose L2s are not coherent with each other;
    the partial tiles travel by write-through stores + agent-scope loads behind a relaxed ticket (splitk_ticket_finish).  A stale
    line or a ticket drawn before the stores landed would show as a changed value: the forward's split layers at their real sizes,
    40 launches each into a NaN-filled output over a workspace poisoned before every launch -- every launch bit-identical to the
    first and equal to the second-stage sum of the same slices (activation ELU: 2e-6), and the ticket region back at zero (the
    next launch on it -- a graph replay -- must start from armed counters)."""
    import ctypes as C
    from wavelet_monodepth_amd import _lib, ops, tuner
    B, H, W, C1, up, C2, Cout = shape
    names = tuner.config_names()
    if name not in names:
        pytest.skip("%s is not in this build's table" % name)
    x1 = t(synth.normal((B, C1, H // up, W // up), "kx1", 21)).to(dev)
    x2 = t(synth.normal((B, C2, H, W), "kx2", 21)).to(dev) if C2 else None
    w, b = [t(a).to(dev) for a in synth.conv_params("kw", Cout, C1 + C2, 3, 21)]
    wp, ww = ops.pack_weights(w), ops.pack_weights_wino(w)
    l = _lib.lib()

    def run(k, y, ws=None):
        a = _lib.ConvArgs(B=B, H=H, W=W, C1=C1, up1=up, C2=C2, Cout=Cout, ksize=3, pad_mode=1, act=1, slope=0.0, x1=x1.data_ptr(),
                          x2=None if x2 is None else x2.data_ptr(), wp=wp.data_ptr(), bias=b.data_ptr(), y=y.data_ptr(), workspace=None,
                          workspace_floats=0, tune_cfg=names.index(name) + 1, tune_ksplit=k, wp_wino=ww.data_ptr())
        n = l.wmd_conv_fwd_workspace_floats(C.byref(a))
        ws = torch.empty(max(n, 1), device=dev) if ws is None else ws
        ws.fill_(float("nan"))
        a.workspace, a.workspace_floats = ws.data_ptr(), n
        _lib.check(l.wmd_conv_fwd(C.byref(a), torch.cuda.current_stream().cuda_stream), name)
        return ws

    ref = torch.full((B, Cout, H, W), float("nan"), device=dev)
    run(-ks, ref)
    first = torch.full_like(ref, float("nan"))
    ws = run(ks, first)
    assert bool(torch.isfinite(first).all())
    assert_close(first, ref, 2e-6, "%s: in-kernel finish vs second-stage sum, %d slices" % (name, ks))
    for rep in range(40):
        y = torch.full_like(ref, float("nan"))
        run(ks, y, ws)
        assert torch.equal(y, first), "%s: launch %d differs from the first" % (name, rep)



@pytest.mark.skipif(os.environ.get("WMD_WINOGRAD", "1") == "0", reason="Winograd family switched off (WMD_WINOGRAD=0)")
@pytest.mark.parametrize("up,C1,C2,pad", [(2, 32, 48, "reflect"), (1, 64, 0, "reflect"), (2, 16, 24, "zero"), (2, 20, 12, "replicate")])
def test_conv_block_sparse_every_winograd_configuration(dev, up, C1, C2, pad):
    """Block-sparse execution (wmd_conv_args.in_mask / out_mask, KITTI/layers.py:439-453 semantics) on every Winograd
    configuration and split-K: input positions outside in_mask read 0 after the coordinate padding, outputs outside out_mask
    are 0, tiles without an active pixel are not computed (out is zero-initialised).  The upsampled operand is masked through
    a 2x2-constant mask (the decoders' upsample mask) with and without the in_mask_2x2 promise: conv_wino32_kernel's flattened
    staging (channel counts that are multiples of its chunk) and the generic gather must agree with the oracle."""
    import ctypes as C
    from wavelet_monodepth_amd import _lib, ops, tuner
    B, Cout, H, W = 2, 40, 40, 72
    gen = torch.Generator().manual_seed(11)
    x1 = t(synth.normal((B, C1, H // up, W // up), "mx1", 5))
    x2 = t(synth.normal((B, C2, H, W), "mx2", 5)) if C2 else None
    w, b = [t(a) for a in synth.conv_params("mw", Cout, C1 + C2, 3, 5)]
    coarse = (torch.rand((B, H // 2, W // 2), generator=gen) < 0.6)
    coarse[:, :, : W // 4] &= torch.rand((B, H // 2, W // 4), generator=gen) < 0.2
    in_mask = coarse.repeat_interleave(2, 1).repeat_interleave(2, 2)                  # constant on 2x2 blocks
    out_mask = torch.rand((B, H, W), generator=gen) < 0.5
    out_mask[:, :16, :32] = False                                                      # whole tiles without active pixels
    out_mask[1, 24:, 40:] = False
    xin = R.up2(x1) if up == 2 else x1
    if x2 is not None:
        xin = torch.cat([xin, x2], 1)
    ref = torch.nn.functional.elu(R.conv3x3(xin * in_mask[:, None].float(), w, b, pad)) * out_mask[:, None].float()
    wd, bd = w.to(dev), b.to(dev)
    wp, ww = ops.pack_weights(wd), ops.pack_weights_wino(wd)
    x1d, x2d = x1.to(dev), None if x2 is None else x2.to(dev)
    im, om = in_mask.to(torch.uint8).to(dev).contiguous(), out_mask.to(torch.uint8).to(dev).contiguous()
    l = _lib.lib()
    tested = 0
    for i, name in enumerate(tuner.config_names()):
        if not name.startswith("conv_wino"):
            continue
        for promise in (1, 0):
            for ks in (1, 2):
                y = torch.zeros((B, Cout, H, W), device=dev)
                a = _lib.ConvArgs(B=B, H=H, W=W, C1=C1, up1=up, C2=C2, Cout=Cout, ksize=3, pad_mode=ops.PAD[pad], act=ops.ACT["elu"],
                                  slope=0.0, x1=x1d.data_ptr(), x2=None if x2d is None else x2d.data_ptr(), wp=wp.data_ptr(),
                                  bias=bd.data_ptr(), y=y.data_ptr(), workspace=None, workspace_floats=0, tune_cfg=i + 1,
                                  tune_ksplit=ks, wp_wino=ww.data_ptr(), in_mask=im.data_ptr(), out_mask=om.data_ptr(),
                                  in_mask_2x2=promise)
                n = l.wmd_conv_fwd_workspace_floats(C.byref(a))
                ws = torch.full((max(n, 1),), float("nan"), device=dev)     # a skipped tile's slots must never be read
                a.workspace, a.workspace_floats = ws.data_ptr(), n
                st = l.wmd_conv_fwd(C.byref(a), torch.cuda.current_stream().cuda_stream)
                if st == -3 and ks > 1:
                    continue
                if quarter_family_declines(name, C1, C2, masked=True, up=up, promise=promise):
                    assert st == -3, name
                    continue
                _lib.check(st, name)
                assert_close(y, ref, 5e-5, "%s ksplit %d promise %d" % (name, ks, promise))
                tested += 1
    assert tested >= 8


@pytest.mark.parametrize("case", [(2, 512, 6, 20, 256, 3, "reflect", 1), (1, 40, 10, 32, 70, 3, "replicate", 1), (2, 24, 8, 10, 20, 3, "reflect", 2), (1, 24, 7, 9, 20, 3, "reflect", 1),
                                  (1, 2208, 15, 20, 96, 1, "zero", 1), (2, 64, 12, 40, 32, 3, "reflect", 1)],
                         ids=lambda c: "x".join(str(v) for v in c))
def test_conv_pre_activation_edge_vs_oracle(dev, case):
    """Encoder edge (ops.conv2d_pre_activated): the convolution of act(x1 * scale[c] + shift[c]).  Against the oracle's
    convolution of the explicitly activated tensor: the KITTI coarsest maps (R18 6x20 with 512 channels), ragged channels /
    sizes, upsampling, DenseNet161's 2208-channel 1x1, with and without the affine, ReLU and LeakyReLU."""
    import ctypes as C
    from wavelet_monodepth_amd import _lib, ops
    B, C1, H, W, Cout, k, pad, up = case
    x = t(synth.normal((B, C1, H // up, W // up), "ex", 7))
    w, b = [t(a) for a in synth.conv_params("ew", Cout, C1, k, 7)]
    sc = t(synth.uniform((C1,), "esc", 7, 0.5, 1.5))
    sh = t(synth.uniform((C1,), "esh", 7, -0.5, 0.5))
    for scale, shift, slope in ((None, None, 0.0), (sc, sh, 0.0), (sc, None, 0.2)):
        v = x
        if scale is not None:
            v = v * scale.view(1, -1, 1, 1)
        if shift is not None:
            v = v + shift.view(1, -1, 1, 1)
        v = torch.nn.functional.leaky_relu(v, slope)
        v = R.up2(v) if up == 2 else v
        ref = torch.nn.functional.elu(R.conv3x3(v, w, b, pad) if k == 3 else R.conv1x1(v, w, b))
        pre = (None if scale is None else scale.to(dev), None if shift is None else shift.to(dev), "leaky", slope)
        with torch.no_grad():
            y = ops.conv2d_pre_activated(x.to(dev), pre, w.to(dev), b.to(dev), up1=up, pad=pad, act="elu")
        assert_close(y, ref, OP_TOL, "pre-activation edge %s" % (pre[2:],))
    xd, bd, scd, shd = x.to(dev), b.to(dev), sc.to(dev), sh.to(dev)
    with pytest.raises(_lib.WmdError):      # the edge's activation is the identity or a (leaky) ReLU
        ops.conv2d_pre_activated(xd, (scd, shd, "elu", 0.0), w.to(dev), bd, up1=up, pad=pad)


def test_kitti_decoders_take_a_deferred_last_feature(dev):
    """The dense and the sparse wavelet decoder fed with the encoder's last PRE-activation (layers.DeferredActivation: ReLU on
    load in upconv(4,0)) give the outputs of the ordinary call on the activated tensor -- eagerly and from the replayed graph --
    and under autograd the wrapper is activated explicitly (same gradients)."""
    from wavelet_monodepth_amd.kitti import DepthWaveProgressiveDecoder, SparseDepthWaveProgressiveDecoder
    from wavelet_monodepth_amd.layers import DeferredActivation
    chans = [64, 64, 128, 256, 512]
    feats = [f.to(dev) for f in kitti_feats(2, 64, 96, seed=4)]
    pre = feats[-1] * 2.0 - 0.3                                  # a tensor with negative values
    act = torch.relu(pre)
    for cls, kw in ((DepthWaveProgressiveDecoder, {}), (SparseDepthWaveProgressiveDecoder, {"thresh_ratio": 0.05})):
        dec = synth.fill_state_dict(cls(np.array(chans)), seed=2).to(dev)
        fa = [f[:1] for f in feats[:-1]] + [act[:1]] if kw else feats[:-1] + [act]
        fp = [f[:1] for f in feats[:-1]] + [DeferredActivation(pre[:1])] if kw else feats[:-1] + [DeferredActivation(pre)]
        with torch.no_grad():
            want = dict(dec(fa, **kw))
            for graph in (False, True):
                dec.enable_graph(graph)
                for _ in range(2 if graph else 1):
                    got = dec(fp, **kw)
                for s in range(4):
                    assert_close(got[("disp", s)], want[("disp", s)].cpu(), 1e-5, "%s graph=%s disp %d" % (cls.__name__, graph, s))
            dec.enable_graph(False)
    dec = synth.fill_state_dict(DepthWaveProgressiveDecoder(np.array(chans)), seed=2).to(dev)
    p1, p2 = pre.clone().requires_grad_(True), pre.clone().requires_grad_(True)
    o1 = dec(feats[:-1] + [DeferredActivation(p1)])
    o2 = dec(feats[:-1] + [torch.relu(p2)])
    sum((o1[("disp", s)] ** 2).mean() for s in range(4)).backward()
    sum((o2[("disp", s)] ** 2).mean() for s in range(4)).backward()
    assert_close(p1.grad, p2.grad.cpu(), 1e-5, "gradient through the activated edge")


def test_conv_rejects_bad_input(dev):
    from wavelet_monodepth_amd import ops, _lib
    w = torch.zeros(4, 3, 3, 3, device=dev)
    with pytest.raises(_lib.WmdError):
        ops.conv2d_fused(torch.zeros(1, 3, 1, 5, device=dev), w, None, pad="reflect")   # reflect needs H >= 2
    with pytest.raises(_lib.WmdError):
        ops.conv2d_fused(torch.zeros(1, 2, 4, 4, device=dev), w, None)                   # channel mismatch
    with pytest.raises(_lib.WmdError):
        ops.conv2d_fused(torch.zeros(1, 3, 4, 4), w.cpu(), None)                          # CPU tensors: no fallback


@pytest.mark.parametrize("mode,cout,pad", [(0, 3, "zero"), (0, 1, "replicate"), (1, 1, "reflect"), (2, 3, "reflect")])
@pytest.mark.parametrize("shape", [(2, 20, 12, 40), (1, 32, 9, 35), (1, 7, 2, 2)])
def test_head3x3(dev, mode, cout, pad, shape):
    from wavelet_monodepth_amd import ops
    B, C, H, W = shape
    xp = t(synth.normal((B, C, H, W), "hxp", 4))
    xn = t(synth.normal((B, C, H, W), "hxn", 4))
    wp, bp = [t(a) for a in synth.conv_params("hwp", cout, C, 3, 4)]
    wn, bn = [t(a) for a in synth.conv_params("hwn", cout, C, 3, 4)]
    scale = 4.0
    cp = R.conv3x3(xp, wp, bp, pad)
    if mode == 0:
        ref = scale * cp
    elif mode == 1:
        ref = scale * torch.sigmoid(cp)
    else:
        ref = scale * torch.sigmoid(cp) - scale * torch.sigmoid(R.conv3x3(xn, wn, bn, pad))
    y = ops.head3x3(xp.to(dev), wp.to(dev), bp.to(dev), xn.to(dev) if mode == 2 else None,
                    wn.to(dev) if mode == 2 else None, bn.to(dev) if mode == 2 else None, pad=pad, mode=mode, scale=scale)
    # differences of sigmoids cancel: compare on the scale of the operands
    err = float((y.cpu() - ref).abs().max()) / scale
    assert err < 2e-6, err


def _kitti_decoder(dev, seed=1):
    from wavelet_monodepth_amd.kitti import DepthWaveProgressiveDecoder
    dec = synth.fill_state_dict(DepthWaveProgressiveDecoder(np.array(R18)), seed=seed)
    return dec.to(dev)


def test_kitti_dense_decoder_vs_reference_golden(dev):
    """Identical synth weights + features as tests/golden/make_golden.py fed to the reference module."""
    gold = load_golden("kitti_dense_r18_64x64.npz")
    dec = _kitti_decoder(dev)
    with torch.no_grad():
        out = dec([f.to(dev) for f in kitti_feats(2, 64, 64)])
    assert set(key_str(k) for k in out) == set(gold)
    for k, v in out.items():
        assert_close(v, gold[key_str(k)], NET_TOL, key_str(k))


def test_kitti_dense_decoder_config2_vs_oracle(dev):
    """BASELINE config 2 shapes (640x192, R18) at batch 2 (the oracle needs ~1 s per sample)."""
    dec = _kitti_decoder(dev, seed=5)
    feats = kitti_feats(2, 192, 640, seed=5)
    sd = {k: v.cpu() for k, v in dec.state_dict().items()}
    with torch.no_grad():
        ref = R.kitti_wave_decoder(feats, sd)
        out = dec([f.to(dev) for f in feats])
    for k in ref:
        assert_close(out[k], ref[k], NET_TOL, key_str(k))


def test_kitti_dense_decoder_batch12_properties(dev):
    """Full config-2 batch: per-sample independence (batch 12 == 12 x batch 1 on a subset) and
    IDWT consistency: disp_s == clamp(idwt chain of the logged coefficients)."""
    dec = _kitti_decoder(dev, seed=6)
    feats = [f.to(dev) for f in kitti_feats(12, 192, 640, seed=6)]
    with torch.no_grad():
        out = {k: v.clone() for k, v in dec(feats).items()}
        one = dec([f[7:8] for f in feats])
    for s in range(4):
        assert_close(out[("disp", s)][7:8], one[("disp", s)], 1e-6, "batch independence")
    yl = out[("wavelets", 3, "LL")].cpu()
    for s in (3, 2, 1, 0):
        yh = torch.stack([out[("wavelets", s, b)].cpu() for b in ("LH", "HL", "HH")], 2)
        assert_close(out[("wavelets", s, "LL")].cpu(), yl, 1e-6, "LL chain")
        yl = R.haar_idwt(yl, yh)
        assert_close(out[("disp", s)].cpu(), torch.clamp(yl / 2 ** s, 0, 1), 1e-6, "disp%d" % s)


def test_kitti_dense_decoder_graph_replay_and_grad_mode_paths_agree(dev):
    """Three execution paths of the same module: eager no_grad (stacked heads), eager with autograd enabled
    (per-head operators) and hipGraph replay must produce the same maps."""
    dec = _kitti_decoder(dev, seed=3)
    feats = [f.to(dev) for f in kitti_feats(2, 64, 96, seed=3)]
    with torch.no_grad():
        ref = {k: v.clone() for k, v in dec(feats).items()}
    with torch.enable_grad():
        out_g = dec(feats)
    for k in ref:
        assert_close(out_g[k], ref[k], 2e-6, "grad-mode path " + key_str(k))
    dec.enable_graph(True)
    with torch.no_grad():
        for _ in range(3):
            out = dec(feats)
        for k in ref:
            assert_close(out[k], ref[k], 2e-6, "graph replay " + key_str(k))
        feats2 = [f * 0.5 for f in feats]              # new buffers -> new capture
        a = {k: v.clone() for k, v in dec(feats2).items()}
        dec.enable_graph(False)
        b = dec(feats2)
        for k in a:
            assert_close(a[k], b[k], 2e-6, "graph vs eager " + key_str(k))


@pytest.mark.parametrize("hw", [(96, 160), (64, 64), (192, 640)])
def test_chained_completion_of_levels_4_to_2_equals_the_per_level_launches(dev, hw, monkeypatch):
    """Round 5: the dense decoder's inference forward completes levels 4, 3 and 2 in ONE launch (wmd_head_shiftsum_chain_fwd: a block
    walks a 4 x 4 coarse tile down two levels through LDS) instead of three wmd_head_shiftsum_fwd launches.  Same arithmetic per
    pixel: every output must be bit-identical, on maps whose coarsest level is not a multiple of the 4 x 4 tile, eager and replayed,
    and equal to the oracle."""
    import numpy as np
    from wavelet_monodepth_amd import ops
    from wavelet_monodepth_amd.kitti import DepthWaveProgressiveDecoder
    H, W = hw
    B = 2
    dec = synth.fill_state_dict(DepthWaveProgressiveDecoder(np.array(R18)), seed=3).to(dev)
    feats = kitti_feats(B, H, W, seed=5)
    gf = [f.to(dev) for f in feats]
    monkeypatch.setattr(ops, "_SHIFTSUM_CHAIN_MAX_PIXELS", 1 << 30)      # (the default switches it off for large batches)
    assert ops.shiftsum_chain_supported([256, 128, 64], B * (H // 4) * (W // 4))
    with torch.no_grad():
        got = {k: v.clone() for k, v in dec(gf).items()}
        dec.enable_graph(True)
        for _ in range(2):
            rep = dec(gf)
        rep = {k: v.clone() for k, v in rep.items()}
        dec.enable_graph(False)
        monkeypatch.setattr(ops, "_SHIFTSUM_CHAIN", False)
        want = dec(gf)
        ref = R.kitti_wave_decoder(feats, {k: v.cpu() for k, v in dec.state_dict().items()})
    assert set(got) == set(want) == set(ref)
    for k in want:
        assert torch.equal(got[k], want[k]), "%s: chained completion differs from the per-level launches" % key_str(k)
        assert torch.equal(rep[k], want[k]), "%s: replayed chained completion differs" % key_str(k)
        assert_close(got[k], ref[k], 1e-4, key_str(k))


def test_config2_in_the_benchmarked_execution_mode_vs_oracle(dev):
    """Round-2 VERDICT: what bench.py times -- BASELINE config 2 at batch 12, hipGraph replay (the decoder's default graph
    mode), the COMMITTED tile choices preloaded -- held against the oracle: three sampled frames, every disparity map and
    coefficient plane <= 1e-4 (north_star's tolerance); the second replay must reproduce the first bit for bit."""
    import importlib.util
    from wavelet_monodepth_amd import tuner
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    tuner.preload(os.path.join(root, "profiles", bench.TUNE_CACHE))
    dec = _kitti_decoder(dev, seed=1)
    feats = [f.to(dev) for f in kitti_feats(12, 192, 640)]
    dec.enable_graph(True)
    assert dec.two_stream_graphs == (os.environ.get("WMD_TWO_STREAM_GRAPHS", "0") == "1")     # bench.py uses the default
    with torch.no_grad():
        for _ in range(3):
            out = dec(feats)
        first = {k: v.clone() for k, v in out.items()}
        out = dec(feats)
        for k in first:
            assert torch.equal(out[k], first[k]), "replay is not repeatable: " + key_str(k)
        sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
        for fr in (0, 5, 11):
            ref = R.kitti_wave_decoder([f[fr:fr + 1].cpu() for f in feats], sd)
            assert set(ref) == set(out)
            for k, v in ref.items():
                assert_close(out[k][fr:fr + 1], v, 1e-4, "frame %d %s" % (fr, key_str(k)))
            for s_ in range(4):      # per pixel on DEPTH (north_star's wording), not norm-wise on the disparity
                assert_depth_close(out[("disp", s_)][fr:fr + 1], ref[("disp", s_)], 1e-4, "frame %d depth %d" % (fr, s_))


def test_bound_static_inputs_replay_fresh_tensors_without_recapturing(dev):
    """decoder.bind_inputs: a caller whose encoder returns NEW tensors every step (trainer.py:240-241) used to re-capture the
    graph segments on every call; with decoder-owned static input buffers the fresh tensors are copied in and the one capture
    is replayed -- zero further captures, same maps as the eager forward."""
    dec = _kitti_decoder(dev, seed=4)
    base = [f.to(dev) for f in kitti_feats(2, 64, 96, seed=4)]
    with torch.no_grad():
        dec.bind_inputs(base, pointer_sets=0)     # the copy route alone (the recurring-address route has its own test below)
        n0 = dec.capture_count
        assert n0 >= 1
        for step, scale in enumerate((1.0, 0.6, 1.7, 0.6)):
            fresh = [f * scale for f in base]                       # new storage every call
            out = {k: v.clone() for k, v in dec(fresh).items()}
            assert dec.capture_count == n0, "re-captured at step %d" % step
            dec_e = _kitti_decoder(dev, seed=4)
            ref = dec_e(fresh)
            for k in ref:
                assert_close(out[k], ref[k], 2e-6, "bound replay " + key_str(k))
        # the buffers themselves (an encoder writing in place): no copy, still no capture
        for dst, src in zip(dec.static_inputs, base):
            dst.copy_(src * 0.3)
        out = dec(dec.static_inputs)
        assert dec.capture_count == n0
        ref = _kitti_decoder(dev, seed=4)([f * 0.3 for f in base])
        for k in ref:
            assert_close(out[k], ref[k], 2e-6, "in-place bound replay " + key_str(k))
        # other shapes fall back to the ordinary keyed path
        small = [f[:1].contiguous() for f in base]
        out = dec(small)
        assert_close(out[("disp", 0)], _kitti_decoder(dev, seed=4)(small)[("disp", 0)], 2e-6, "fallback")


def test_bound_static_inputs_zero_copy_routes(dev):
    """Round 6 (trainer.py:240-241 hands the decoder fresh encoder outputs every step): the two hand-overs that
    reach the captured launches WITHOUT the 167.7 MB copy.  (a) Tensors that come back at recurring device addresses -- what a
    caching allocator in steady state returns -- get ONE capture per address set on their second sighting and are then replayed
    in place; the captures are bounded (`pointer_sets`), a one-off address set never captures, and new values written at the
    same addresses flow through.  (b) adopt=True: the caller's own tensors become the graph's input buffers
    (`decoder.input_buffers()`), an encoder writes into them, no copy and no capture ever again."""
    ref_dec = _kitti_decoder(dev, seed=4)
    base = [f.to(dev) for f in kitti_feats(2, 64, 96, seed=4)]

    def check(out, feats, what):
        ref = ref_dec(feats)
        for k in ref:
            assert_close(out[k], ref[k], 2e-6, what + " " + key_str(k))

    with torch.no_grad():
        # (a) recurring addresses
        dec = _kitti_decoder(dev, seed=4)
        dec.bind_inputs(base, pointer_sets=2)
        n0 = dec.capture_count
        sets = [[f.clone() for f in base] for _ in range(3)]          # three address sets that keep coming back
        for step in range(9):
            cur = sets[step % 3]
            for f, b in zip(cur, base):
                f.copy_(b * (0.5 + 0.25 * step))                         # new values at old addresses
            out = {k: v.clone() for k, v in dec(cur).items()}
            check(out, cur, "recurring set, step %d" % step)
        assert dec.capture_count == n0 + 2, "one capture per recurring address set, at most pointer_sets of them (%d -> %d)" % (n0, dec.capture_count)
        r = dict(dec.static_route)
        # first sightings (3) copy; sets 0 and 1 capture at their second sighting and replay in place from then on; set 2 keeps copying
        assert r["copy"] == 3 + 2 and r["pointer_replay"] == 4, r
        once = [f * 1.25 for f in base]                                  # an address set seen once: the copy route, no capture
        out = {k: v.clone() for k, v in dec(once).items()}
        check(out, once, "one-off set")
        assert dec.capture_count == n0 + 2
        for g in (dec._graphs._entries.values()):                        # the pointer-set captures keep no input tensor alive
            assert g[2] is None or all(a is b for a, b in zip(g[2], dec.static_inputs))

        # (b) adopted buffers
        dec = _kitti_decoder(dev, seed=4)
        mine = [f.clone() for f in base]
        dec.bind_inputs(mine, adopt=True)
        n0 = dec.capture_count
        assert all(a is b for a, b in zip(dec.input_buffers(), mine))
        for scale in (0.3, 1.9):
            for dst, src in zip(dec.input_buffers(), base):
                torch.mul(src, scale, out=dst)                           # "the encoder's last operator" writes in place
            out = dec(mine)
            check(out, [f * scale for f in base], "adopted buffers x%.1f" % scale)
        assert dec.capture_count == n0 and dec.static_route["copy"] == 0 and dec.static_route["buffers"] == 3
        with pytest.raises(ValueError):
            dec.bind_inputs([f[:, :, ::2] for f in base], adopt=True)   # strided views cannot be adopted


def test_eager_context_keeps_the_captured_graphs(dev):
    """decoder.eager() (round 5; bench.py's per-kernel pass between capture and the timed replays): forwards inside the context are
    eager launches, the captured graphs survive it -- no second capture afterwards, same maps on every path."""
    dec = _kitti_decoder(dev, seed=6)
    feats = [f.to(dev) for f in kitti_feats(2, 64, 96, seed=6)]
    with torch.no_grad():
        ref = {k: v.clone() for k, v in dec(feats).items()}
        dec.enable_graph(True)
        dec(feats)
        n0 = dec.capture_count
        assert n0 >= 1
        with dec.eager():
            out_e = {k: v.clone() for k, v in dec(feats).items()}
            assert dec.capture_count == n0
        out_g = dec(feats)
        assert dec.capture_count == n0, "the eager context dropped the captured graphs"
        for k in ref:
            assert_close(out_e[k], ref[k], 2e-6, "eager context " + key_str(k))
            assert_close(out_g[k], ref[k], 2e-6, "replay after the eager context " + key_str(k))


@pytest.mark.parametrize("two_streams", [False, True])
def test_kitti_dense_decoder_graph_modes_repeatable_in_place(dev, two_streams):
    """Graph replay (one graph / trunk + heads as graph segments on two streams): the inputs are live buffers -- new
    values written IN PLACE must flow through every segment -- and back-to-back replays must not race (every replay
    of the same input gives the same bits, consumers on the caller's stream see finished outputs)."""
    dec = _kitti_decoder(dev, seed=5)
    dec.two_stream_graphs = two_streams
    base = [f.to(dev) for f in kitti_feats(2, 64, 96, seed=5)]
    feats = [f.clone() for f in base]
    with torch.no_grad():
        ref1 = {k: v.clone() for k, v in dec(feats).items()}
        ref2 = {k: v.clone() for k, v in dec([f * 0.7 for f in base]).items()}
        dec.enable_graph(True)
        for rep in range(4):
            for scale, ref in ((1.0, ref1), (0.7, ref2)):
                for f, b in zip(feats, base):
                    f.copy_(b * scale)
                out = dec(feats)
                got = {k: v.clone() for k, v in out.items()}       # consumer on the caller's stream
                for k in ref:
                    assert_close(got[k], ref[k], 2e-6, "replay %d scale %.1f %s" % (rep, scale, key_str(k)))
        dec.enable_graph(False)


@pytest.mark.parametrize("C,H,W", [(32, 12, 40), (64, 9, 28), (128, 6, 20), (256, 12, 40), (32, 5, 7), (32, 10, 84),
                                   (64, 48, 160), (32, 2, 2)])
def test_fused_head_level_vs_oracle(dev, C, H, W):
    """wmd_head_level_fwd (C = 32: one launch -- head_stream_kernel, which takes every plain inference launch at this width
    unless it is switched off, head_level_kernel then) and wmd_head_fused_fwd + wmd_head_shiftsum_fwd (C = 64, 128, 256)
    == Conv1x1 -> LeakyReLU -> Conv3x3(refl) -> sigmoid combine -> IDWT; maps with overhang in both directions.  The launch
    profile must name the kernels of that route."""
    from wavelet_monodepth_amd import _lib, ops
    B, s = 2, 2
    x = t(synth.normal((B, C, H, W), "fx", 6))
    yl = t(synth.normal((B, 1, H, W), "fyl", 6)) * 2 + 4
    hp = [t(a) for a in synth.conv_params("f1p", C, C, 1, 6)] + [t(a) for a in synth.conv_params("f3p", 3, C, 3, 6)]
    hn = [t(a) for a in synth.conv_params("f1n", C, C, 1, 6)] + [t(a) for a in synth.conv_params("f3n", 3, C, 3, 6)]
    lk = lambda v: torch.nn.functional.leaky_relu(v, 0.1)
    sp = torch.sigmoid(R.conv3x3(lk(R.conv1x1(x, hp[0], hp[1])), hp[2], hp[3], "reflect"))
    sn = torch.sigmoid(R.conv3x3(lk(R.conv1x1(x, hn[0], hn[1])), hn[2], hn[3], "reflect"))
    yh_ref = (2 ** (s - 1) * sp - 2 ** (s - 1) * sn).unsqueeze(1)
    out_ref = R.haar_idwt(yl, yh_ref)
    g = lambda v: v.to(dev)
    _lib.profile_begin()
    yh, out, disp = ops.head_fused_level_nograd(g(x), [g(v) for v in hp], [g(v) for v in hn], scale=2.0 ** (s - 1), yl=g(yl),
                                                disp_scale=1.0 / 2 ** (s - 1), clamp01=True)
    recs = _lib.profile_end()
    ran = [r["kernel"] for r in recs if not r["kernel"].startswith("conv_pack")]
    if C == 32:
        if "WMD_HEAD_STREAM_MIN_PIXELS" not in os.environ:
            assert ran == ["head_stream_kernel" if os.environ.get("WMD_HEAD_STREAM", "1") != "0" else "head_level_kernel"], recs
    else:
        first = "head_chain_kernel" if os.environ.get("WMD_HEAD_CHAIN", "1") != "0" else "conv_fwd_kernel<fused head>"
        assert ran == [first, "head_shiftsum_kernel"], recs
    assert float((yh.cpu() - yh_ref).abs().max()) < 4e-6          # differences of sigmoids: absolute tolerance
    assert_close(out, out_ref, 2e-6, "idwt")
    assert_close(disp, torch.clamp(out_ref / 2 ** (s - 1), 0, 1), 2e-6, "disp")


@pytest.mark.parametrize("B,H,W", [(2, 3, 5), (1, 5, 7)])
def test_low_pass_chain_beside_the_fuse_form_vs_oracle(dev, B, H, W):
    """C = 256 on planes that are not a multiple of 4 pixels: the chained kernel declines the level, so wmd_head_fused_fwd runs the
    +- heads AND the low-pass chain (a launch of its own, planes 54..62 of the 81-plane buffer) on the FUSE instantiations of
    conv_fwd_kernel; the shift-sum completes both.  Every output against the oracle, the low-pass plane against the oracle's own
    chain scale_ll * sigmoid(conv3x3(leaky(conv1x1)))."""
    from wavelet_monodepth_amd import ops
    C, s, scale_ll = 256, 4, 16.0
    x = t(synth.normal((B, C, H, W), "lx", 41))
    hp = [t(a) for a in synth.conv_params("l1p", C, C, 1, 41)] + [t(a) for a in synth.conv_params("l3p", 3, C, 3, 41)]
    hn = [t(a) for a in synth.conv_params("l1n", C, C, 1, 41)] + [t(a) for a in synth.conv_params("l3n", 3, C, 3, 41)]
    hl = [t(a) for a in synth.conv_params("l1l", C // 4, C, 1, 41)] + [t(a) for a in synth.conv_params("l3l", 1, C // 4, 3, 41)]
    lk = lambda v: torch.nn.functional.leaky_relu(v, 0.1)
    sp = torch.sigmoid(R.conv3x3(lk(R.conv1x1(x, hp[0], hp[1])), hp[2], hp[3], "reflect"))
    sn = torch.sigmoid(R.conv3x3(lk(R.conv1x1(x, hn[0], hn[1])), hn[2], hn[3], "reflect"))
    yh_ref = (2 ** (s - 1) * sp - 2 ** (s - 1) * sn).unsqueeze(1)
    yl_ref = scale_ll * torch.sigmoid(R.conv3x3(lk(R.conv1x1(x, hl[0], hl[1])), hl[2], hl[3], "reflect"))
    out_ref = R.haar_idwt(yl_ref, yh_ref)
    g = lambda v: v.to(dev)
    yh, out, disp, yl_ll = ops.head_fused_level_nograd(g(x), [g(v) for v in hp], [g(v) for v in hn], scale=2.0 ** (s - 1), yl=None,
                                                       disp_scale=1.0 / 2 ** (s - 1), clamp01=True, head_ll=[g(v) for v in hl], scale_ll=scale_ll)
    assert float((yh.cpu() - yh_ref).abs().max()) < 4e-6          # differences of sigmoids: absolute tolerance
    assert_close(out, out_ref, 2e-6, "idwt")
    assert_close(disp, torch.clamp(out_ref / 2 ** (s - 1), 0, 1), 2e-6, "disp")
    assert_close(yl_ll, yl_ref, 2e-6, "low-pass head")


@pytest.mark.parametrize("B,H,W", [(2, 160, 320), (3, 131, 270), (1, 322, 320), (7, 96, 160)])
def test_streaming_head_level_vs_oracle(dev, B, H, W):
    """Round 6: head_stream_kernel (wmd_head_stream.hip) takes wmd_head_level_fwd's plain inference launches at every size
    (WMD_HEAD_STREAM_MIN_PIXELS defaults to 0; the small maps are in test_gpu_head_fwd.py), here at 100 000 pixels and more
    (strip segments of 32 columns streamed through a ring of tap-partial planes; the GEMM waves' LDS traffic and
    wait counts are hand-written) -- same contract as the tile kernel: Conv1x1 -> LeakyReLU -> Conv3x3(refl) -> sigmoid combine
    -> IDWT -> clamp.  Whole strips, ragged last strips / segments (270 = 8 x 32 + 14 columns, 131 rows), one frame taller than
    wide, several units per block; every output against the oracle, and the launch must really be the streaming kernel."""
    from wavelet_monodepth_amd import _lib, ops
    C, s = 32, 1
    x = t(synth.normal((B, C, H, W), "sx", 16))
    yl = t(synth.normal((B, 1, H, W), "syl", 16)) * 2 + 4
    hp = [t(a) for a in synth.conv_params("s1p", C, C, 1, 16)] + [t(a) for a in synth.conv_params("s3p", 3, C, 3, 16)]
    hn = [t(a) for a in synth.conv_params("s1n", C, C, 1, 16)] + [t(a) for a in synth.conv_params("s3n", 3, C, 3, 16)]
    lk = lambda v: torch.nn.functional.leaky_relu(v, 0.1)
    sp = torch.sigmoid(R.conv3x3(lk(R.conv1x1(x, hp[0], hp[1])), hp[2], hp[3], "reflect"))
    sn = torch.sigmoid(R.conv3x3(lk(R.conv1x1(x, hn[0], hn[1])), hn[2], hn[3], "reflect"))
    yh_ref = (2 ** (s - 1) * sp - 2 ** (s - 1) * sn).unsqueeze(1)
    out_ref = R.haar_idwt(yl, yh_ref)
    g = lambda v: v.to(dev)
    _lib.profile_begin()
    yh, out, disp = ops.head_fused_level_nograd(g(x), [g(v) for v in hp], [g(v) for v in hn], scale=2.0 ** (s - 1), yl=g(yl),
                                                disp_scale=1.0 / 2 ** (s - 1), clamp01=True)
    recs = _lib.profile_end()
    if os.environ.get("WMD_HEAD_STREAM", "1") != "0" and "WMD_HEAD_STREAM_MIN_PIXELS" not in os.environ:
        assert [r["kernel"] for r in recs if not r["kernel"].startswith("conv_pack")] == ["head_stream_kernel"], recs
    assert float((yh.cpu() - yh_ref).abs().max()) < 4e-6          # differences of sigmoids: absolute tolerance
    assert_close(out, out_ref, 2e-6, "idwt")
    assert_close(disp, torch.clamp(out_ref / 2 ** (s - 1), 0, 1), 2e-6, "disp")
    # without the synthesis (yl = None): yh alone
    yh2, out2, disp2 = ops.head_fused_level_nograd(g(x), [g(v) for v in hp], [g(v) for v in hn], scale=2.0 ** (s - 1))
    assert out2 is None and disp2 is None and torch.equal(yh2, yh)


def test_merged_first_stage_of_levels_4_to_2_equals_the_per_level_launches(dev):
    """Round 6: wmd_head_fused_multi_fwd runs the chained GEMMs of levels 4 / 3 / 2 as block ranges of ONE launch (the dense decoder
    postpones them until upconv(2,1) is done: alone none of these levels fills 256 CUs).  Same per-pixel arithmetic: every
    tap-partial plane bit-identical to the per-level launches (the C = 256 level runs as 16-pixel blocks there, 32 / 48 here), with
    and without the low-pass head, ragged plane sizes, and a level the merged launch cannot take (odd plane) falling back."""
    from wavelet_monodepth_amd import ops
    g = lambda v: v.to(dev)
    for B, (h4, w4), with_ll in ((2, (6, 20), True), (3, (5, 12), True), (1, (12, 40), False)):
        levels = []
        for k, C in enumerate((256, 128, 64)):
            H, W = h4 << k, w4 << k
            x = g(t(synth.normal((B, C, H, W), "mx%d" % k, 31)))
            hp = [g(t(a)) for a in synth.conv_params("m1p%d" % k, C, C, 1, 31)] + [g(t(a)) for a in synth.conv_params("m3p%d" % k, 3, C, 3, 31)]
            hn = [g(t(a)) for a in synth.conv_params("m1n%d" % k, C, C, 1, 31)] + [g(t(a)) for a in synth.conv_params("m3n%d" % k, 3, C, 3, 31)]
            hl = None
            if C == 256 and with_ll:
                hl = [g(t(a)) for a in synth.conv_params("m1l", C // 4, C, 1, 31)] + [g(t(a)) for a in synth.conv_params("m3l", 1, C // 4, 3, 31)]
            levels.append((x, hp, hn, hl))
        merged = ops.head_fused_gemm_multi_nograd(levels)
        for (x, hp, hn, hl), m in zip(levels, merged):
            one = ops.head_fused_gemm_nograd(x, hp, hn, hl)
            used = 63 if hl is not None else 54          # (planes 63..80 of the 81-plane buffer are never written)
            assert m["t"].shape == one["t"].shape and torch.equal(m["t"][:, :used], one["t"][:, :used]), "C=%d" % x.shape[1]
        # completions from the merged items == the two-launch level
        yl = None
        for k, ((x, hp, hn, hl), m) in enumerate(zip(levels, merged)):
            s = 4 - k
            if hl is None and yl is None:
                yl = g(t(synth.normal((B, 1, x.shape[2], x.shape[3]), "myl", 31)))
            ref = ops.head_fused_level_nograd(x, hp, hn, scale=2.0 ** (s - 1), yl=None if hl is not None else yl, disp_scale=1.0 / 2 ** (s - 1),
                                              clamp01=True, head_ll=hl, scale_ll=16.0)
            yh, out, disp, yl_ll = ops.head_shiftsum_item_nograd(m, 2.0 ** (s - 1), 1.0 / 2 ** (s - 1), yl=None if hl is not None else yl, scale_ll=16.0)
            assert torch.equal(yh, ref[0]) and torch.equal(out, ref[1]) and torch.equal(disp, ref[2])
            if hl is not None:
                assert torch.equal(yl_ll, ref[3])
            yl = out
    # a plane that is not a multiple of 4 pixels: the per-level fallback inside the entry point, same contract
    x = g(t(synth.normal((1, 64, 3, 5), "mo", 31)))
    hp = [g(t(a)) for a in synth.conv_params("o1p", 64, 64, 1, 31)] + [g(t(a)) for a in synth.conv_params("o3p", 3, 64, 3, 31)]
    hn = [g(t(a)) for a in synth.conv_params("o1n", 64, 64, 1, 31)] + [g(t(a)) for a in synth.conv_params("o3n", 3, 64, 3, 31)]
    both = ops.head_fused_gemm_multi_nograd([(x, hp, hn, None), (x, hp, hn, None)])
    assert torch.equal(both[0]["t"], ops.head_fused_gemm_nograd(x, hp, hn)["t"]) and torch.equal(both[0]["t"], both[1]["t"])


def test_dense_decoder_with_postponed_heads_equals_the_level_by_level_forward(dev):
    """The dense KITTI decoder's inference forward postpones the first stage of levels 4..2 (one merged launch) at batches beyond the
    chained-completion size: every output bit-identical to the level-by-level forward (fuse path forced per level)."""
    from wavelet_monodepth_amd import ops
    dec = _kitti_decoder(dev, seed=8)
    feats = [f.to(dev) for f in kitti_feats(6, 96, 160, seed=8)]      # level 2: 6 x 24 x 40 = 5760 pixels (x 6 frames > the chained-completion size?)
    with torch.no_grad():
        old = ops._SHIFTSUM_CHAIN_MAX_PIXELS
        ops._SHIFTSUM_CHAIN_MAX_PIXELS = 0            # neither decoder takes the chained completion: merged vs per-level first stages
        try:
            out = {k: v.clone() for k, v in dec(feats).items()}
            saved = ops._HEAD_CHAIN_MULTI
            ops._HEAD_CHAIN_MULTI = False
            try:
                ref = dec(feats)
            finally:
                ops._HEAD_CHAIN_MULTI = saved
        finally:
            ops._SHIFTSUM_CHAIN_MAX_PIXELS = old
    assert set(out) == set(ref)
    for k in ref:
        assert torch.equal(out[k], ref[k]), key_str(k)


@pytest.mark.parametrize("B,H1,W1", [(2, 48, 96), (3, 96, 64), (1, 16, 16), (2, 104, 72), (12, 96, 320), (2, 160, 512)])
def test_level1_launch_with_the_coarser_completions_as_a_pyramid(dev, B, H1, W1):
    """Round 6: wmd_head_level_pyramid_fwd -- head_stream_kernel's epilogue waves complete levels 4..2 over every unit's footprint
    (4 x TH/8, 8 x TH/4, 16 x TH/2 pixels under its 32 x TH) before the level's own pipeline starts, handing the low-pass tiles down
    through LDS.  Every output of every level bit-identical to the chained completion launch followed by the level-1 launch;
    whole / ragged strips and segments, one unit per frame, a level 4 of 2 x 2 pixels."""
    from wavelet_monodepth_amd import ops
    g = lambda v: v.to(dev)
    levels = []
    for k, C in enumerate((256, 128, 64)):
        H, W = H1 >> (3 - k), W1 >> (3 - k)
        x = g(t(synth.normal((B, C, H, W), "px%d" % k, 41)))
        hp = [g(t(a)) for a in synth.conv_params("p1p%d" % k, C, C, 1, 41)] + [g(t(a)) for a in synth.conv_params("p3p%d" % k, 3, C, 3, 41)]
        hn = [g(t(a)) for a in synth.conv_params("p1n%d" % k, C, C, 1, 41)] + [g(t(a)) for a in synth.conv_params("p3n%d" % k, 3, C, 3, 41)]
        hl = [g(t(a)) for a in synth.conv_params("p1l", C // 4, C, 1, 41)] + [g(t(a)) for a in synth.conv_params("p3l", 1, C // 4, 3, 41)] if C == 256 else None
        levels.append((x, hp, hn, hl))
    x1 = g(t(synth.normal((B, 32, H1, W1), "px1", 41)))
    hp1 = [g(t(a)) for a in synth.conv_params("q1p", 32, 32, 1, 41)] + [g(t(a)) for a in synth.conv_params("q3p", 3, 32, 3, 41)]
    hn1 = [g(t(a)) for a in synth.conv_params("q1n", 32, 32, 1, 41)] + [g(t(a)) for a in synth.conv_params("q3n", 3, 32, 3, 41)]
    sc, ds = [2.0 ** (k - 1) for k in (4, 3, 2)], [1.0 / 2 ** (k - 1) for k in (4, 3, 2)]
    items = ops.head_fused_gemm_multi_nograd(levels)
    ref = ops.head_shiftsum_chain_nograd(items, sc, ds, scale_ll=16.0)
    ref1 = ops.head_fused_level_nograd(x1, hp1, hn1, scale=1.0, yl=ref[2][1], disp_scale=1.0, clamp01=True)
    items = ops.head_fused_gemm_multi_nograd(levels)
    got, got1 = ops.head_level_pyramid_nograd(x1, hp1, hn1, 1.0, 1.0, items, sc, ds, scale_ll=16.0)
    for k in range(3):
        for a, b in zip(got[k], ref[k]):
            assert (a is None) == (b is None)
            if a is not None:
                assert torch.equal(a, b), "coarse level %d" % k
    for a, b in zip(got1, ref1[:3]):
        assert torch.equal(a, b), "level 1"


@pytest.mark.parametrize("C,H,W", [(256, 12, 40), (64, 9, 28), (128, 5, 7), (32, 6, 10)])
def test_fused_head_level_with_the_low_pass_head_as_third_chain(dev, C, H, W):
    """Coarsest level (depth_decoder.py:104-106,126-136): the LL head C -> C/4 -> 1 rides in the fused launches as a third,
    zero-padded chain; yl = 2^s sigmoid(.), and the synthesis consumes it in the same pass.  (C = 32 takes the one-launch
    kernel for the +/- chains and the stand-alone operators for LL: same contract.)"""
    from wavelet_monodepth_amd import ops
    B, s = 2, 4
    x = t(synth.normal((B, C, H, W), "lx", 7))
    hp = [t(a) for a in synth.conv_params("l1p", C, C, 1, 7)] + [t(a) for a in synth.conv_params("l3p", 3, C, 3, 7)]
    hn = [t(a) for a in synth.conv_params("l1n", C, C, 1, 7)] + [t(a) for a in synth.conv_params("l3n", 3, C, 3, 7)]
    hl = [t(a) for a in synth.conv_params("l1l", C // 4, C, 1, 7)] + [t(a) for a in synth.conv_params("l3l", 1, C // 4, 3, 7)]
    lk = lambda v: torch.nn.functional.leaky_relu(v, 0.1)
    sig = lambda h: torch.sigmoid(R.conv3x3(lk(R.conv1x1(x, h[0], h[1])), h[2], h[3], "reflect"))
    yl_ref = 2.0 ** s * sig(hl)
    yh_ref = (2 ** (s - 1) * sig(hp) - 2 ** (s - 1) * sig(hn)).unsqueeze(1)
    out_ref = R.haar_idwt(yl_ref, yh_ref)
    g = lambda v: v.to(dev)
    yh, out, disp, yl = ops.head_fused_level_nograd(g(x), [g(v) for v in hp], [g(v) for v in hn], scale=2.0 ** (s - 1),
                                                    disp_scale=1.0 / 2 ** (s - 1), clamp01=True,
                                                    head_ll=[g(v) for v in hl], scale_ll=2.0 ** s)
    assert float((yh.cpu() - yh_ref).abs().max()) < 3e-5          # differences of sigmoids x 8: absolute tolerance
    assert_close(yl, yl_ref, 2e-6, "yl")
    assert_close(out, out_ref, 4e-6, "idwt")
    assert_close(disp, torch.clamp(out_ref / 2 ** (s - 1), 0, 1), 4e-6, "disp")


def test_kitti_baseline_decoder_vs_reference_golden(dev):
    from wavelet_monodepth_amd.kitti import DepthDecoder
    gold = load_golden("kitti_baseline_r18_64x64.npz")
    dec = synth.fill_state_dict(DepthDecoder(np.array(R18)), seed=4).to(dev)
    with torch.no_grad():
        out = dec([f.to(dev) for f in kitti_feats(2, 64, 64)])
    assert set(key_str(k) for k in out) == set(gold)
    for k, v in out.items():
        assert_close(v, gold[key_str(k)], NET_TOL, key_str(k))


NYU_ENC = [8, 8, 16, 32, 64]


def _nyu_decoder(dev, enc=NYU_ENC, seed=8):
    from wavelet_monodepth_amd.nyu import DecoderWave
    return synth.fill_state_dict(DecoderWave(enc_features=enc), seed=seed).to(dev)


def test_nyu_dense_decoder_vs_reference_golden(dev):
    from util import nyu_feats
    gold = load_golden("nyu_dense_small_64x96.npz")
    dec = _nyu_decoder(dev)
    with torch.no_grad():
        out = dec([f.to(dev) for f in nyu_feats(2, 64, 96, NYU_ENC)])
    assert set(key_str(k) for k in out) == set(gold)
    for k, v in out.items():
        assert_close(v, gold[key_str(k)], NET_TOL, key_str(k))


def test_nyu_dense_decoder_gradients_vs_reference_golden(dev):
    from util import nyu_feats, sample
    g = load_golden("nyu_dense_small_64x96_grads.npz")
    dec = _nyu_decoder(dev)
    feats = [f.to(dev).requires_grad_(True) for f in nyu_feats(2, 64, 96, NYU_ENC)]
    out = dec(feats)
    loss = sum(out[("disp", s)].mean() for s in range(4))
    loss.backward()
    assert abs(float(loss) - float(g["loss"])) < 1e-5 * max(1.0, abs(float(g["loss"])))
    for k, f in enumerate(feats):
        if "dfeat%d" % k in g:
            assert_close(f.grad, g["dfeat%d" % k], NET_TOL, "dfeat%d" % k)
    for name, p in dec.named_parameters():
        assert_close(sample(p.grad.cpu().numpy()), g["d|" + name], NET_TOL, name)


def test_nyu_depthwise_conv_layer_vs_reference_golden(dev):
    """Conv3x3(is_depthwise=True): wmd_dwconv3x3_fwd/bwd + the bias-free 1x1, outputs and gradients vs the reference layer."""
    from wavelet_monodepth_amd.layers import NyuConv3x3
    g = load_golden("nyu_depthwise_layers.npz")
    for name, cin, cout, h, w, pad in [("reflection_6_5", 6, 5, 5, 7, "reflection"), ("replicate_19_3", 19, 3, 4, 6, "replicate"),
                                       ("zero_9_3", 9, 3, 6, 8, "zero")]:
        m = synth.fill_state_dict(NyuConv3x3(cin, cout, padding=pad, is_depthwise=True), seed=7).to(dev)
        x = t(synth.normal((2, cin, h, w), "dwx_" + name, 7)).to(dev).requires_grad_(True)
        y = m(x)
        (y * y).sum().backward()
        assert_close(y, g["y_" + name], OP_TOL, name)
        assert_close(x.grad, g["dx_" + name], 5e-5, "dx " + name)
        for n, p in m.named_parameters():
            assert_close(p.grad, g["d|%s|%s" % (name, n)], 5e-5, n)


def test_depthwise_fused_upsample_concat_vs_oracle(dev):
    """The depthwise kernel's fused nearest-upsample + concat + pad gather (UpSampleBlock with is_depthwise) and its adjoint."""
    from wavelet_monodepth_amd import ops
    x1 = t(synth.normal((2, 5, 6, 10), "dwu_x1", 3)).requires_grad_(True)
    x2 = t(synth.normal((2, 7, 12, 20), "dwu_x2", 3)).requires_grad_(True)
    w = t(synth.normal((12, 1, 3, 3), "dwu_w", 3)).requires_grad_(True)
    ref = torch.relu(torch.nn.functional.conv2d(R.pad1(torch.cat([R.up2(x1), x2], 1), "reflect"), w, None, groups=12))
    (ref * ref).sum().backward()
    g1, g2, gw = [v.to(dev).detach().requires_grad_(True) for v in (x1, x2, w)]
    y = ops.dwconv3x3_relu(g1, gw, x2=g2, up1=2, pad="reflect")
    (y * y).sum().backward()
    assert_close(y, ref.detach(), OP_TOL, "dw fwd")
    assert_close(g1.grad, x1.grad, 5e-5, "dx1")
    assert_close(g2.grad, x2.grad, 5e-5, "dx2")
    assert_close(gw.grad, w.grad, 5e-5, "dw")


@pytest.mark.parametrize("name", ["decoder", "decoder224", "decoderwave224", "decoder_dw", "decoder224_dw", "decoderwave_dw"])
def test_nyu_decoder_variants_vs_reference_golden(dev, name):
    """Decoder / Decoder224 / DecoderWave224 forward + gradients vs the reference's own modules."""
    from util import nyu_feats, sample
    from wavelet_monodepth_amd import nyu
    g = load_golden("nyu_%s_small_64x96.npz" % name)
    cls, seed, kw = {"decoder": (nyu.Decoder, 21, {}), "decoder224": (nyu.Decoder224, 22, {}), "decoderwave224": (nyu.DecoderWave224, 23, {}),
                     "decoder_dw": (nyu.Decoder, 24, {"is_depthwise": True}), "decoder224_dw": (nyu.Decoder224, 25, {"is_depthwise": True}),
                     "decoderwave_dw": (nyu.DecoderWave, 26, {"dw_waveconv": True, "dw_upconv": True})}[name]
    dec = synth.fill_state_dict(cls(enc_features=NYU_ENC, **kw), seed=seed).to(dev)
    feats = [f.to(dev).requires_grad_(True) for f in nyu_feats(2, 64, 96, NYU_ENC)]
    out = dec(feats)
    assert set(key_str(k) for k in out) == {k for k in g if k.startswith("disp") or k.startswith("wavelets")}
    for k, v in out.items():
        if name == "decoderwave224" and k == ("disp", 1):
            # floor division: values within rounding noise of an integer may land on either side
            diff = (v.detach().cpu() - t(g[key_str(k)])).abs()
            assert float((diff > 1e-4).float().mean()) < 1e-3 and float(diff.max()) <= 1.0 + 1e-4
        else:
            assert_close(v, g[key_str(k)], NET_TOL, key_str(k))
    loss = sum((v * v).mean() for k, v in out.items() if k[0] == "disp" and not (name == "decoderwave224" and k[1] == 1))
    loss.backward()
    assert abs(float(loss) - float(g["loss"])) < 2e-5 * max(1e-3, abs(float(g["loss"])))
    for k, f in enumerate(feats):
        if "dfeat%d" % k in g:
            assert_close(f.grad, g["dfeat%d" % k], NET_TOL, "dfeat%d" % k)
    for n, p in dec.named_parameters():
        assert_close(sample(p.grad.cpu().numpy()), g["d|" + n], NET_TOL, n)


def test_nyu_dense_decoder_densenet161_shapes_vs_oracle(dev):
    """BASELINE config 5 shapes (DenseNet161 features of a 640x480 image), batch 1, with the ragged
    channel counts 2208/1104/552/276/138."""
    from util import nyu_feats
    enc = [96, 96, 192, 384, 2208]
    dec = _nyu_decoder(dev, enc, seed=9)
    feats = nyu_feats(1, 480, 640, enc, seed=9, prefix="nyu_big")
    sd = {k: v.cpu() for k, v in dec.state_dict().items()}
    with torch.no_grad():
        ref = R.nyu_wave_decoder(feats, sd)
        out = dec([f.to(dev) for f in feats])
    for k in ref:
        assert_close(out[k], ref[k], NET_TOL, key_str(k))


@pytest.mark.parametrize("shape,size,ac", [((2, 1, 6, 20), (192, 640), False), ((2, 1, 96, 320), (192, 640), False),
                                           ((1, 1, 30, 40), (240, 320), True), ((2, 3, 5, 7), (11, 9), False),
                                           ((1, 1, 12, 40), (12, 40), True)])
def test_upsample_bilinear_and_disp_to_depth(dev, shape, size, ac):
    """Loss front-end against F.interpolate + disp_to_depth on the CPU, forward and backward."""
    from wavelet_monodepth_amd import ops
    x = t(synth.uniform(shape, "ux", 7, 0.05, 0.95)).requires_grad_(True)
    gy = t(synth.normal((shape[0], shape[1]) + size, "ugy", 7))
    gd = t(synth.normal((shape[0], shape[1]) + size, "ugd", 7))
    ref = torch.nn.functional.interpolate(x, size, mode="bilinear", align_corners=ac)
    _, dref = R.disp_to_depth(ref, 0.1, 100.0)
    ((ref * gy).sum() + (dref * gd).sum() * 1e-3).backward()
    xg = x.detach().to(dev).requires_grad_(True)
    y, d = ops.upsample_bilinear(xg, size, align_corners=ac, depth_range=(0.1, 100.0))
    ((y * gy.to(dev)).sum() + (d * gd.to(dev)).sum() * 1e-3).backward()
    assert_close(y, ref, 2e-6, "bilinear")
    assert_close(d, dref, 1e-5, "depth")
    assert_close(xg.grad, x.grad, 2e-5, "dx")
    y2 = ops.upsample_bilinear(xg.detach(), size, align_corners=ac)
    assert torch.equal(y2, y.detach())


def test_nyu_model_forward_is_encoder_then_decoder(dev):
    """NYUv2/model.py:66-71: Model(opts)(x, threshold) == decoder(encoder(x)[, threshold]) for the dense and the sparse
    decoder; the decoder half runs on the HIP kernels (checked against the CPU oracle on the same features)."""
    from types import SimpleNamespace as NS
    from wavelet_monodepth_amd import nyu
    torch.manual_seed(3)
    base = dict(encoder_type="resnet", num_layers=18, pretrained_encoder=False, normalize_input=False, use_wavelets=True,
                use_224=False, dw_waveconv=False, dw_upconv=False)
    x = torch.rand(1, 3, 64, 96, device=dev)
    for sparse in (False, True):
        m = nyu.Model(NS(use_sparse=sparse, **base)).to(dev).eval()
        synth.fill_state_dict(m.decoder, seed=8)
        with torch.no_grad():
            m.encoder(x)                       # MIOpen settles on its algorithms in the first call
            out = m(x, 0.1)
            feats = m.encoder(x)
            want = m.decoder(feats, 0.1) if sparse else m.decoder(feats)
            sd = {k: v.cpu() for k, v in m.decoder.state_dict().items()}
            cf = [f.cpu() for f in feats]
            ref = R.nyu_sparse_wave_decoder(cf, sd, 0.1) if sparse else R.nyu_wave_decoder(cf, sd)
        assert set(out) == set(want)
        for k, v in want.items():
            if torch.is_tensor(v) and v.dtype.is_floating_point:
                assert_close(out[k], v, 1e-5, key_str(k))      # the PyTorch encoder is not bit-reproducible run to run
            elif not torch.is_tensor(v) and not sparse:
                assert out[k] == v
        if not sparse:                                          # (a threshold pixel may flip between CPU and GPU features)
            for s in range(4):
                assert_close(out[("disp", s)].cpu(), ref[("disp", s)], 1e-4, "disp%d vs oracle" % s)
