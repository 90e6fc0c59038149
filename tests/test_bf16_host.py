"""CPU: the bf16 trunk-precision entry points (include/wmd.h, wmd_conv_bf16_*) -- packed-image size, every refusal that
happens before a launch, the decoder's set_precision surface, and the CPU reference of the numerics contract
(tests/bf16_ref.py) against the fp32 oracle."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import decoder_ref as R
from wavelet_monodepth_amd import _lib, synth
from bf16_ref import kitti_wave_decoder_bf16
from util import R18, R50, assert_close, assert_depth_close, key_str, kitti_feats

DEC = [16, 32, 64, 128, 256]


def trunk_layers(enc, B, H, W):
    """The eight trunk layers of a KITTI wavelet decoder at image size H x W: (B, H, W, C1, up1, C2, Cout) per layer."""
    out = []
    h, w, cx = H // 32, W // 32, enc[4]
    for i in range(4, 0, -1):
        out.append((B, h, w, cx, 1, 0, DEC[i]))
        out.append((B, 2 * h, 2 * w, DEC[i], 2, enc[i - 1], DEC[i]))
        h, w, cx = 2 * h, 2 * w, DEC[i]
    return out


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from wavelet_monodepth_amd import build
        build.build()
    return _lib.lib()


def conv_args(B=2, H=12, W=40, C1=32, up1=1, C2=16, Cout=32, ksize=3, pad_mode=1, **kw):
    a = _lib.ConvArgs(B=B, H=H, W=W, C1=C1, up1=up1, C2=C2, Cout=Cout, ksize=ksize, pad_mode=pad_mode, act=1, slope=0.0,
                      x1=1, x2=1 if C2 else None, wp=1, bias=1, y=1, workspace=None, workspace_floats=0, tune_cfg=0, tune_ksplit=0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_packed_weight_bytes_is_the_documented_formula(lib):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wmd.h")).read()
    assert "wmd_conv_bf16_packed_weight_bytes = 2 * 9 * Cout * Cin * (terms == 3 ? 2 : 1)" in header
    for enc in (R18, R50):
        for (_, _, _, c1, _, c2, cout) in trunk_layers(enc, 1, 192, 640):
            for terms in (1, 3):
                assert lib.wmd_conv_bf16_packed_weight_bytes(cout, c1 + c2, terms) == 2 * 9 * cout * (c1 + c2) * (2 if terms == 3 else 1)
    assert lib.wmd_conv_bf16_packed_weight_bytes(32, 24, 3) == 0
    assert lib.wmd_conv_bf16_packed_weight_bytes(16, 32, 3) == 0
    assert lib.wmd_conv_bf16_packed_weight_bytes(32, 32, 2) == 0
    assert lib.wmd_conv_bf16_num_configs() >= 1
    names = [lib.wmd_conv_bf16_config_name(i) for i in range(lib.wmd_conv_bf16_num_configs())]
    assert all(n.startswith(b"conv_bf16_kernel<") for n in names) and len(set(names)) == len(names)
    assert lib.wmd_conv_bf16_config_name(len(names)) is None


def test_refusals_before_any_launch(lib):
    def refused(a, terms, status, word, unsupported=None):
        assert lib.wmd_conv_bf16_fwd(C.byref(a), terms, None) == status, word
        assert word.encode() in lib.wmd_last_error(), (word, lib.wmd_last_error())
        if status == -3:
            assert lib.wmd_conv_bf16_supported(C.byref(a), terms) == 0, word

    refused(conv_args(), 2, -1, "terms")
    refused(conv_args(x1=None), 3, -1, "null")
    refused(conv_args(ksize=1), 3, -3, "ksize")
    refused(conv_args(C1=24), 3, -3, "C1=24")
    refused(conv_args(out_mask=1), 1, -3, "out_mask")
    refused(conv_args(gate=1), 1, -3, "gate")
    refused(conv_args(pad_mode=2), 3, -3, "replicate")
    refused(conv_args(W=1), 3, -2, "reflect")
    refused(conv_args(tune_cfg=lib.wmd_conv_bf16_num_configs() + 1), 3, -3, "tune_cfg")
    # a forced split with its workspace one float short
    a = conv_args(tune_ksplit=3)
    n = lib.wmd_conv_bf16_workspace_floats(C.byref(a), 3)
    assert n == 3 * 2 * 32 * 12 * 40
    a.workspace, a.workspace_floats = 1, n - 1
    refused(a, 3, -5, "workspace")
    assert lib.wmd_conv_bf16_supported(C.byref(a), 3) == 1
    for enc in (R18, R50):
        for (B, H, W, c1, up, c2, cout) in trunk_layers(enc, 1, 192, 640):
            for terms in (1, 3):
                assert lib.wmd_conv_bf16_supported(C.byref(conv_args(B=B, H=H, W=W, C1=c1, up1=up, C2=c2, Cout=cout)), terms) == 1


def test_set_precision_surface_and_cpu_refusal():
    from wavelet_monodepth_amd import ops
    from wavelet_monodepth_amd.kitti import DepthWaveProgressiveDecoder
    dec = DepthWaveProgressiveDecoder(np.array(R18))
    keys = list(dec.state_dict().keys())
    assert dec.trunk_precision == "fp32"
    for mode in ("bf16x3", "bf16", "fp32"):
        assert dec.set_precision(mode) is dec and dec.trunk_precision == mode
    with pytest.raises(ValueError):
        dec.set_precision("fp16")
    assert dec.trunk_precision == "fp32"
    assert list(dec.state_dict().keys()) == keys
    with pytest.raises(_lib.WmdError):
        ops.conv3x3_bf16_nograd(torch.zeros(1, 32, 4, 4), torch.zeros(32, 32, 3, 3))


@pytest.mark.parametrize("size", [(64, 64), (64, 96)])
def test_three_term_reference_is_inside_the_parity_contract(size):
    """The reference alone (also the record of the figures in DESIGN.md): bf16x3 against the fp32 oracle, R18 B=2."""
    from wavelet_monodepth_amd.kitti import DepthWaveProgressiveDecoder
    sd = synth.fill_state_dict(DepthWaveProgressiveDecoder(np.array(R18)), seed=1).state_dict()
    feats = kitti_feats(2, *size)
    with torch.no_grad():
        ref = R.kitti_wave_decoder(feats, sd)
        got = kitti_wave_decoder_bf16(feats, sd, 3)
    assert set(ref) == set(got)
    for k, v in ref.items():
        assert_close(got[k], v, 1e-4, key_str(k))
    for s in range(4):
        assert_depth_close(got[("disp", s)], ref[("disp", s)], 1e-4, "depth %d" % s)
