"""GPU: the three-pass Winograd F(4x4,3x3) convolution (wmd_conv_wino44_fwd) against the oracle's conv3x3 + activation at 5e-5
(the project's figure for a forced Winograd configuration), its determinism, and the route that decides which layers run it."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from oracle import decoder_ref as R
from wavelet_monodepth_amd import _lib, layers, ops, tuner
from util import assert_close, max_rel

pytestmark = pytest.mark.gpu
TOL = 5e-5


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _operands(B, C1, C2, cout, H, W, up, seed):
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn(B, C1, H // up, W // up, generator=g)
    x2 = torch.randn(B, C2, H, W, generator=g) if C2 else None
    w = torch.randn(cout, C1 + C2, 3, 3, generator=g) * (2.0 / (9 * (C1 + C2))) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    return x1, x2, w, b


def _oracle(x1, x2, w, b, up, pad, act, slope=0.0):
    x = R.up2(x1) if up == 2 else x1
    if x2 is not None:
        x = torch.cat([x, x2], 1)
    y = R.conv3x3(x.double(), w.double(), b.double(), pad)
    return {"none": lambda v: v, "elu": F.elu, "leaky": lambda v: F.leaky_relu(v, slope)}[act](y)


def _forced(dev, x1, x2, w, b, up, pad, act, slope=0.0):
    with torch.no_grad():
        return ops.conv3x3_wino44_nograd(x1.to(dev), w.to(dev), b.to(dev), x2=None if x2 is None else x2.to(dev), up1=up, pad=pad,
                                         act=act, slope=slope)


@pytest.mark.parametrize("pad", ["reflect", "zero", "replicate"])
@pytest.mark.parametrize("B,C,cout,H,W", [(2, 16, 40, 8, 12),     # exact tiles, ragged Cout
                                          (2, 16, 32, 6, 10),     # H and W both 2 mod 4
                                          (1, 24, 8, 5, 7)])      # odd sizes
def test_pure_layers_vs_oracle(dev, B, C, cout, H, W, pad):
    x1, _, w, b = _operands(B, C, 0, cout, H, W, 1, 1)
    assert_close(_forced(dev, x1, None, w, b, 1, pad, "elu"), _oracle(x1, None, w, b, 1, pad, "elu"), TOL, "pure %s" % pad)


@pytest.mark.parametrize("act", ["none", "elu", "leaky"])
@pytest.mark.parametrize("pad", ["reflect", "zero"])
@pytest.mark.parametrize("B,C1,C2,cout,H,W", [(2, 16, 24, 32, 12, 20),
                                              (2, 16, 24, 19, 6, 10),
                                              (3, 8, 8, 32, 12, 20)])     # 45 tiles: not a multiple of 32
def test_up_and_skip_layers_vs_oracle(dev, B, C1, C2, cout, H, W, pad, act):
    x1, x2, w, b = _operands(B, C1, C2, cout, H, W, 2, 2)
    got = _forced(dev, x1, x2, w, b, 2, pad, act, 0.1)
    assert_close(got, _oracle(x1, x2, w, b, 2, pad, act, 0.1), TOL, "up+skip %s %s" % (pad, act))


def test_upsampled_layer_without_a_skip_tensor_vs_oracle(dev):
    x1, _, w, b = _operands(2, 16, 0, 32, 12, 20, 2, 3)
    assert_close(_forced(dev, x1, None, w, b, 2, "reflect", "elu"), _oracle(x1, None, w, b, 2, "reflect", "elu"), TOL)


@pytest.mark.parametrize("C1,C2,up", [(512, 0, 1), (256, 256, 2)])
def test_long_reduction_vs_oracle(dev, C1, C2, up):
    x1, x2, w, b = _operands(1, C1, C2, 32, 8, 8, up, 4)
    assert_close(_forced(dev, x1, x2, w, b, up, "reflect", "elu"), _oracle(x1, x2, w, b, up, "reflect", "elu"), TOL)


@pytest.mark.parametrize("up,C2", [(2, 24), (1, 0)])
def test_two_launches_over_a_nan_workspace_are_bit_identical_and_write_everything(dev, up, C2):
    B, C1, cout, H, W = 3, 16, 19, 10, 14
    x1, x2, w, b = [None if v is None else v.to(dev) for v in _operands(B, C1, C2, cout, H, W, up, 5)]
    l = _lib.lib()
    wp = ops.pack_weights_wino44(w, C1, up)
    a = ops._conv_args(B, H, W, C1, up, C2, cout, 3, "reflect", "elu", 0.0)
    n = l.wmd_conv_wino44_workspace_floats(C.byref(a))
    outs = []
    for _ in range(2):
        ws = torch.full((n,), float("nan"), device=dev)
        y = torch.full((B, cout, H, W), float("nan"), device=dev)
        a.x1, a.x2, a.wp, a.bias, a.y = x1.data_ptr(), None if x2 is None else x2.data_ptr(), wp.data_ptr(), b.data_ptr(), y.data_ptr()
        a.workspace, a.workspace_floats = ws.data_ptr(), n
        _lib.check(l.wmd_conv_wino44_fwd(C.byref(a), torch.cuda.current_stream().cuda_stream), "wmd_conv_wino44_fwd")
        torch.cuda.synchronize()
        outs.append(y)
    assert not torch.isnan(outs[0]).any()
    assert torch.equal(outs[0], outs[1])


@pytest.fixture
def fresh_route(monkeypatch):
    monkeypatch.setattr(ops, "_wino44_route", {})
    monkeypatch.setattr(tuner, "_cache", dict(tuner._cache))
    return monkeypatch


def _layer(dev, x1, x2, w, b, up):
    m = layers.Conv3x3(w.shape[1], w.shape[0]).to(dev)
    with torch.no_grad():
        m.conv.weight.copy_(w)
        m.conv.bias.copy_(b)
        x1d, x2d = x1.to(dev), None if x2 is None else x2.to(dev)
        return m, m(x1d, skip=x2d, up=up, act="elu", routed=True), ops.conv2d_fused(x1d, m.conv.weight, m.conv.bias, x2=x2d, up1=up, pad="reflect", act="elu")


def test_a_layer_below_256_tiles_takes_todays_path(dev, fresh_route):
    x1, x2, w, b = _operands(2, 16, 24, 32, 24, 40, 2, 6)     # 120 tiles
    fresh_route.setitem(tuner._cache, "route|conv|2|24|40|16|2|24|32|3", ("wino44", 0))   # even a remembered choice is not honoured
    _, y, y_fused = _layer(dev, x1, x2, w, b, 2)
    assert torch.equal(y, y_fused)


def test_the_kill_switch_keeps_todays_path_at_any_size(dev, fresh_route):
    x1, x2, w, b = _operands(6, 16, 24, 32, 24, 40, 2, 7)     # 360 tiles
    fresh_route.setitem(tuner._cache, "route|conv|6|24|40|16|2|24|32|3", ("wino44", 0))
    fresh_route.setattr(ops, "_WINO44", False)
    _, y, y_fused = _layer(dev, x1, x2, w, b, 2)
    assert torch.equal(y, y_fused)


def test_without_a_remembered_choice_a_large_layer_takes_todays_path(dev, fresh_route):
    x1, x2, w, b = _operands(6, 16, 24, 32, 24, 40, 2, 7)
    assert tuner.remembered("route|conv|6|24|40|16|2|24|32|3") is None and ops.wino44_offered(6, 24, 40, 16, 2, 24, 32)
    _, y, y_fused = _layer(dev, x1, x2, w, b, 2)
    assert torch.equal(y, y_fused)


def test_a_choice_that_arrives_after_the_first_forward_is_taken(dev, fresh_route):
    """an absent entry is no choice: the layer runs fused, and the entry that a later preload brings routes it"""
    x1, x2, w, b = _operands(6, 16, 24, 32, 24, 40, 2, 7)
    m, y, y_fused = _layer(dev, x1, x2, w, b, 2)
    assert torch.equal(y, y_fused)
    fresh_route.setitem(tuner._cache, "route|conv|6|24|40|16|2|24|32|3", ("wino44", 0))
    with torch.no_grad():
        y2 = m(x1.to(dev), skip=x2.to(dev), up=2, act="elu", routed=True)
    assert torch.equal(y2, _forced(dev, x1, x2, w, b, 2, "reflect", "elu"))


def test_a_remembered_choice_routes_the_layer_and_holds(dev, fresh_route):
    x1, x2, w, b = _operands(6, 16, 24, 32, 24, 40, 2, 7)
    key = "route|conv|6|24|40|16|2|24|32|3"
    fresh_route.setitem(tuner._cache, key, ("wino44", 0))
    m, y, y_fused = _layer(dev, x1, x2, w, b, 2)
    assert torch.equal(y, _forced(dev, x1, x2, w, b, 2, "reflect", "elu")) and not torch.equal(y, y_fused)
    fresh_route.setitem(tuner._cache, key, ("fused", 0))      # the process keeps its first choice
    with torch.no_grad():
        assert torch.equal(m(x1.to(dev), skip=x2.to(dev), up=2, act="elu", routed=True), y)
        assert torch.equal(m(x1.to(dev), skip=x2.to(dev), up=2, act="elu"), y_fused)      # a caller that does not ask for routes
    with torch.enable_grad():                                   # never under autograd
        xg = x1.to(dev).requires_grad_(True)
        assert torch.equal(m(xg, skip=x2.to(dev), up=2, act="elu", routed=True).detach(), y_fused)


def test_forced_route_on_the_12x40_up_skip_layer(dev, fresh_route, capsys):
    """(12, 256 + 256 -> 256, 12x40): within 5e-5 of the oracle; against today's path the distance is recorded as a multiple k of
    the generic operator tolerance 2e-5, not asserted.  Measured: k = 1.03 (2.07e-5; 2.06e-5 against the oracle, today's
    path 6.5e-7)."""
    x1, x2, w, b = _operands(12, 256, 256, 256, 12, 40, 2, 8)
    fresh_route.setitem(tuner._cache, "route|conv|12|12|40|256|2|256|256|3", ("wino44", 0))
    _, y, y_fused = _layer(dev, x1, x2, w, b, 2)
    ref = _oracle(x1, x2, w, b, 2, "reflect", "elu")
    with capsys.disabled():
        print("\n[wino44] 12x40 up+skip layer: vs oracle %.2e (today's path %.2e), vs today's path %.2e = %.2f x 2e-5"
              % (max_rel(y.cpu().numpy(), ref.numpy()), max_rel(y_fused.cpu().numpy(), ref.numpy()),
                 max_rel(y.cpu().numpy(), y_fused.cpu().numpy()), max_rel(y.cpu().numpy(), y_fused.cpu().numpy()) / 2e-5))
    assert not torch.equal(y, y_fused)
    assert_close(y, ref, TOL, "forced route")


def _r18_decoder(dev, seed):
    import numpy as np
    from wavelet_monodepth_amd import synth
    from wavelet_monodepth_amd.kitti import DepthWaveProgressiveDecoder
    from util import R18
    return synth.fill_state_dict(DepthWaveProgressiveDecoder(np.array(R18)), seed=seed).to(dev)


def test_batch12_graph_decoder_with_the_committed_routes_vs_oracle(dev, fresh_route):
    """What bench.py times, with the committed route file active: the batch-12 640x192 decoder in graph mode runs its 12x40 up+skip
    layer on the F(4x4,3x3) kernels -- whether the cache is preloaded after the decoder's first forward (decoder A) or before it
    (decoder B): same bits --, replays bit for bit, and holds every map of three frames to the oracle at 1e-4.  The same decoder
    in eager mode does not take the route: its batch-12 maps are those of twelve batch-1 forwards
    (test_kitti_dense_decoder_batch12_properties, 1e-6), which the routed layer moves by 1.2e-6."""
    import json
    import os
    from util import ROOT, assert_depth_close, bench_tune_cache_name, key_str, kitti_feats
    key = "route|conv|12|12|40|256|2|256|256|3"
    cache = os.path.join(ROOT, "profiles", bench_tune_cache_name())
    tiles = {k: tuple(v) for k, v in json.load(open(cache)).items()}      # the committed tile choices alone: nothing is tuned here
    fresh_route.setattr(tuner, "_cache", tiles)
    assert not any(k.startswith("route|") for k in tiles)
    feats = [f.to(dev) for f in kitti_feats(12, 192, 640)]
    names = ("wino44_input_kernel", "wino44_gemm_kernel", "wino44_output_kernel")

    def kernels(dec):
        _lib.profile_begin()
        with dec.eager():
            dec(feats)
        return {r["kernel"] for r in _lib.profile_end()}

    with torch.no_grad():
        a = _r18_decoder(dev, 1)
        eager = {k: v.clone() for k, v in a(feats).items()}          # eager mode
        a.enable_graph(True)
        before = {k: v.clone() for k, v in a(feats).items()}         # graph mode, no route known: today's path, and no choice is made
        assert all(torch.equal(before[k], eager[k]) for k in eager) and key not in ops._wino44_route
        assert not set(names) & kernels(a)
        tuner.preload(cache)                                         # ... the route arrives after the first forward
        assert tuner.remembered(key) == ("wino44", 0)
        assert set(names) <= kernels(a) and ops._wino44_route[key] is True
        for _ in range(2):
            out = a(feats)
        first = {k: v.clone() for k, v in out.items()}
        out = a(feats)
        assert all(torch.equal(out[k], first[k]) for k in first), "replay is not repeatable"
        assert not all(torch.equal(first[k], eager[k]) for k in eager), "the routed layer did not run in the replays"
        b = _r18_decoder(dev, 1).enable_graph(True)                  # ... and before it
        assert all(torch.equal(v, first[k]) for k, v in b(feats).items())
        a.enable_graph(False)
        again = a(feats)                                             # eager mode with the route known: still today's path
        assert all(torch.equal(again[k], eager[k]) for k in eager)
    sd = {k: v.detach().cpu() for k, v in a.state_dict().items()}
    for fr in (0, 5, 11):
        ref = R.kitti_wave_decoder([f[fr:fr + 1].cpu() for f in feats], sd)
        assert set(ref) == set(first)
        for k, v in ref.items():
            assert_close(first[k][fr:fr + 1], v, 1e-4, "frame %d %s" % (fr, key_str(k)))
        for s_ in range(4):
            assert_depth_close(first[("disp", s_)][fr:fr + 1], ref[("disp", s_)], 1e-4, "frame %d depth %d" % (fr, s_))
