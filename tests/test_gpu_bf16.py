"""GPU: the opt-in bf16 / split-bf16 trunk precision (wmd_conv_bf16_fwd, DepthWaveProgressiveDecoder.set_precision) against
the CPU reference of its numerics contract (tests/bf16_ref.py) and against the fp32 oracle.

Tolerances: a single operator on GIVEN fp32 operands is held to the project's per-operator figure OP_TOL = 2e-5 (only the
fp32 summation order differs; a dropped cross term shows as ~1e-3); the whole decoder in "bf16x3" to the project's contract
NET_TOL = 1e-4 against the fp32 oracle.  In "bf16" a last-bit difference of a trunk activation flips the bf16 rounding of a few
elements the next layer reads, so two correct implementations differ by a few 1e-4 end to end: that test calibrates itself
on the reference (fp32- against fp64-accumulation of the same rounded operands), see its docstring."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import decoder_ref as R
from wavelet_monodepth_amd import _lib, synth
from bf16_ref import conv_block_bf16, kitti_wave_decoder_bf16
from test_bf16_host import trunk_layers
from util import R18, R50, assert_close, assert_depth_close, key_str, kitti_feats, max_rel, t

pytestmark = pytest.mark.gpu

OP_TOL = 2e-5
NET_TOL = 1e-4
MOBILENET = [32, 24, 32, 64, 1280]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _decoder(dev, chans=R18, seed=1):
    from wavelet_monodepth_amd.kitti import DepthWaveProgressiveDecoder
    return synth.fill_state_dict(DepthWaveProgressiveDecoder(np.array(chans)), seed=seed).to(dev)


def _operands(shape, seed, bias=True):
    B, H, W, c1, up, c2, cout = shape
    tag = "b16_%d_%d_%d_%d_%d_%d_%d" % shape
    x1 = t(synth.normal((B, c1, H // up, W // up), tag + "x1", seed))
    x2 = t(synth.normal((B, c2, H, W), tag + "x2", seed)) if c2 else None
    w = t(synth.normal((cout, c1 + c2, 3, 3), tag + "w", seed)) * float(1.0 / np.sqrt(9.0 * (c1 + c2)))
    b = t(synth.normal((cout,), tag + "b", seed)) * 0.1 if bias else None
    return x1, x2, w, b


def _reference(x1, x2, w, b, up, terms, pad, act, slope):
    x = R.up2(x1) if up == 2 else x1
    if x2 is not None:
        x = torch.cat([x, x2], 1)
    return conv_block_bf16(x, w, b, terms, pad=pad, act=act, slope=slope)


class _Op:
    """wmd_conv_bf16_fwd through ctypes with a forced table entry / split (ops.conv3x3_bf16_nograd lets the tuner choose)."""

    def __init__(self, dev, x1, x2, w, b, up, terms, pad="reflect", act="elu", slope=0.0):
        from wavelet_monodepth_amd import ops
        self.l, self.terms, self.dev = _lib.lib(), terms, dev
        self.keep = [v.to(dev) if v is not None else None for v in (x1, x2, w, b)]
        gx1, gx2, gw, gb = self.keep
        self.wp = ops.pack_weights_bf16(gw, terms)
        B, c1, h, w_ = gx1.shape
        self.shape = (B, w.shape[0], h * up, w_ * up)
        self.a = _lib.ConvArgs(B=B, H=h * up, W=w_ * up, C1=c1, up1=up, C2=0 if gx2 is None else gx2.shape[1], Cout=w.shape[0],
                               ksize=3, pad_mode=_lib.PAD[pad], act=_lib.ACT[act], slope=float(slope), x1=_lib.ptr(gx1),
                               x2=_lib.ptr(gx2), wp=_lib.ptr(self.wp), bias=_lib.ptr(gb), y=1, workspace=None, workspace_floats=0)

    def run(self, cfg=0, ks=0, poison=False):
        """-> (status, y)"""
        a = self.a
        a.tune_cfg, a.tune_ksplit = cfg, ks
        a.workspace, a.workspace_floats = None, 0
        n = self.l.wmd_conv_bf16_workspace_floats(C.byref(a), self.terms)
        ws = None
        if n:
            ws = torch.full((n,), float("nan"), device=self.dev) if poison else torch.empty(n, device=self.dev)
            a.workspace, a.workspace_floats = _lib.ptr(ws), n
        y = torch.full(self.shape, float("nan"), device=self.dev)
        a.y = _lib.ptr(y)
        st = self.l.wmd_conv_bf16_fwd(C.byref(a), self.terms, _lib.current_stream())
        torch.cuda.synchronize()
        return st, y, n


def _check_every_config(dev, shape, terms, pad="reflect", act="elu", slope=0.0, bias=True, seed=3, trunk=False):
    x1, x2, w, b = _operands(shape, seed, bias)
    ref = _reference(x1, x2, w, b, shape[4], terms, pad, act, slope)
    op = _Op(dev, x1, x2, w, b, shape[4], terms, pad, act, slope)
    ncfg = op.l.wmd_conv_bf16_num_configs()
    declines = 0
    for cfg in range(0, ncfg + 1):
        st, y, _ = op.run(cfg)
        name = "library" if cfg == 0 else op.l.wmd_conv_bf16_config_name(cfg - 1).decode()
        if st == -3 and cfg > 0:
            declines += 1
            continue
        assert st == 0, "%s %s terms=%d: status %d (%s)" % (shape, name, terms, st, op.l.wmd_last_error().decode())
        err = max_rel(y.cpu().numpy(), ref.numpy())
        print("conv_bf16 %s terms=%d %s: max_rel %.3e" % (shape, terms, name, err))
        assert err <= OP_TOL, "%s %s terms=%d: max relative error %.3e > %.1e" % (shape, name, terms, err, OP_TOL)
    assert declines <= (1 if trunk else ncfg - 1), "%d table entries declined %s" % (declines, shape)


CONFIG2 = trunk_layers(R18, 2, 192, 640)
R50_1024 = trunk_layers(R50, 1, 320, 1024)


@pytest.mark.parametrize("terms", [1, 3])
@pytest.mark.parametrize("layer", range(8))
def test_trunk_layers_config2_every_table_entry(dev, layer, terms):
    _check_every_config(dev, CONFIG2[layer], terms, trunk=True)


@pytest.mark.parametrize("terms", [1, 3])
@pytest.mark.parametrize("layer", range(8))
def test_trunk_layers_r50_1024x320_every_table_entry(dev, layer, terms):
    _check_every_config(dev, R50_1024[layer], terms, trunk=True)


@pytest.mark.parametrize("terms", [1, 3])
@pytest.mark.parametrize("size,up", [((5, 7), 1), ((13, 27), 1), ((33, 65), 1), ((6, 10), 2), ((34, 66), 2)])
def test_ragged_sizes_pads_and_activations(dev, size, up, terms):
    shape = (2, size[0], size[1], 32, up, 16, 32)
    for pad in ("reflect", "zero"):
        _check_every_config(dev, shape, terms, pad=pad, act="elu")
    _check_every_config(dev, shape, terms, act="none", bias=False)
    _check_every_config(dev, shape, terms, pad="zero", act="leaky", slope=0.1)


@pytest.mark.parametrize("terms", [1, 3])
@pytest.mark.parametrize("shape", [CONFIG2[0], CONFIG2[1], R50_1024[0], R50_1024[1]])
def test_forced_k_splits_match_and_repeat_bit_for_bit(dev, shape, terms):
    x1, x2, w, b = _operands(shape, 5)
    ref = _reference(x1, x2, w, b, shape[4], terms, "reflect", "elu", 0.0)
    op = _Op(dev, x1, x2, w, b, shape[4], terms)
    for ks in (2, 3, 5):
        st, y, n = op.run(0, ks, poison=True)
        assert st == 0 and n == ks * y.numel(), (st, n)
        err = max_rel(y.cpu().numpy(), ref.numpy())
        print("conv_bf16 %s terms=%d ksplit %d: max_rel %.3e" % (shape, terms, ks, err))
        assert err <= OP_TOL, "ksplit %d: %.3e" % (ks, err)
        st2, y2, _ = op.run(0, ks, poison=True)
        assert st2 == 0 and torch.equal(y, y2), "a %d-way split is not bit-repeatable" % ks


# ---- whole decoder ------------------------------------------------------------------------------------------------------------

CASES = {"r18_64x64": (R18, 2, 64, 64, 1), "r18_64x96": (R18, 2, 64, 96, 1), "config2_b2": (R18, 2, 192, 640, 1),
         "r50_96x320": (R50, 1, 96, 320, 2)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (chans, feats, state dict, fp32 oracle outputs)"""
    from wavelet_monodepth_amd.kitti import DepthWaveProgressiveDecoder
    chans, B, H, W, seed = CASES[name]
    sd = {k: v.detach() for k, v in synth.fill_state_dict(DepthWaveProgressiveDecoder(np.array(chans)), seed=seed).state_dict().items()}
    feats = kitti_feats(B, H, W, chans, seed=seed)
    with torch.no_grad():
        return chans, feats, sd, R.kitti_wave_decoder(feats, sd)


def _gpu_forward(dev, name, mode):
    chans, feats, _, _ = _case(name)
    dec = _decoder(dev, chans, CASES[name][4]).set_precision(mode)
    with torch.no_grad():
        out = dec([f.to(dev) for f in feats])
    assert set(dec.trunk_precision_report().values()) == {mode}
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_decoder_bf16x3_is_inside_the_fp32_contract(dev, name):
    _, _, _, ref = _case(name)
    out = _gpu_forward(dev, name, "bf16x3")
    assert set(out) == set(ref)
    worst = max(max_rel(out[k].numpy(), v.numpy()) for k, v in ref.items())
    print("bf16x3 %s: worst plane max_rel vs fp32 oracle %.3e" % (name, worst))
    for k, v in ref.items():
        assert_close(out[k], v, NET_TOL, "%s %s" % (name, key_str(k)))
    for s in range(4):
        assert_depth_close(out[("disp", s)], ref[("disp", s)], NET_TOL, "%s depth %d" % (name, s))


def test_decoder_bf16_against_its_reference_with_self_calibrated_bounds(dev):
    """One-product mode.  Both bounds come from the reference alone, pooled over the planes of all four inputs:
    spread = the difference between fp32- and fp64-accumulation of the SAME rounded operands (two correct implementations:
    rounding flips of the activations the next layer reads), cost = the one-product reference against the fp32 oracle.
    GPU vs one-product reference <= 4 * spread (flips are rare discrete events with a heavy tail), GPU vs fp32 oracle <=
    2 * cost, and cost > 1e-4 so that a mode that silently ran fp32 or three products fails."""
    pooled = lambda a, b: max(max_rel(a[k].numpy(), b[k].numpy()) for k in b)
    spread = cost = got_ref = got_oracle = 0.0
    for name in CASES:
        _, feats, sd, oracle = _case(name)
        with torch.no_grad():
            one = kitti_wave_decoder_bf16(feats, sd, 1)
            one64 = kitti_wave_decoder_bf16(feats, sd, 1, acc64=True)
        out = _gpu_forward(dev, name, "bf16")
        spread, cost = max(spread, pooled(one, one64)), max(cost, pooled(one, oracle))
        got_ref, got_oracle = max(got_ref, pooled(out, one)), max(got_oracle, pooled(out, oracle))
        print("bf16 %s: spread %.3e cost %.3e | GPU vs reference %.3e, vs fp32 oracle %.3e" %
              (name, pooled(one, one64), pooled(one, oracle), pooled(out, one), pooled(out, oracle)))
    print("bf16 pooled: spread %.3e, GPU vs reference %.3e (ratio %.2f); cost %.3e, GPU vs fp32 oracle %.3e" %
          (spread, got_ref, got_ref / spread, cost, got_oracle))
    assert cost > 1e-4
    assert got_ref <= 4 * spread, "GPU vs one-product reference %.3e > 4 x spread %.3e" % (got_ref, spread)
    assert got_oracle <= 2 * cost, "GPU vs fp32 oracle %.3e > 2 x cost %.3e" % (got_oracle, cost)


def _profiled_forward(dec, feats):
    with torch.no_grad():
        dec(feats)                      # tile choices, packed weights
        torch.cuda.synchronize()
        _lib.profile_begin()
        out = dec(feats)
        recs = _lib.profile_end()
    return out, recs


@pytest.mark.parametrize("size", [(64, 96), (192, 640)])
def test_the_mode_is_taken_and_the_default_is_untouched(dev, size):
    feats = [f.to(dev) for f in kitti_feats(2, *size)]
    calls = lambda recs, pred: sum(r["calls"] for r in recs if pred(r["kernel"]))
    is_fp32_trunk = lambda n: n.startswith("conv_wino") or (n.startswith("conv_fwd_kernel<") and n.endswith(",9>"))
    for mode, terms in (("bf16x3", 3), ("bf16", 1)):
        dec = _decoder(dev).set_precision(mode)
        _, recs = _profiled_forward(dec, feats)
        assert calls(recs, lambda n: n.startswith("conv_bf16_kernel<") and n.endswith(",%d>" % terms)) == 8, recs
        assert calls(recs, lambda n: n.startswith("conv_bf16_kernel<")) == 8
        assert calls(recs, is_fp32_trunk) == 0, recs
        rep = dec.trunk_precision_report()
        assert len(rep) == 8 and set(rep.values()) == {mode}
        for r in recs:
            if r["kernel"].startswith("conv_bf16_kernel<"):
                assert r["mfma_flops"] == pytest.approx(terms * r["flops"])
    ref_dec = _decoder(dev)
    ref_out, recs = _profiled_forward(ref_dec, feats)
    assert calls(recs, lambda n: "bf16" in n) == 0
    assert calls(recs, is_fp32_trunk) >= 1
    assert set(ref_dec.trunk_precision_report().values()) == {"fp32"}
    dec = _decoder(dev).set_precision("bf16x3")
    with torch.no_grad():
        dec(feats)
        out = dec.set_precision("fp32")(feats)
    for k, v in ref_out.items():
        assert torch.equal(out[k], v), key_str(k)


def test_graph_routes_honour_the_mode(dev):
    feats = [f.to(dev) for f in kitti_feats(2, 64, 96)]
    clone = lambda o: {k: v.clone() for k, v in o.items()}
    same = lambda a, b: all(torch.equal(a[k], b[k]) for k in b) and set(a) == set(b)
    with torch.no_grad():
        eager = {m: clone(_decoder(dev).set_precision(m)(feats)) for m in ("bf16x3", "bf16")}
        assert not same(eager["bf16"], eager["bf16x3"])
        dec = _decoder(dev).set_precision("bf16x3").enable_graph(True)
        first = clone(dec(feats))
        n0 = dec.capture_count
        for _ in range(2):
            assert same(clone(dec(feats)), first)
        assert dec.capture_count == n0 and same(first, eager["bf16x3"])
        assert same(clone(dec.set_precision("bf16")(feats)), eager["bf16"])
        assert dec.capture_count == n0 + 1
        assert same(clone(dec.set_precision("bf16x3")(feats)), first)
        assert dec.capture_count == n0 + 1
        assert set(dec.trunk_precision_report().values()) == {"bf16x3"}
        # two graph segments on two streams
        dec2 = _decoder(dev).set_precision("bf16x3")
        dec2.two_stream_graphs = True
        dec2.enable_graph(True)
        assert same(clone(dec2(feats)), eager["bf16x3"])
        assert same(clone(dec2.set_precision("bf16")(feats)), eager["bf16"])
        # bind_inputs, copy route: fresh tensors, no re-capture
        dec3 = _decoder(dev).set_precision("bf16x3")
        dec3.bind_inputs(feats, pointer_sets=0)
        n3 = dec3.capture_count
        fresh = [f.to(dev) for f in kitti_feats(2, 64, 96, seed=7)]
        want = clone(_decoder(dev).set_precision("bf16x3")(fresh))
        assert same(clone(dec3(fresh)), want)
        assert dec3.capture_count == n3 and dec3.static_route["copy"] >= 1
        # encoder edge: a deferred ReLU in front of upconv(4, 0)
        from wavelet_monodepth_amd.layers import DeferredActivation
        pre = [f.clone() for f in feats]
        pre[-1] = feats[-1] - 0.5
        act = pre[:-1] + [torch.relu(pre[-1])]
        dec4 = _decoder(dev).set_precision("bf16x3")
        want = clone(dec4(act))
        got = dec4(pre[:-1] + [DeferredActivation(pre[-1], "leaky", 0.0)])
        assert same(got, want) and set(dec4.trunk_precision_report().values()) == {"bf16x3"}
    # autograd enabled: the fp32 path runs regardless of the mode
    fg = [f.clone().requires_grad_(True) for f in feats]
    with torch.enable_grad():
        out = _decoder(dev).set_precision("bf16x3")(fg)
        ref = _decoder(dev)([f.clone().requires_grad_(True) for f in feats])
        for k, v in ref.items():
            assert torch.equal(out[k], v), key_str(k)
        sum((out[("disp", s)] ** 2).mean() for s in range(4)).backward()
    assert all(f.grad is not None for f in fg)


def test_unsupported_layers_fall_back_per_layer_and_are_reported(dev):
    from wavelet_monodepth_amd.kitti import DepthWaveProgressiveDecoder
    dec = _decoder(dev, MOBILENET, seed=4).set_precision("bf16x3")
    feats = kitti_feats(1, 64, 64, MOBILENET, seed=4)
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    with torch.no_grad():
        out = dec([f.to(dev) for f in feats])
        ref = R.kitti_wave_decoder(feats, sd)
    for k, v in ref.items():
        assert_close(out[k], v, NET_TOL, key_str(k))
    rep = dec.trunk_precision_report()
    assert rep[("upconv", 2, 1)] == "fp32"
    assert [v for k, v in rep.items() if k != ("upconv", 2, 1)] == ["bf16x3"] * 7
