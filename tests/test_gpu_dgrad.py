"""The data gradient (wmd_conv_dgrad) held against autograd of the oracle in float64, configuration by configuration.

wmd_conv_dgrad has no kernels of its own: it runs the forward convolution table in a geometry the forward never uses (dz as the
input, read at (y-1, x-1) and zero outside its H x W extent -- shift1 = 1 --, an (H+2) x (W+2) output, the transposed and flipped
weight images, zero padding, no activation), then conv_dgrad_fold_kernel folds the padded-domain gradient back onto dx1 / dx2
(reflect / replicate borders, the concat split, the 2x2 sum of an upsampled x1, the optional x1_fwd gate).  The autotuner picks
the (configuration, K split) pair by time alone, so every pair it may pick is compared here, forced through
wmd_conv_dgrad_args.tune_cfg / tune_ksplit, every launch into NaN-filled outputs over a NaN-filled workspace.
"""
import collections
import ctypes as C
import os
import zlib

import numpy as np
import pytest
import torch

from oracle import decoder_ref as R
from util import (bench_tune_cache_name, channel_subset, chunk_channels, committed_entries, family, offered_splits,
                  quarter_family_declines, serves, split_accepted)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT_TOL, WINO_TOL = 2e-5, 5e-5
WINOGRAD = os.environ.get("WMD_WINOGRAD", "1") != "0"
FAMILIES = ("direct3x3", "1x1", "wino", "wino32", "wino32q")
COMPARED = collections.Counter()     # family -> (configuration, split) pairs compared with the oracle in dgrad geometry
TICKETS = collections.Counter()      # family -> in-kernel split-K finishes among them


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()))


def _act64(act, slope):
    return {"elu": torch.nn.functional.elu, "leaky": lambda v: torch.nn.functional.leaky_relu(v, slope), "sigmoid": torch.sigmoid}[act]


class Dgrad:
    """One data-gradient problem: float32 device operands, packed weight images, the float64 oracle's dx1 / dx2 (optionally
    gated: x1 = act(pre) is then an activation output and the oracle differentiates through it)."""

    def __init__(self, dev, B, C1, C2, up, Cout, H, W, k, pad, tag, gate=None, slope=0.1, oracle=True):
        from wavelet_monodepth_amd import ops
        self.dev, self.B, self.C1, self.C2, self.up, self.Cout, self.H, self.W, self.k, self.pad = dev, B, C1, C2, up, Cout, H, W, k, pad
        self.gate, self.slope = gate, slope
        g = _gen(tag)
        self.w = torch.randn((Cout, C1 + C2, k, k), generator=g) / (3.0 * (C1 + C2) ** 0.5)
        self.dz = torch.randn((B, Cout, H, W), generator=g)
        self.pre = torch.randn((B, C1, H // up, W // up), generator=g, dtype=torch.float64) if gate else None
        wd = self.w.to(dev)
        self.wpd = ops.pack_weights(wd, dgrad=True)
        self.wpw = ops.pack_weights_wino(wd, dgrad=True) if k == 3 else None
        self.dzd = self.dz.to(dev)
        self.x1_fwd = _act64(gate, slope)(self.pre).float().to(dev) if gate else None
        self.ref1 = self.ref2 = None
        if oracle:
            r1, r2 = self.oracle(range(B))
            self.ref1 = r1.to(dev)
            self.ref2 = None if r2 is None else r2.to(dev)

    def oracle(self, frames):
        """autograd of sum(dz * conv(P(x1, x2))) through oracle.decoder_ref in float64 on the CPU, for the listed frames"""
        frames = list(frames)
        n, h, w = len(frames), self.H // self.up, self.W // self.up
        if self.gate:
            pre = self.pre[frames].clone().requires_grad_(True)
            x1 = _act64(self.gate, self.slope)(pre)
        else:
            pre = x1 = torch.zeros((n, self.C1, h, w), dtype=torch.float64, requires_grad=True)
        x2 = torch.zeros((n, self.C2, self.H, self.W), dtype=torch.float64, requires_grad=True) if self.C2 else None
        xin = R.up2(x1) if self.up == 2 else x1
        if x2 is not None:
            xin = torch.cat([xin, x2], 1)
        w64 = self.w.double()
        y = R.conv3x3(xin, w64, None, self.pad) if self.k == 3 else R.conv1x1(xin, w64, None)
        (y * self.dz[frames].double()).sum().backward()
        return pre.grad, None if x2 is None else x2.grad

    def launch(self, cfg, ks, dx1=True, dx2=None, out=None):
        """-> (status, dx1, dx2): NaN-filled outputs (or the caller's `out` pair), workspace filled with NaN before the launch"""
        from wavelet_monodepth_amd import _lib
        dx2 = self.C2 > 0 if dx2 is None else dx2
        nan = float("nan")
        if out is None:
            o1 = torch.full((self.B, self.C1, self.H // self.up, self.W // self.up), nan, device=self.dev) if dx1 else None
            o2 = torch.full((self.B, self.C2, self.H, self.W), nan, device=self.dev) if dx2 else None
        else:
            o1, o2 = out
        p = lambda v: None if v is None else v.data_ptr()
        a = _lib.ConvDgradArgs(B=self.B, H=self.H, W=self.W, C1=self.C1, up1=self.up, C2=self.C2, Cout=self.Cout, ksize=self.k,
                               pad_mode=_lib.PAD[self.pad], dz=self.dzd.data_ptr(), wp_dgrad=self.wpd.data_ptr(), dx1=p(o1), dx2=p(o2),
                               workspace=None, workspace_floats=0, tune_cfg=cfg, tune_ksplit=ks, wp_dgrad_wino=p(self.wpw),
                               x1_fwd=p(self.x1_fwd), x1_act=_lib.ACT[self.gate] if self.gate else 0, x1_slope=self.slope)
        l = _lib.lib()
        n = l.wmd_conv_dgrad_workspace_floats(C.byref(a))
        ws = torch.full((max(n, 1),), nan, device=self.dev)
        a.workspace, a.workspace_floats = ws.data_ptr(), n
        st = l.wmd_conv_dgrad(C.byref(a), torch.cuda.current_stream().cuda_stream)
        return st, o1, o2

    def compare(self, dx1, dx2, tol, what):
        for got, ref, nm in ((dx1, self.ref1, "dx1"), (dx2, self.ref2, "dx2")):
            if got is None:
                continue
            assert bool(torch.isfinite(got).all()), "%s: %s has non-finite values (an unwritten or poisoned element)" % (what, nm)
            err = float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
            assert err <= tol, "%s: %s max relative error %.3e > %.1e" % (what, nm, err, tol)


# ---- A. every configuration x every offered split, in dgrad geometry -------------------------------------------------------
DGRAD_CASES = [
    # B, C1, C2, up, Cout, H, W, k, pad          (dgrad geometry: (H+2) x (W+2) outputs, a reduction over the forward's Cout)
    (2, 24, 0, 1, 40, 11, 46, 3, "reflect"),     # 13 x 48: every tile overhangs in both directions (6-row, 40- and 32-wide ones too)
    (2, 16, 0, 1, 21, 13, 48, 3, "replicate"),   # ragged reduction (the quarter family declines); padded width 50 = 2 (mod 4)
    (2, 16, 16, 2, 24, 12, 40, 3, "reflect"),    # upsampled x1 + skip tensor: concat split and 2x2 sum in the fold; 14 x 42
    (2, 24, 0, 2, 32, 8, 16, 3, "zero"),         # upsampled x1 without a skip tensor
    (3, 8, 0, 1, 16, 2, 2, 3, "reflect"),        # smallest legal reflect map: every border folds onto every pixel
    (2, 5, 0, 1, 12, 1, 9, 3, "zero"),           # H = 1, ragged channels on both sides
    (2, 16, 0, 1, 16, 6, 206, 3, "zero"),        # 8 x 208: three-plus 64-wide tiles, interior tiles take 16-byte staging with sh = 1
    (2, 8, 8, 2, 136, 10, 30, 3, "replicate"),   # deep ragged-by-slice reduction: 17 chunks of 8 (ks_eff < ks, a short last slice)
    (2, 24, 0, 1, 128, 9, 20, 3, "reflect"),     # 16 chunks of 8: ks = 16 runs one chunk per slice
    (2, 40, 0, 1, 100, 7, 9, 1, "zero"),         # 1x1 direct (the GEMM writes dx1), ragged 4-chunk reduction
    (2, 24, 16, 1, 72, 5, 12, 1, "zero"),        # 1x1 concat: through the fold with no halo
]


def _case_id(c):
    return "x".join(str(v) for v in c)


@pytest.mark.parametrize("case", DGRAD_CASES, ids=_case_id)
def test_dgrad_every_configuration_and_split_vs_oracle(dev, case):
    """Each table entry that serves the layer, forced, on every split the tuner may offer it (tuner.KSPLITS and their second-stage
    forms -k), against the float64 oracle; a split the planner cannot form must be refused (-3), never computed.  Where both ran,
    the in-kernel finish k and the second-stage sum -k of a configuration are bit-identical (dgrad has no activation: same
    slices, same order, same bits)."""
    from wavelet_monodepth_amd import _lib, tuner
    B, C1, C2, up, Cout, H, W, k, pad = case
    p = Dgrad(dev, B, C1, C2, up, Cout, H, W, k, pad, "A" + _case_id(case))
    tested = served = 0
    for i, name in enumerate(tuner.config_names()):
        if not serves(name, k) or (name.startswith("conv_wino") and not WINOGRAD):
            continue
        served += 1
        fam = family(name)
        tol = WINO_TOL if name.startswith("conv_wino") else DIRECT_TOL
        got = {}
        for ks in offered_splits():
            what = "%s ksplit %d case %s" % (name, ks, _case_id(case))
            st, dx1, dx2 = p.launch(i + 1, ks)
            if quarter_family_declines(name, Cout, 0):       # dgrad geometry: the reduction (forward Cout) is the conv's C1
                assert st == -3, "%s: the quarter family must decline a ragged reduction (status %d)" % (what, st)
                continue
            if not split_accepted(name, ks, Cout):
                assert st == -3, "%s: the planner accepted a split it cannot form (status %d)" % (what, st)
                continue
            _lib.check(st, what)
            p.compare(dx1, dx2, tol, what)
            got[ks] = (dx1, dx2)
            COMPARED[fam] += 1
            if ks > 1 and fam.startswith("wino32"):
                TICKETS[fam] += 1
            tested += 1
        assert 1 in got or quarter_family_declines(name, Cout, 0), "%s case %s: not compared unsplit" % (name, _case_id(case))
        for ks in [s for s in got if s > 1 and -s in got]:
            for a_, b_, nm in zip(got[ks], got[-ks], ("dx1", "dx2")):
                if a_ is not None:
                    assert torch.equal(a_, b_), "%s case %s: %s of the in-kernel finish (%d) != second-stage sum (%d)" % (
                        name, _case_id(case), nm, ks, -ks)
    assert served >= (4 if k == 1 else 50 if WINOGRAD else 30) and tested >= served, "case %s: %d pairs compared over %d configurations" % (
        _case_id(case), tested, served)


# ---- B. the fold and the gate ------------------------------------------------------------------------------------------------
FOLD_CASES = [
    # B, C1, C2, up, Cout, H, W, k, pad, (dx1, dx2)
    (2, 16, 8, 2, 24, 12, 20, 3, "reflect", (True, False)),
    (2, 16, 8, 2, 24, 12, 20, 3, "reflect", (False, True)),
    (2, 16, 8, 2, 24, 12, 20, 3, "reflect", (True, True)),
    (2, 12, 10, 1, 16, 7, 10, 3, "replicate", (True, True)),    # W % 4 != 0: the scalar fold even when aligned
    (2, 12, 10, 1, 16, 7, 12, 1, "zero", (False, True)),
    (2, 12, 10, 1, 16, 7, 12, 1, "zero", (True, True)),
]


def _view_at_4_bytes(shape, dev):
    """NaN-filled [shape] view that starts one float into a larger buffer: 4-byte aligned, never 16-byte aligned"""
    n = int(np.prod(shape))
    buf = torch.full((n + 4,), float("nan"), device=dev)
    v = buf[1:1 + n].view(shape)
    assert v.data_ptr() % 16 == 4
    return v


def _check_offset_launch(p, dx_mask, aligned, what):
    """the same launch into views at a 4-byte offset (the scalar fold, or the GEMM's own stores for the 1x1 direct path):
    bit-identical to the aligned launch and within the oracle's tolerance"""
    from wavelet_monodepth_amd import _lib
    want1, want2 = dx_mask
    o1 = _view_at_4_bytes((p.B, p.C1, p.H // p.up, p.W // p.up), p.dev) if want1 else None
    o2 = _view_at_4_bytes((p.B, p.C2, p.H, p.W), p.dev) if want2 else None
    st, d1, d2 = p.launch(0, 0, out=(o1, o2))
    _lib.check(st, what + " (4-byte offset outputs)")
    for a_, b_, nm in ((d1, aligned[0], "dx1"), (d2, aligned[1], "dx2")):
        if a_ is not None:
            assert torch.equal(a_, b_), "%s: %s at a 4-byte offset differs from the aligned launch" % (what, nm)
    p.compare(d1, d2, WINO_TOL, what + " (4-byte offset outputs)")


@pytest.mark.parametrize("case", FOLD_CASES, ids=_case_id)
def test_dgrad_fold_dx1_dx2_and_unaligned_views_vs_oracle(dev, case):
    """dx1 only, dx2 only and both (a launch writes what it is given and nothing else), aligned and at a 4-byte offset"""
    from wavelet_monodepth_amd import _lib
    B, C1, C2, up, Cout, H, W, k, pad, (want1, want2) = case
    p = Dgrad(dev, B, C1, C2, up, Cout, H, W, k, pad, "B" + _case_id(case[:-1]))
    what = "fold case %s dx1=%d dx2=%d" % (_case_id(case[:-1]), want1, want2)
    st, d1, d2 = p.launch(0, 0, dx1=want1, dx2=want2)
    _lib.check(st, what)
    assert (d1 is None) != want1 and (d2 is None) != want2
    p.compare(d1, d2, WINO_TOL, what)
    _check_offset_launch(p, (want1, want2), (d1, d2), what)


GATE_CASES = [
    # B, C1, C2, up, Cout, H, W, k, pad
    (2, 16, 0, 1, 24, 10, 12, 3, "replicate"),    # up = 1: the fold's vector path gates 4 outputs a thread
    (2, 16, 8, 2, 24, 12, 20, 3, "reflect"),      # up = 2 (+ skip): 2 gated outputs a thread
    (2, 16, 0, 2, 24, 6, 14, 3, "zero"),          # up = 2, W % 4 != 0: the scalar fold
]


@pytest.mark.parametrize("act", ["elu", "leaky", "sigmoid"])
@pytest.mark.parametrize("case", GATE_CASES, ids=_case_id)
def test_dgrad_fold_gate_vs_oracle(dev, case, act):
    """x1_fwd gating: x1 is an activation output, dx1 comes back multiplied by the activation's derivative at x1_fwd (the oracle
    differentiates through act(pre) in float64); the library's choice, a forced split of each family, and the 4-byte offset views"""
    from wavelet_monodepth_amd import _lib, tuner
    B, C1, C2, up, Cout, H, W, k, pad = case
    p = Dgrad(dev, B, C1, C2, up, Cout, H, W, k, pad, "G" + _case_id(case) + act, gate=act)
    what = "gate %s case %s" % (act, _case_id(case))
    st, d1, d2 = p.launch(0, 0)
    _lib.check(st, what)
    p.compare(d1, d2, WINO_TOL, what)
    _check_offset_launch(p, (True, C2 > 0), (d1, d2), what)
    names = tuner.config_names()
    for name in ("conv_fwd_kernel<8,16,2,4,1,2,8,9>", "conv_wino_kernel<8,16,2,2,2,8>", "conv_wino32_kernel<8,16,1,8>",
                 "conv_wino32q_kernel<8,16,8>"):
        assert name in names, name
        if name.startswith("conv_wino") and not WINOGRAD:
            continue
        for ks in (1, 3, -3) if name.startswith("conv_wino32") else (1, 3):
            st, e1, e2 = p.launch(names.index(name) + 1, ks)
            _lib.check(st, "%s %s ksplit %d" % (what, name, ks))
            p.compare(e1, e2, WINO_TOL if name.startswith("conv_wino") else DIRECT_TOL, "%s %s ksplit %d" % (what, name, ks))


@pytest.mark.parametrize("act", ["elu", "leaky", "sigmoid"])
def test_dgrad_1x1_direct_gate_in_the_gemm_epilogue_and_split_reduce(dev, act):
    """1x1 without upsample / concat: the GEMM output is dx1 itself and the gate lives in its epilogue (ks = 1) or in the split-K
    reduce (ks > 1) -- every 1x1 configuration, splits 1..4, against the oracle; the library's choice also at a 4-byte offset"""
    from wavelet_monodepth_amd import _lib, tuner
    p = Dgrad(dev, 2, 40, 0, 1, 100, 7, 9, 1, "zero", "D" + act, gate=act)
    tested = 0
    for i, name in enumerate(tuner.config_names()):
        if not serves(name, 1):
            continue
        for ks in (1, 2, 3, 4):
            what = "1x1 direct gate %s %s ksplit %d" % (act, name, ks)
            st, d1, _ = p.launch(i + 1, ks)
            if not split_accepted(name, ks, 100):
                assert st == -3, what
                continue
            _lib.check(st, what)
            p.compare(d1, None, DIRECT_TOL, what)
            COMPARED["1x1"] += 1
            tested += 1
    assert tested >= 4 * 3
    st, d1, _ = p.launch(0, 0)
    _lib.check(st, "1x1 direct gate %s" % act)
    _check_offset_launch(p, (True, False), (d1, None), "1x1 direct gate %s" % act)


# ---- C. coherence of the in-kernel finish at the data gradient's real geometry ------------------------------------------------
@pytest.mark.skipif(not WINOGRAD, reason="Winograd family switched off (WMD_WINOGRAD=0)")
@pytest.mark.parametrize("name,ks,shape", [
    # config 2 levels at batch 12 (B, H, W, C1, up, C2, Cout): padded widths 322 / 162 / 162 / 42, all = 2 (mod 4)
    ("conv_wino32q_kernel<8,16,8>", 4, (12, 96, 320, 16, 1, 0, 32)),
    ("conv_wino32_kernel<16,16,2,8>", 8, (12, 48, 160, 32, 1, 0, 64)),
    ("conv_wino32_kernel<8,16,1,8>", 4, (12, 48, 160, 64, 2, 64, 64)),
    ("conv_wino32_kernel<6,40,2,8>", 8, (12, 12, 40, 256, 1, 0, 128)),
])
def test_dgrad_in_kernel_finish_is_coherent_at_real_level_sizes(dev, name, ks, shape):
    """The split-K ticket finish in dgrad geometry (TW = 16 tiles and a 40-wide one on widths = 2 mod 4: the finish's dword path):
    40 launches into NaN-filled outputs over a workspace poisoned before every launch, each bit-identical to the first and to the
    second-stage sum of the same slices; the first against the float64 oracle on three frames"""
    from wavelet_monodepth_amd import _lib, tuner
    B, H, W, C1, up, C2, Cout = shape
    names = tuner.config_names()
    assert name in names, name
    p = Dgrad(dev, B, C1, C2, up, Cout, H, W, 3, "reflect", "C%s%d" % (name, ks), oracle=False)
    cfg = names.index(name) + 1
    assert split_accepted(name, ks, Cout)
    st, r1, r2 = p.launch(cfg, -ks)
    _lib.check(st, "%s ksplit %d" % (name, -ks))
    st, f1, f2 = p.launch(cfg, ks)
    _lib.check(st, "%s ksplit %d" % (name, ks))
    for a_, b_, nm in ((f1, r1, "dx1"), (f2, r2, "dx2")):
        if a_ is not None:
            assert bool(torch.isfinite(a_).all()), "%s: %s of the first launch is not finite" % (name, nm)
            assert torch.equal(a_, b_), "%s: %s of the in-kernel finish != second-stage sum, %d slices" % (name, nm, ks)
    for rep in range(40):
        st, y1, y2 = p.launch(cfg, ks)
        _lib.check(st, name)
        for a_, b_, nm in ((y1, f1, "dx1"), (y2, f2, "dx2")):
            if a_ is not None:
                assert torch.equal(a_, b_), "%s ksplit %d: %s of launch %d differs from the first" % (name, ks, nm, rep)
    frames = (0, 7, 11)
    o1, o2 = p.oracle(frames)
    for got, ref, nm in ((f1, o1, "dx1"), (f2, o2, "dx2")):
        if got is not None:
            err = float((got[list(frames)].double().cpu() - ref).abs().max() / ref.abs().max())
            assert err <= WINO_TOL, "%s ksplit %d frames %s: %s max relative error %.3e" % (name, ks, frames, nm, err)
    COMPARED[family(name)] += 1
    TICKETS[family(name)] += 1


def test_every_family_was_compared_in_dgrad_geometry():
    """(runs after the sweeps above, in file order) each family met the oracle in dgrad geometry, with in-kernel finishes"""
    want = FAMILIES if WINOGRAD else ("direct3x3", "1x1")
    print("dgrad (configuration, split) pairs compared per family: %s; in-kernel finishes: %s" % (
        ", ".join("%s %d" % (f, COMPARED[f]) for f in FAMILIES), ", ".join("%s %d" % (f, TICKETS[f]) for f in FAMILIES)))
    missing = [f for f in want if COMPARED[f] == 0]
    assert not missing, "families never compared in dgrad geometry (run the whole module): %s" % missing
    if WINOGRAD:
        assert TICKETS["wino32"] + TICKETS["wino32q"] > 0, "no in-kernel split-K finish was compared"


# ---- D. what bench.py runs: every committed choice at its own shape -------------------------------------------------------------
_BENCH = {}


def _bench_module():
    if "m" not in _BENCH:
        import importlib.util
        spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(ROOT, "bench.py"))
        bench = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(bench)
        _BENCH["m"] = bench
    return _BENCH["m"]


def _err(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


@pytest.mark.skipif(not WINOGRAD, reason="Winograd family switched off (WMD_WINOGRAD=0): the committed choices name it")
@pytest.mark.parametrize("key,choice", committed_entries(), ids=[k for k, _ in committed_entries()])
def test_committed_tune_choice_vs_oracle(dev, key, choice):
    """Every conv| / dgrad| / wgrad| entry of the tile choices bench.py preloads, forced at the entry's own H, W and channels with
    B = 2, against the float64 oracle on a channel subset (forward y[co] needs only w[co]; dgrad dx[ci] only w[:, ci]; wgrad
    dW[co, ci] only dz[co] and x[ci]: the subset's values are exact, not approximated)."""
    from wavelet_monodepth_amd import _lib, ops, tuner
    bench = _bench_module()
    assert bench.TUNE_CACHE == bench_tune_cache_name()
    kind, *f = key.split("|")
    _, H, W, C1, up, C2, Cout, k = (int(v) for v in f[:8])
    B, pad = 2, "reflect"
    label, ks = choice
    l = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    g = _gen("D" + key)
    Cin = C1 + C2
    w = torch.randn((Cout, Cin, k, k), generator=g) / (3.0 * Cin ** 0.5)
    what = "%s -> %s ksplit %d" % (key, label, ks)
    if kind in ("conv", "dgrad"):
        names = tuner.config_names()
        assert label in names, "%s: the committed choice is not in the table" % what
        cfg = names.index(label) + 1
        tol = WINO_TOL if label.startswith("conv_wino") else DIRECT_TOL
    if kind == "conv":
        x1 = torch.randn((B, C1, H // up, W // up), generator=g)
        x2 = torch.randn((B, C2, H, W), generator=g) if C2 else None
        b = torch.randn((Cout,), generator=g) * 0.1
        wd, x1d, x2d, bd = w.to(dev), x1.to(dev), None if x2 is None else x2.to(dev), b.to(dev)
        wp, ww = ops.pack_weights(wd), ops.pack_weights_wino(wd)
        y = torch.full((B, Cout, H, W), float("nan"), device=dev)
        a = _lib.ConvArgs(B=B, H=H, W=W, C1=C1, up1=up, C2=C2, Cout=Cout, ksize=k, pad_mode=_lib.PAD[pad], act=_lib.ACT["elu"],
                          slope=0.0, x1=x1d.data_ptr(), x2=None if x2d is None else x2d.data_ptr(), wp=wp.data_ptr(),
                          bias=bd.data_ptr(), y=y.data_ptr(), workspace=None, workspace_floats=0, tune_cfg=cfg, tune_ksplit=ks,
                          wp_wino=None if ww is None else ww.data_ptr())
        n = l.wmd_conv_fwd_workspace_floats(C.byref(a))
        ws = torch.full((max(n, 1),), float("nan"), device=dev)
        a.workspace, a.workspace_floats = ws.data_ptr(), n
        _lib.check(l.wmd_conv_fwd(C.byref(a), stream), what)
        co = channel_subset(Cout, key)
        xin = R.up2(x1.double()) if up == 2 else x1.double()
        if x2 is not None:
            xin = torch.cat([xin, x2.double()], 1)
        ws_, bs_ = w[co].double(), b[co].double()
        ref = torch.nn.functional.elu(R.conv3x3(xin, ws_, bs_, pad) if k == 3 else R.conv1x1(xin, ws_, bs_))
        got = y[:, co]
        assert bool(torch.isfinite(y).all()), "%s: non-finite outputs" % what
        err = _err(got, ref)
        assert err <= tol, "%s: y[%d channels] max relative error %.3e > %.1e" % (what, len(co), err, tol)
    elif kind == "dgrad":
        mask = int(f[8])
        p = Dgrad(dev, B, C1, C2, up, Cout, H, W, k, pad, "D" + key, oracle=False)
        st, d1, d2 = p.launch(cfg, ks, dx1=bool(mask & 1), dx2=bool(mask & 2))
        _lib.check(st, what)
        # oracle over the input-channel subset only: dx[ci] = (W[:, ci])^T (*) dz
        s1 = channel_subset(C1, key + "|1")
        s2 = channel_subset(C2, key + "|2") if C2 and mask & 2 else []
        x1 = torch.zeros((B, len(s1), H // up, W // up), dtype=torch.float64, requires_grad=True)
        x2 = torch.zeros((B, len(s2), H, W), dtype=torch.float64, requires_grad=True) if s2 else None
        xin = R.up2(x1) if up == 2 else x1
        if x2 is not None:
            xin = torch.cat([xin, x2], 1)
        wsub = p.w[:, s1 + [C1 + c for c in s2]].double()
        yv = R.conv3x3(xin, wsub, None, pad) if k == 3 else R.conv1x1(xin, wsub, None)
        (yv * p.dz.double()).sum().backward()
        for got, sub, ref, nm in ((d1, s1, x1.grad, "dx1"), (d2, s2, None if x2 is None else x2.grad, "dx2")):
            if got is None:
                continue
            assert bool(torch.isfinite(got).all()), "%s: %s has non-finite values" % (what, nm)
            if ref is not None:
                err = _err(got[:, sub], ref)
                assert err <= tol, "%s: %s[%d channels] max relative error %.3e > %.1e" % (what, nm, len(sub), err, tol)
        assert (d1 is not None) == bool(mask & 1) and (d2 is not None) == bool(mask & 2)
    else:
        assert kind == "wgrad", key
        wn = [l.wmd_conv_wgrad_config_name(i).decode() for i in range(l.wmd_conv_wgrad_num_configs())]
        cfg = {"library": 0, "direct": -1}.get(label)
        if cfg is None:
            assert label in wn, "%s: the committed choice is not in the weight-gradient table" % what
            cfg = wn.index(label) + 1
        x1 = torch.randn((B, C1, H // up, W // up), generator=g)
        x2 = torch.randn((B, C2, H, W), generator=g) if C2 else None
        dz = torch.randn((B, Cout, H, W), generator=g)
        x1d, x2d, dzd = x1.to(dev), None if x2 is None else x2.to(dev), dz.to(dev)
        dw = torch.full((Cout, Cin, k, k), float("nan"), device=dev)
        db = torch.full((Cout,), float("nan"), device=dev)
        a = _lib.ConvWgradArgs(B=B, H=H, W=W, C1=C1, up1=up, C2=C2, Cout=Cout, ksize=k, pad_mode=_lib.PAD[pad], x1=x1d.data_ptr(),
                               x2=None if x2d is None else x2d.data_ptr(), dz=dzd.data_ptr(), dw=dw.data_ptr(), dbias=db.data_ptr(),
                               workspace=None, workspace_floats=0, tune_cfg=cfg, tune_nsplit=0)
        n = l.wmd_conv_wgrad_workspace_floats(C.byref(a))
        ws = torch.full((max(n, 1),), float("nan"), device=dev)
        a.workspace, a.workspace_floats = ws.data_ptr(), n
        _lib.check(l.wmd_conv_wgrad(C.byref(a), stream), what)
        co, ci = channel_subset(Cout, key + "|o"), channel_subset(Cin, key + "|i")
        xin = R.up2(x1.double()) if up == 2 else x1.double()
        if x2 is not None:
            xin = torch.cat([xin, x2.double()], 1)
        wsub = w[co][:, ci].double().requires_grad_(True)
        yv = R.conv3x3(xin[:, ci], wsub, None, pad) if k == 3 else R.conv1x1(xin[:, ci], wsub, None)
        (yv * dz[:, co].double()).sum().backward()
        assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all()), "%s: non-finite dW / db" % what
        err = _err(dw[co][:, ci], wsub.grad)
        assert err <= DIRECT_TOL, "%s: dW[%d x %d channels] max relative error %.3e" % (what, len(co), len(ci), err)
        err = _err(db[co], dz[:, co].double().sum((0, 2, 3)))
        assert err <= DIRECT_TOL, "%s: db max relative error %.3e" % (what, err)
