"""The weight gradient (wmd_conv_wgrad) held against autograd of the oracle in float64, configuration by configuration.

wmd_conv_wgrad runs one of three families, each over a split of the pixel tiles into partial sums that a second kernel reduces in
a fixed order: the Winograd F(2x2,3x3) table (conv_wgrad_wino_kernel / conv_wgrad_wino32_kernel, tune_cfg = k forces entry k-1;
wgrad_wino_reduce_kernel), the direct MFMA table kWCfgs of wmd_conv_wgrad.hip (3x3 and 1x1; tune_cfg = -1, WMD_WGRAD_CFG=<1-based
index> forces an entry; wgrad_reduce_kernel) and the VALU kernel of the heads' Cout <= 4 filters (WMD_WGRAD_SMALLCO=1).  Every
(entry, split) pair is compared here, every launch into NaN-filled dw / db over a NaN-filled workspace; the split the plan used is
read back from the workspace it asked for, and the kernel that ran from the library's launch profile.
"""
import collections
import ctypes as C
import os
import re
import zlib

import pytest
import torch

from oracle import decoder_ref as R
from util import channel_subset, committed_entries

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-5
FAMILIES = ("wino", "wino32", "direct3x3", "direct1x1", "smallco")
COMPARED = collections.defaultdict(set)   # family -> {(entry, split)} compared with the oracle
BIG_SPLIT = set()                         # entries compared with nsplit > 16
EMPTY_TAIL = set()                        # entries compared with a split whose last slices own no pixel tile
PLANNED = {}                              # section D: key -> (kernel, nsplit, dW error, db error)
ENV = ("WMD_WGRAD_CFG", "WMD_WGRAD_NSPLIT", "WMD_WGRAD_SMALLCO", "WMD_WGRAD_WINO", "WMD_WGRAD_WINO_CFG")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _planner_env(monkeypatch):
    """the planner's development switches are read per call: none of them may leak in from the caller's environment"""
    for v in ENV:
        monkeypatch.delenv(v, raising=False)


def family(name):
    if name.startswith("conv_wgrad_wino32"):
        return "wino32"
    if name.startswith("conv_wgrad_wino"):
        return "wino"
    if name.startswith("conv_wgrad_smallco"):
        return "smallco"
    return "direct1x1" if name.endswith(",1>") else "direct3x3"


def wino_names():
    from wavelet_monodepth_amd import _lib
    l = _lib.lib()
    return [l.wmd_conv_wgrad_config_name(i).decode() for i in range(l.wmd_conv_wgrad_num_configs())]


def direct_names():
    """kWCfgs in table order (WMD_WGRAD_CFG counts from 1), read from wmd_conv_wgrad.hip: the C ABI does not list this table"""
    src = open(os.path.join(ROOT, "wavelet_monodepth_amd", "csrc", "wmd_conv_wgrad.hip")).read()
    body = src[src.index("static const WgradCfg kWCfgs[] = {"):]
    body = body[:body.index("};")]
    rows = re.findall(r"^\s*WMD_WCFG\(([^)]*)\)", body, flags=re.M)
    return ["conv_wgrad_kernel<%s>" % ",".join(v.strip() for v in r.split(",")) for r in rows]


def ntiles(name, B, H, W):
    """pixel tiles the plan splits: the first two template arguments are the tile's rows and columns; the 1x1 direct entries
    see the map flattened to 1 x HW"""
    args = [int(v) for v in name[name.index("<") + 1:-1].split(",")]
    if family(name) == "direct1x1":
        H, W = 1, H * W
    return B * -(-H // args[0]) * -(-W // args[1])


def empty_tail(nt, ns):
    """per = ceil(ntiles / nsplit) tiles a slice: do the last slices start past the last tile?"""
    return (ns - 1) * -(-nt // ns) >= nt


def padded_input(x1, x2, up, k, pad):
    xin = R.up2(x1.double()) if up == 2 else x1.double()
    if x2 is not None:
        xin = torch.cat([xin, x2.double()], 1)
    return R.pad1(xin, pad) if k == 3 else xin


def autograd_oracle(x1, x2, dz, up, k, pad):
    """autograd of sum(dz * conv(P(x1, x2))) through oracle.decoder_ref in float64 on the CPU w.r.t. the weight and the bias"""
    Cin = x1.shape[1] + (0 if x2 is None else x2.shape[1])
    w = torch.zeros((dz.shape[1], Cin, k, k), dtype=torch.float64, requires_grad=True)
    b = torch.zeros((dz.shape[1],), dtype=torch.float64, requires_grad=True)
    xin = R.up2(x1.double()) if up == 2 else x1.double()
    if x2 is not None:
        xin = torch.cat([xin, x2.double()], 1)
    y = R.conv3x3(xin, w, b, pad) if k == 3 else R.conv1x1(xin, w, b)
    (y * dz.double()).sum().backward()
    return w.grad, b.grad


def gemm_oracle(x1, x2, dz, up, k, pad):
    """the same gradient as k*k float64 GEMMs over N = B*H*W: dW[:, :, ky, kx] = dz (Cout x N) . P(ky, kx) (N x Cin), with
    P = pad1(cat(up2(x1), x2)) and P(ky, kx) its window shifted by (ky, kx); db = the row sums of dz"""
    P = padded_input(x1, x2, up, k, pad)
    B, Cout, H, W = dz.shape
    dzm = dz.double().transpose(0, 1).reshape(Cout, -1)
    dw = torch.empty((Cout, P.shape[1], k, k), dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            dw[:, :, ky, kx] = dzm @ P[:, :, ky:ky + H, kx:kx + W].transpose(0, 1).reshape(P.shape[1], -1).T
    return dw, dzm.sum(1)


def _err(got, ref):
    return float((got.double().cpu() - ref.cpu()).abs().max() / ref.abs().max().clamp_min(1e-30))


class Wgrad:
    """One weight-gradient problem: float32 device x1, x2, dz and the float64 oracle's dW, db"""

    def __init__(self, dev, B, C1, C2, up, Cout, H, W, k, pad, tag):
        self.dev, self.B, self.C1, self.C2, self.up, self.Cout, self.H, self.W, self.k, self.pad = dev, B, C1, C2, up, Cout, H, W, k, pad
        g = torch.Generator().manual_seed(zlib.crc32(tag.encode()))
        x1 = torch.randn((B, C1, H // up, W // up), generator=g)
        x2 = torch.randn((B, C2, H, W), generator=g) if C2 else None
        dz = torch.randn((B, Cout, H, W), generator=g)
        self.x1, self.x2, self.dz = x1.to(dev), None if x2 is None else x2.to(dev), dz.to(dev)
        rw, rb = autograd_oracle(x1, x2, dz, up, k, pad)
        self.ref_w, self.ref_b = rw.to(dev), rb.to(dev)

    def launch(self, cfg, ns, bias=True, profile=False):
        """-> (status, dw, db, workspace floats, names of the kernels launched when profiled)"""
        from wavelet_monodepth_amd import _lib
        nan = float("nan")
        Cin = self.C1 + self.C2
        dw = torch.full((self.Cout, Cin, self.k, self.k), nan, device=self.dev)
        db = torch.full((self.Cout,), nan, device=self.dev) if bias else None
        a = _lib.ConvWgradArgs(B=self.B, H=self.H, W=self.W, C1=self.C1, up1=self.up, C2=self.C2, Cout=self.Cout, ksize=self.k,
                               pad_mode=_lib.PAD[self.pad], x1=self.x1.data_ptr(), x2=None if self.x2 is None else self.x2.data_ptr(),
                               dz=self.dz.data_ptr(), dw=dw.data_ptr(), dbias=None if db is None else db.data_ptr(),
                               workspace=None, workspace_floats=0, tune_cfg=cfg, tune_nsplit=ns)
        l = _lib.lib()
        n = l.wmd_conv_wgrad_workspace_floats(C.byref(a))
        ws = torch.full((max(n, 1),), nan, device=self.dev)
        a.workspace, a.workspace_floats = ws.data_ptr(), n
        if profile:
            _lib.profile_begin()
        st = l.wmd_conv_wgrad(C.byref(a), torch.cuda.current_stream().cuda_stream)
        names = [r["kernel"] for r in _lib.profile_end()] if profile else None
        return st, dw, db, n, names

    def compare(self, dw, db, what):
        for got, ref, nm in ((dw, self.ref_w, "dW"), (db, self.ref_b, "db")):
            if got is None:
                continue
            assert bool(torch.isfinite(got).all()), "%s: %s has non-finite values (an unwritten or poisoned element)" % (what, nm)
            err = _err(got, ref)
            assert err <= TOL, "%s: %s max relative error %.3e > %.1e" % (what, nm, err, TOL)


def sweep(p, name, cfg, splits, per_split):
    """Each requested split of one forced entry: the kernel that ran, the split the plan used (workspace / per_split floats,
    min(request, ntiles)), dW and db against the oracle, a second launch bit-identical to the first (the split is
    deterministic), a launch without dbias with the same dW bits.  A request above ntiles must equal the ntiles result."""
    from wavelet_monodepth_amd import _lib
    nt = ntiles(name, p.B, p.H, p.W) if family(name) != "smallco" else None
    got = {}
    for ns in splits:
        what = "%s nsplit %d case %s" % (name, ns, p.case)
        st, dw, db, n, kernels = p.launch(cfg, ns, profile=True)
        _lib.check(st, what)
        assert name in kernels, "%s: the launch ran %s" % (what, kernels)
        assert n > 0 and n % per_split == 0, "%s: workspace of %d floats is not whole slices of %d" % (what, n, per_split)
        used = n // per_split
        if nt is not None:
            assert used == min(ns, nt), "%s: the plan used %d slices (ntiles %d)" % (what, used, nt)
        p.compare(dw, db, what)
        st, dw2, db2, _, _ = p.launch(cfg, ns)
        _lib.check(st, what + " (second launch)")
        assert torch.equal(dw, dw2) and torch.equal(db, db2), "%s: two launches differ" % what
        st, dw3, _, _, _ = p.launch(cfg, ns, bias=False)
        _lib.check(st, what + " (dbias = NULL)")
        p.compare(dw3, None, what + " (dbias = NULL)")
        assert torch.equal(dw, dw3), "%s: dW without dbias differs from dW with it" % what
        if nt is not None and ns > nt:
            assert torch.equal(dw, got[nt][0]) and torch.equal(db, got[nt][1]), "%s: != the ntiles (%d) result" % (what, nt)
        got[used] = (dw, db)
        COMPARED[family(name)].add((name, used))
        if used > 16:
            BIG_SPLIT.add(name)
        if nt is not None and empty_tail(nt, used):
            EMPTY_TAIL.add(name)
    return got


def _case_id(c):
    return "x".join(str(v) for v in c)


def _problem(dev, case, tag):
    B, C1, C2, up, Cout, H, W, k, pad = case
    p = Wgrad(dev, B, C1, C2, up, Cout, H, W, k, pad, tag + _case_id(case))
    p.case = _case_id(case)
    return p


# ---- A. every Winograd entry x every pixel split --------------------------------------------------------------------------
WINO_SPLITS = (1, 2, 3, 7, 16, 17, 33, 49, 65)
WINO_CASES = [
    # B, C1, C2, up, Cout, H, W, k, pad
    (3, 48, 24, 2, 100, 24, 80, 3, "reflect"),    # 72 - 108 tiles (nsplit 65); a wino32 slab straddles x1 / x2; Cout > 64, 100 % 16 != 0
    (2, 19, 0, 1, 7, 6, 10, 3, "zero"),           # ragged channels, a map smaller than one tile row
    (3, 8, 0, 1, 16, 2, 2, 3, "reflect"),         # the smallest reflect map: one tile, every border mirrors
    (2, 32, 16, 2, 40, 12, 44, 3, "replicate"),   # C1 = 32: a pure upsampled slab next to a skip tensor; W = 44
    (2, 16, 8, 2, 19, 8, 26, 3, "reflect"),       # upsampled C1 < 32 (every slab mixes x1 and x2); W = 26
    (3, 64, 0, 2, 72, 14, 46, 3, "zero"),         # upsampled without x2, two pure slabs; Cout = 72; W = 46
    (2, 24, 0, 1, 40, 7, 21, 3, "replicate"),     # odd sizes: tiles overhang in both directions
    (1, 64, 0, 1, 3, 16, 48, 3, "reflect"),       # a head's Cout = 3 filter
]


@pytest.mark.parametrize("case", WINO_CASES, ids=_case_id)
def test_wgrad_winograd_every_entry_and_split_vs_oracle(dev, case):
    """Every entry of the Winograd table, forced through tune_cfg (the co16 head tiles at any Cout too), on the splits
    {1, 2, 3, 7, 16, 17, 33, 49, 65, ntiles} that fit and on one request above ntiles"""
    p = _problem(dev, case, "A")
    names = wino_names()
    assert len(names) >= 17 and all(n.startswith("conv_wgrad_wino") for n in names), names
    per_split = 16 * p.Cout * (p.C1 + p.C2) + p.Cout
    for i, name in enumerate(names):
        nt = ntiles(name, p.B, p.H, p.W)
        splits = sorted({s for s in WINO_SPLITS if s <= nt} | {nt}) + [nt + 5]
        sweep(p, name, i + 1, splits, per_split)


# ---- B. every direct entry, 3x3 and 1x1 --------------------------------------------------------------------------------------
DIRECT_SPLITS = (1, 3, 17, 49, 65)
DIRECT_CASES = [
    # B, C1, C2, up, Cout, H, W, k, pad
    (3, 48, 24, 2, 100, 24, 80, 3, "reflect"),    # 108 - 216 tiles; concat of an upsampled x1; Cout > 64 ragged
    (2, 19, 0, 1, 7, 5, 9, 3, "zero"),            # ragged channels, one tile
    (3, 8, 0, 1, 16, 2, 2, 3, "reflect"),         # 2 x 2 reflect
    (2, 16, 8, 2, 24, 10, 46, 3, "replicate"),    # W = 46
    (2, 40, 24, 1, 72, 5, 7, 1, "zero"),          # 1x1 concat, HW = 35 (the pixel domain is flattened to 1 x HW)
    (3, 40, 25, 1, 72, 45, 99, 1, "zero"),        # 1x1 concat, HW = 4455: 210 tiles of 64 pixels, the last one ragged
]


@pytest.mark.parametrize("case", DIRECT_CASES, ids=_case_id)
def test_wgrad_direct_every_entry_and_split_vs_oracle(dev, case, monkeypatch):
    """Every entry of kWCfgs with the layer's tap count, forced through WMD_WGRAD_CFG with tune_cfg = -1 (an entry of the other
    tap count would be ignored silently: the launch profile names the kernel that ran), on {1, 3, 17, 49, 65, ntiles} that fit
    and one request above ntiles"""
    p = _problem(dev, case, "B")
    names = direct_names()
    assert len(names) >= 14 and sum(n.endswith(",1>") for n in names) >= 2, names
    taps = 9 if p.k == 3 else 1
    per_split = p.Cout * (p.C1 + p.C2) * taps + p.Cout
    tested = 0
    for i, name in enumerate(names):
        if not name.endswith(",%d>" % taps):
            continue
        monkeypatch.setenv("WMD_WGRAD_CFG", str(i + 1))
        nt = ntiles(name, p.B, p.H, p.W)
        splits = sorted({s for s in DIRECT_SPLITS if s <= nt} | {nt}) + [nt + 5]
        sweep(p, name, -1, splits, per_split)
        tested += 1
    assert tested >= (12 if taps == 9 else 2)


# ---- C. the VALU kernel of the heads' Cout <= 4 filters ----------------------------------------------------------------------
@pytest.mark.parametrize("pad", ["zero", "reflect", "replicate"])
@pytest.mark.parametrize("cout", [1, 2, 3, 4])
def test_wgrad_smallco_kernel_vs_oracle(dev, monkeypatch, cout, pad):
    """conv_wgrad_smallco_kernel (WMD_WGRAD_SMALLCO=1): H in {2, 9, 37} (one slab, several slabs), W in {2, 21, 300} (300 columns
    are more than the block's 256 threads)"""
    monkeypatch.setenv("WMD_WGRAD_SMALLCO", "1")
    for H in (2, 9, 37):
        for W in (2, 21, 300):
            p = _problem(dev, (2, 6, 0, 1, cout, H, W, 3, pad), "C")
            sweep(p, "conv_wgrad_smallco_kernel", 0, [0], cout * 6 * 9 + cout)


# ---- D. the committed choices at their own batch -----------------------------------------------------------------------------
WGRAD_COMMITTED = [(k, v) for k, v in committed_entries() if k.startswith("wgrad|")]
LARGE_1X1 = [
    # 1x1 layers at level-1 sizes, where the library's plan takes large pixel splits (nsplit >= 49: the reduce's 4-deep loop)
    ("wgrad|12|96|320|32|1|0|32|1", ("library", 0)),
    ("wgrad|8|160|512|32|1|0|32|1", ("library", 0)),
]


def test_gemm_oracle_equals_autograd_oracle():
    """the GEMM form that section D uses against autograd of the oracle, 3x3 in every pad mode with an upsampled x1 and a skip
    tensor, and 1x1"""
    g = torch.Generator().manual_seed(7)
    for up, C2, k, pad in ((2, 5, 3, "reflect"), (2, 5, 3, "replicate"), (1, 0, 3, "zero"), (1, 5, 1, "zero")):
        x1 = torch.randn((2, 6, 10 // up, 14 // up), generator=g)
        x2 = torch.randn((2, C2, 10, 14), generator=g) if C2 else None
        dz = torch.randn((2, 7, 10, 14), generator=g)
        aw, ab = autograd_oracle(x1, x2, dz, up, k, pad)
        gw, gb = gemm_oracle(x1, x2, dz, up, k, pad)
        assert _err(gw, aw) < 1e-12 and _err(gb, ab) < 1e-12, (up, C2, k, pad)


@pytest.mark.parametrize("key,choice", WGRAD_COMMITTED + LARGE_1X1, ids=[k for k, _ in WGRAD_COMMITTED + LARGE_1X1])
def test_wgrad_choice_at_its_own_batch_vs_oracle(dev, key, choice):
    """What bench.py runs: each committed wgrad| choice (library -> 0, direct -> -1, a table name -> its entry) at the key's own
    B, H, W and channels with tune_nsplit = 0 (the planner's split, recorded from the workspace), reflect padding, against the
    float64 GEMM oracle on channel subsets (dW[co, ci] depends on dz[co] and x[ci] only: the subset's values are exact)"""
    from wavelet_monodepth_amd import _lib
    B, H, W, C1, up, C2, Cout, k = (int(v) for v in key.split("|")[1:9])
    label, ks = choice
    assert ks == 0, "%s: the weight gradient's committed split is the planner's" % key
    names = wino_names()
    cfg = {"library": 0, "direct": -1}.get(label)
    if cfg is None:
        assert label in names, "%s: %s is not in the weight-gradient table" % (key, label)
        cfg = names.index(label) + 1
    pad, Cin = "reflect", C1 + C2
    g = torch.Generator(device=dev).manual_seed(zlib.crc32(key.encode()))
    x1 = torch.randn((B, C1, H // up, W // up), generator=g, device=dev)
    x2 = torch.randn((B, C2, H, W), generator=g, device=dev) if C2 else None
    dz = torch.randn((B, Cout, H, W), generator=g, device=dev)
    nan = float("nan")
    dw = torch.full((Cout, Cin, k, k), nan, device=dev)
    db = torch.full((Cout,), nan, device=dev)
    a = _lib.ConvWgradArgs(B=B, H=H, W=W, C1=C1, up1=up, C2=C2, Cout=Cout, ksize=k, pad_mode=_lib.PAD[pad], x1=x1.data_ptr(),
                           x2=None if x2 is None else x2.data_ptr(), dz=dz.data_ptr(), dw=dw.data_ptr(), dbias=db.data_ptr(),
                           workspace=None, workspace_floats=0, tune_cfg=cfg, tune_nsplit=0)
    l = _lib.lib()
    n = l.wmd_conv_wgrad_workspace_floats(C.byref(a))
    ws = torch.full((max(n, 1),), nan, device=dev)
    a.workspace, a.workspace_floats = ws.data_ptr(), n
    _lib.profile_begin()
    st = l.wmd_conv_wgrad(C.byref(a), torch.cuda.current_stream().cuda_stream)
    kernels = [r["kernel"] for r in _lib.profile_end()]
    what = "%s -> %s" % (key, label)
    _lib.check(st, what)
    kernel = [kn for kn in kernels if kn.startswith("conv_wgrad_")]
    assert len(kernel) == 1, "%s: launched %s" % (what, kernels)
    kernel = kernel[0]
    if cfg > 0:
        assert kernel == label, "%s: ran %s" % (what, kernel)
    elif cfg < 0:
        assert kernel.startswith("conv_wgrad_kernel<"), "%s: ran %s" % (what, kernel)
    per_split = (16 if kernel.startswith("conv_wgrad_wino") else k * k) * Cout * Cin + Cout
    assert n % per_split == 0, "%s: workspace of %d floats is not whole slices" % (what, n)
    nsplit = n // per_split
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all()), "%s: non-finite dW / db" % what
    co, ci = channel_subset(Cout, key + "|o"), channel_subset(Cin, key + "|i")
    s1, s2 = [c for c in ci if c < C1], [c - C1 for c in ci if c >= C1]
    rw, rb = gemm_oracle(x1[:, s1].cpu(), x2[:, s2].cpu() if s2 else None, dz[:, co].cpu(), up, k, pad)
    ew, eb = _err(dw[co][:, ci], rw), _err(db[co], rb)
    PLANNED[key] = (kernel, nsplit, ew, eb)
    print("%s: %s nsplit %d, dW max rel err %.2e, db %.2e" % (key, kernel, nsplit, ew, eb))
    assert ew <= TOL, "%s: dW[%d x %d channels] max relative error %.3e (nsplit %d)" % (what, len(co), len(ci), ew, nsplit)
    assert eb <= TOL, "%s: db max relative error %.3e (nsplit %d)" % (what, eb, nsplit)
    if key in dict(LARGE_1X1):
        assert nsplit >= 49, "%s: the plan split %d ways; the case is meant for the reduce's 4-deep loop" % (what, nsplit)


# ---- F. coverage ---------------------------------------------------------------------------------------------------------------
def test_every_wgrad_entry_met_the_oracle():
    """(runs after the sweeps above, in file order) every entry of both tables met the oracle with nsplit > 16 and with an empty
    trailing split; every family was compared"""
    print("wgrad (entry, split) pairs compared per family: %s" % ", ".join("%s %d" % (f, len(COMPARED[f])) for f in FAMILIES))
    for key in sorted(PLANNED):
        print("  %s: %s nsplit %d, dW %.2e, db %.2e" % ((key,) + PLANNED[key]))
    missing = [f for f in FAMILIES if not COMPARED[f]]
    assert not missing, "families never compared (run the whole module): %s" % missing
    entries = wino_names() + direct_names()
    seen = {n for f in FAMILIES for n, _ in COMPARED[f]}
    assert not [n for n in entries if n not in seen], "entries never compared: %s" % [n for n in entries if n not in seen]
    assert not [n for n in entries if n not in BIG_SPLIT], "never compared with nsplit > 16: %s" % [n for n in entries if n not in BIG_SPLIT]
    assert not [n for n in entries if n not in EMPTY_TAIL], "never compared with an empty trailing split: %s" % [
        n for n in entries if n not in EMPTY_TAIL]
