"""The wavelet heads' backward kernels (wmd_head_bwd.hip, wmd_head_bwd1.h, wmd_head_bwd1.hip) held against the float64 oracle of
head_bwd_ref.py, kernel by kernel: head3x3_bwd_{data,weight,reduce}_kernel<1|3>, head1x1_bwd_{data,weight,reduce}_kernel,
head_bwd_stage2_kernel, head_bwd_reduce2_kernel and head_bwd_fused32_kernel.

Every call goes through the C entry with an argument block built here.  Every output is a view inside a NaN-filled buffer with a
guard band on each side (pin_harness.Bufs): a store outside an output shows in the bands, an element never written in the output,
and what the contract leaves alone (channels of no head, dzmid of the fused form, everything of a refused call) must still be NaN.
Workspaces are NaN-filled too and hold exactly the floats the matching *_workspace_floats query answers, so a reduce that reads a
partial no block wrote poisons its output.  The launch profile names the kernels that ran; the shape rules that send a row down a
form are re-derived in head_bwd_ref.py and asserted here again.

Tolerances are measured, not chosen: for every compared tensor, on the same inputs,
    e_ref = max |oracle32 - oracle64| / max |oracle64|     the torch-CPU oracle in float32 against itself in float64
    e_hip = max |hip      - oracle64| / max |oracle64|
and the assertion is e_hip <= F[kind] * e_ref + 4 * 2^-23.  No element is excluded: the gate is read off the activation OUTPUT
(an input of these calls), so there is no kink ambiguity."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import head_bwd_ref as HB
import pin_harness as P
from pin_harness import GUARD, NAN, Bufs, untouched, written

pytestmark = pytest.mark.gpu

# per tensor kind, the smallest power of two >= twice the largest need_F measured on the MI355X among the comparisons whose e_hip
# exceeds the floor (profiles/head_bwd_pins.md; the table and the case that set each entry are in DESIGN.md §4.6.4); 1 where no
# comparison of the kind exceeds the floor.  Measured: dz, dw1, db1 never above the floor; dw3 0.27, db3 0.32, dx 0.13 -> 1 each
F = {"dz": 1, "dw3": 1, "db3": 1, "dx": 1, "dw1": 1, "db1": 1}
assert max(F.values()) <= 16
SWITCHES = ("WMD_HEAD_CHAIN", "WMD_HEAD_CHAIN_MULTI", "WMD_HEAD_CHAIN_PG256", "WMD_HEAD_STREAM", "WMD_HEAD_STREAM_TH", "WMD_HEAD_STREAM_MIN_PIXELS",
            "WMD_SHIFTSUM_CHAIN_SQUARE", "WMD_HEAD_CSPLIT", "WMD_HEAD_NG", "WMD_HEAD_BWD_FUSED")    # test_host_logic._HEAD_SWITCH_NAMES
FUSED_SWITCH = os.environ.get("WMD_HEAD_BWD_FUSED", "1").strip() not in ("0", "")
BAD_SHAPE, UNSUPPORTED = -2, -3
K3 = ("head3x3_bwd_data_kernel", "head3x3_bwd_weight_kernel", "head3x3_bwd_reduce_kernel")
K1 = ("head1x1_bwd_data_kernel", "head1x1_bwd_weight_kernel", "head1x1_bwd_reduce_kernel")
THREE = {"head3x3_bwd_data_kernel": 1, "head_bwd_stage2_kernel": 1, "head_bwd_reduce2_kernel": 1}
FUSED = {"head_bwd_fused32_kernel": 1, "head_bwd_reduce2_kernel": 1}


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


def launch(fn, what, *args):
    """-> (status, {kernel name: launches}); a refused call launched nothing"""
    from wavelet_monodepth_amd import _lib
    _lib.profile_begin()
    st = fn(*[C.byref(a) for a in args], torch.cuda.current_stream().cuda_stream)
    prof = _lib.profile_end()
    return st, {r["kernel"]: r["calls"] for r in prof}


def nothing_happened(bufs, wss, what):
    for name, buf, _n in bufs.items:
        untouched(buf, "%s: %s of a refused call" % (what, name))
    for ws in wss:
        untouched(ws, what + ": the workspace of a refused call")


_ORACLES, _CASES = {}, {}


def oracle(key, fn):
    """(float32, float64) oracle results, computed once per key and left unchanged"""
    if key not in _ORACLES:
        _ORACLES[key] = (fn(torch.float32), fn(torch.float64))
    return _ORACLES[key]


def memo(key, fn):
    if key not in _CASES:
        _CASES[key] = fn()
    return _CASES[key]


def on_device(dev, c, names):
    """the operands of a case on the device, 16-byte aligned allocations of their own, memoised on the case"""
    if "dev" not in c:
        c["dev"] = {}
    for n in names:
        if n not in c["dev"]:
            v = c[n]
            c["dev"][n] = [e.to(dev).contiguous() for e in v] if isinstance(v, list) else v.to(dev).contiguous()
    return c["dev"]


def case3(shape, layout, act):
    B, H, W = shape
    return memo(("3", shape, str(layout), act), lambda: HB.case3x3("A%s%s%s" % (shape, layout, act), B, H, W, layout["Ct"], layout["n_out"], layout["heads"], act))


def case1(shape, Cc, Ct, x_act, dz=True):
    B, H, W = shape
    return memo(("1", shape, Cc, Ct, x_act, dz), lambda: HB.case1x1("B%s%d,%d%s" % (shape, Cc, Ct, x_act), B, H, W, Cc, Ct, x_act, dz))


def workspace(dev, a, query, floats=None):
    """a NaN-filled workspace of exactly the floats the query answers (or `floats`), GUARD more behind it -> (buffer, the answer)"""
    n = query(C.byref(a))
    have = n if floats is None else floats
    ws = torch.full((have + GUARD,), NAN, device=dev)
    a.workspace, a.workspace_floats = ws.data_ptr(), have
    assert ws.data_ptr() % 16 == 0
    return ws, n


def args3x3(dev, c, pad, bufs):
    from wavelet_monodepth_amd import _lib
    k = on_device(dev, c, ("dy3", "mid", "w3"))
    o = dict(dz=bufs.new("dzmid", c["B"], c["Ct"], c["H"], c["W"]), dw3=[], db3=[])
    a = _lib.Head3x3BwdArgs(B=c["B"], H=c["H"], W=c["W"], Ct=c["Ct"], n_out=c["n_out"], pad_mode=_lib.PAD[pad], act=_lib.ACT[c["act"]], slope=HB.SLOPE,
                            dy3=ptr(k["dy3"]), mid=ptr(k["mid"]), dzmid=ptr(o["dz"]), n_heads=len(c["heads"]), workspace=None, workspace_floats=0)
    for i, (row0, nrows, ch0, nch) in enumerate(c["heads"]):
        o["dw3"].append(bufs.new("dw3[%d]" % i, nrows, nch, 3, 3))
        o["db3"].append(bufs.new("db3[%d]" % i, nrows))
        a.head[i] = _lib.HeadBwdHead(row0=row0, nrows=nrows, ch0=ch0, nch=nch, w3=ptr(k["w3"][i]), dw3=ptr(o["dw3"][i]), db3=ptr(o["db3"][i]))
    for v in (k["dy3"], k["mid"], o["dz"]):
        assert v.data_ptr() % 16 == 0
    return a, o


def args1x1(dev, c, bufs, with_dx=True, dz=None):
    from wavelet_monodepth_amd import _lib
    k = on_device(dev, c, ("x", "w1") + (("dz",) if dz is None else ()))
    o = dict(dx=bufs.new("dx", c["B"], c["C"], c["H"], c["W"]) if with_dx else None, dw1=bufs.new("dw1", c["Ct"], c["C"]), db1=bufs.new("db1", c["Ct"]))
    dz = k["dz"] if dz is None else dz
    a = _lib.Head1x1BwdArgs(B=c["B"], H=c["H"], W=c["W"], C=c["C"], Ct=c["Ct"], x_act=_lib.ACT[c["x_act"]], x_slope=HB.SLOPE, dz=ptr(dz), x=ptr(k["x"]),
                            w1=ptr(k["w1"]), dx=ptr(o["dx"]), dw1=ptr(o["dw1"]), db1=ptr(o["db1"]), workspace=None, workspace_floats=0)
    for v in (dz, k["x"], o["dx"]):
        assert v is None or v.data_ptr() % 16 == 0
    return a, o


def compare3x3(dev, chk, what, c, o, o32, o64, dz=True):
    """dz (per head; channels of no head untouched), dw3 and db3 of every head against the oracle"""
    own = torch.zeros(c["Ct"], dtype=torch.bool)
    for i, (_row0, _nrows, ch0, nch) in enumerate(c["heads"]):
        sl = slice(ch0, ch0 + nch)
        own[sl] = True
        if dz:
            written(o["dz"][:, sl], "%s: dz of head %d" % (what, i))
            chk.add("dz", "%s dz[%d]" % (what, i), o["dz"][:, sl], o32["dz"][:, sl], o64["dz"][:, sl])
        written(o["dw3"][i], "%s: dw3 of head %d" % (what, i))
        written(o["db3"][i], "%s: db3 of head %d" % (what, i))
        chk.add("dw3", "%s dw3[%d]" % (what, i), o["dw3"][i], o32["dw3"][i], o64["dw3"][i])
        chk.add("db3", "%s db3[%d]" % (what, i), o["db3"][i], o32["db3"][i], o64["db3"][i])
    if not dz:
        untouched(o["dz"], what + ": dzmid of the fused form")
    elif not bool(own.all()):
        untouched(o["dz"][:, (~own).to(dev)], what + ": dzmid channels of no head")


def compare1x1(chk, what, o, o32, o64):
    for name in ("dx", "dw1", "db1"):
        if o[name] is not None:
            written(o[name], "%s: %s" % (what, name))
            chk.add(name, "%s %s" % (what, name), o[name], o32[name], o64[name])


# ---- A. wmd_head3x3_bwd: head3x3_bwd_{data,weight,reduce}_kernel<1|3> --------------------------------------------------------------
def run3x3(dev, chk, shape, name, pad, act, status=0):
    from wavelet_monodepth_amd import _lib
    l = _lib.lib()
    layout = HB.LAYOUTS[name]
    c = case3(shape, layout, act)
    what = "%dx%dx%d %s %s %s" % (shape + (name, pad, act))
    bufs = Bufs(dev)
    a, o = args3x3(dev, c, pad, bufs)
    ws, n = workspace(dev, a, l.wmd_head3x3_bwd_workspace_floats)
    st, kernels = launch(l.wmd_head3x3_bwd, what, a)
    assert st == status, "%s: status %d (%s)" % (what, st, l.wmd_last_error().decode())
    if status:
        assert n == 0 and kernels == {}, "%s: a refused call answered %d workspace floats and launched %s" % (what, n, kernels)
        nothing_happened(bufs, [ws], what)
        return
    assert n == HB.workspace3x3(*shape, layout["heads"])[0], "%s: %d workspace floats" % (what, n)
    kinds = len({h[1] for h in layout["heads"]})      # one launch set per head kind: <3>, then <1>
    assert kernels == {k: kinds for k in K3}, "%s: the profile shows %s" % (what, kernels)
    bufs.bands(what)
    untouched(ws[n:], what + ": past the workspace")
    o32, o64 = oracle(("3", shape, name, pad, act), lambda dt: HB.oracle3x3(c, pad, dt))
    compare3x3(dev, chk, what, c, o, o32, o64)


@pytest.mark.parametrize("row", range(len(HB.A_TABLE)), ids=["x".join(map(str, r[0])) for r in HB.A_TABLE])
def test_head3x3_bwd_vs_oracle(dev, row):
    """Every row of the table under all three paddings (one row / one column: zero and replicate; reflection there is refused with
    WMD_ERR_BAD_SHAPE and launches nothing), the activation rotating over none / leaky(0.1) / ELU, crossed with the head layouts:
    nch 8, 20, 64, 80 (two slices), [LL, +, -] over 7 rows in two orders, one head alone (3-row and 1-row), channels of no head."""
    shape, why, _layouts = HB.A_TABLE[row]
    assert HB.row_reaches(shape, why) == [], "%s no longer reaches %s" % (shape, HB.row_reaches(shape, why))
    chk = Checks("A %dx%dx%d" % shape)
    runs = [r for r in HB.a_runs() if r[0] == shape]
    for _s, name, pad, act in runs:
        run3x3(dev, chk, shape, name, pad, act)
    if min(shape[1:]) < 2:
        assert all(pad != "reflect" for _s, _n, pad, _a in runs)
        run3x3(dev, chk, shape, runs[0][1], "reflect", "leaky", status=BAD_SHAPE)
    chk.done()


@pytest.mark.parametrize("tiles", HB.REDUCE3_TILES)
def test_head3x3_bwd_reduce_with_empty_and_uneven_quarters(dev, tiles):
    """1, 2, 3, 5, 9 and 17 tiles (frames of 4 x 16): 1, 1, 1, 2, 3 and 5 blocks of partials, some of them with idle waves, for a
    reduce that splits the blocks four ways -- on a workspace whose unwritten floats are NaN."""
    assert HB.classify(tiles, 4, 16)["tiles"] == tiles
    chk = Checks("A reduce %d tiles" % tiles)
    for i, name in enumerate(("n20", "ll")):
        run3x3(dev, chk, (tiles, 4, 16), name, HB.PADS[(tiles + i) % 3], HB.ACTS[(tiles + 2 * i) % 3])
    chk.done()


def test_head3x3_bwd_slice_limit(dev):
    """three heads of 512 channels: 24 slices, the limit, accepted; 25: WMD_ERR_UNSUPPORTED, nothing launched"""
    chk = Checks("A slices")
    run3x3(dev, chk, (1, 2, 2), "s24", "reflect", "leaky")
    run3x3(dev, chk, (1, 2, 2), "s24", "replicate", "elu")
    run3x3(dev, chk, (1, 2, 2), "s25", "reflect", "leaky", status=UNSUPPORTED)
    chk.done()


# ---- B. wmd_head1x1_bwd: head1x1_bwd_{data,weight,reduce}_kernel -------------------------------------------------------------------
def run1x1(dev, chk, shape, Cc, Ct, x_act, with_dx=True, status=0):
    from wavelet_monodepth_amd import _lib
    l = _lib.lib()
    c = case1(shape, Cc, Ct, x_act)
    what = "%dx%dx%d C%d Ct%d %s%s" % (shape + (Cc, Ct, x_act, "" if with_dx else " no-dx"))
    bufs = Bufs(dev)
    a, o = args1x1(dev, c, bufs, with_dx)
    ws, n = workspace(dev, a, l.wmd_head1x1_bwd_workspace_floats)
    st, kernels = launch(l.wmd_head1x1_bwd, what, a)
    assert st == status, "%s: status %d (%s)" % (what, st, l.wmd_last_error().decode())
    if status:
        assert n == 0 and kernels == {}, "%s: a refused call answered %d workspace floats and launched %s" % (what, n, kernels)
        nothing_happened(bufs, [ws], what)
        return
    assert n == HB.workspace1x1(*shape, Cc, Ct), "%s: %d workspace floats" % (what, n)
    assert kernels == {k: 1 for k in (K1 if with_dx else K1[1:])}, "%s: the profile shows %s" % (what, kernels)
    bufs.bands(what)
    untouched(ws[n:], what + ": past the workspace")
    o32, o64 = oracle(("1", shape, Cc, Ct, x_act), lambda dt: HB.oracle1x1(c, dt))
    compare1x1(chk, what, o, o32, o64)


@pytest.mark.parametrize("j", range(len(HB.B_CHANNELS)), ids=["C%d_Ct%d" % v for v in HB.B_CHANNELS])
def test_head1x1_bwd_vs_oracle(dev, j):
    """(C, Ct) with last channel groups of 2 and 8 and up to 3 x 3 channel-group pairs, on the scalar path, the 16-byte path with a
    ragged tile, one whole tile and whole tiles; x_act rotating; dx == NULL: no data kernel, dw1 and db1 still right."""
    Cc, Ct = HB.B_CHANNELS[j]
    chk = Checks("B C%d Ct%d" % (Cc, Ct))
    for i, shape in enumerate(HB.B_SHAPES):
        run1x1(dev, chk, shape, Cc, Ct, HB.ACTS[(i + j) % 3])
    for i in (j % 4, (j + 1) % 4):
        run1x1(dev, chk, HB.B_SHAPES[i], Cc, Ct, HB.ACTS[(i + j) % 3], with_dx=False)
    chk.done()


@pytest.mark.parametrize("k", range(len(HB.B_WRAPS)), ids=["x".join(map(str, r[0])) for r in HB.B_WRAPS])
def test_head1x1_bwd_persistent_loops_wrap(dev, k):
    """2051 tiles: the weight stage's 512 x 4 waves wrap, remainder 3; 16387: the data stage's 4096 x 4, remainder 3"""
    shape, why = HB.B_WRAPS[k]
    assert HB.row_reaches(shape, why) == [], "%s no longer reaches %s" % (shape, why)
    chk = Checks("B %dx%dx%d" % shape)
    run1x1(dev, chk, shape, 8, 8, HB.ACTS[k + 1])
    run1x1(dev, chk, shape, 8, 8, HB.ACTS[k + 1], with_dx=False)
    chk.done()


@pytest.mark.parametrize("tiles", HB.REDUCE1_TILES)
def test_head1x1_bwd_reduce_with_empty_sixteenths(dev, tiles):
    """1, 3, 17 and 33 tiles: 1, 1, 5 and 9 blocks of partials for a reduce that splits them sixteen ways; 2 x 2 channel-group pairs"""
    chk = Checks("B reduce %d tiles" % tiles)
    run1x1(dev, chk, (tiles, 4, 16), 80, 72, HB.ACTS[tiles % 3], with_dx=tiles % 2 == 1)
    chk.done()


def test_head1x1_bwd_refuses_ct_12(dev):
    run1x1(dev, None, (2, 5, 7), 8, 12, "elu", status=UNSUPPORTED)


# ---- C, D. wmd_head_bwd: head_bwd_stage2_kernel + head_bwd_reduce2_kernel, head_bwd_fused32_kernel -----------------------------------
def run_both(dev, chk, shape, layout, tag, pad, act, x_act, Cc, with_dx=True, ws3_floats=None, expect=None, status=0, separate=True):
    """one wmd_head_bwd call against the oracle of both stages; the three-launch form also bit for bit against wmd_head3x3_bwd
    followed by wmd_head1x1_bwd on the same inputs.  ws3_floats: "fused-1": a 3x3 workspace one float short of the fused need"""
    from wavelet_monodepth_amd import _lib
    l = _lib.lib()
    c3, c1 = case3(shape, layout, act), case1(shape, Cc, layout["Ct"], x_act, dz=False)
    what = "%dx%dx%d %s %s %s x:%s%s%s" % (shape + (tag, pad, act, x_act, "" if with_dx else " no-dx", "" if ws3_floats is None else " ws3 short"))
    admitted = HB.head_bwd_fused_ok(*shape, layout["heads"], layout["Ct"], Cc, pad, with_dx, FUSED_SWITCH)
    q3, need3, fused3 = HB.workspace3x3(*shape, layout["heads"])
    if ws3_floats == "fused-1":
        assert admitted and need3 <= fused3 - 1, what
        ws3_floats, admitted = fused3 - 1, False
    if expect is not None:
        assert admitted == (expect == "fused"), "%s: the case no longer reaches the %s form" % (what, expect)

    def call(fns, bufs):
        a3, o3 = args3x3(dev, c3, pad, bufs)
        a1, o1 = args1x1(dev, c1, bufs, with_dx, dz=o3["dz"])
        ws3, n3 = workspace(dev, a3, l.wmd_head3x3_bwd_workspace_floats, ws3_floats)
        ws1, n1 = workspace(dev, a1, l.wmd_head1x1_bwd_workspace_floats)
        if fns is None:
            st, kernels = launch(l.wmd_head_bwd, what, a3, a1)
        else:
            st, k3 = launch(l.wmd_head3x3_bwd, what, a3)
            assert st == 0, "%s: wmd_head3x3_bwd: status %d" % (what, st)
            st, k1 = launch(l.wmd_head1x1_bwd, what, a1)
            kernels = dict(k3, **k1)
        return st, kernels, o3, o1, (ws3, n3, ws1, n1)

    bufs = Bufs(dev)
    st, kernels, o3, o1, (ws3, n3, ws1, n1) = call(None, bufs)
    assert st == status, "%s: status %d (%s)" % (what, st, l.wmd_last_error().decode())
    if status:
        assert kernels == {}, "%s: a refused call launched %s" % (what, kernels)
        nothing_happened(bufs, [ws3, ws1], what)
        return
    assert (n3, n1) == (q3, HB.workspace1x1(*shape, Cc, layout["Ct"])), "%s: %d and %d workspace floats" % (what, n3, n1)
    assert kernels == (FUSED if admitted else THREE), "%s: the profile shows %s" % (what, kernels)
    bufs.bands(what)
    untouched(ws3[ws3.numel() - GUARD:], what + ": past the 3x3 workspace")
    untouched(ws1[n1:], what + ": past the 1x1 workspace")
    o32, o64 = oracle(("both", shape, tag, pad, act, x_act, Cc), lambda dt: HB.oracle_both(c3, c1, pad, dt))
    compare3x3(dev, chk, what, c3, o3, o32, o64, dz=not admitted)
    compare1x1(chk, what, o1, o32, o64)
    if admitted or not separate:
        return
    # "same arguments and results": the bodies, the block counts of both weight stages and the order of the partials are shared, and a
    # tile's data gradient does not depend on the block that computes it -- so the bits are
    bufs2 = Bufs(dev)
    st, kernels, p3, p1, _ws = call("separate", bufs2)
    assert st == 0 and kernels == {k: 1 for k in K3 + (K1 if with_dx else K1[1:])}, "%s: the separate calls: status %d, %s" % (what, st, kernels)
    bufs2.bands(what + " (separate calls)")
    pairs = [("dzmid", o3["dz"], p3["dz"]), ("dw1", o1["dw1"], p1["dw1"]), ("db1", o1["db1"], p1["db1"])] + ([("dx", o1["dx"], p1["dx"])] if with_dx else [])
    for i in range(len(layout["heads"])):
        pairs += [("dw3[%d]" % i, o3["dw3"][i], p3["dw3"][i]), ("db3[%d]" % i, o3["db3"][i], p3["db3"][i])]
    for name, got, want in pairs:
        assert torch.equal(got, want), "%s: %s differs from wmd_head3x3_bwd + wmd_head1x1_bwd by %.3e" % (what, name, float((got - want).abs().max()))


C_RUNS = [r for r in HB.a_runs() if r[1] in HB.C_LAYOUT_C]
C_ROWS = [i for i, row in enumerate(HB.A_TABLE) if any(r[0] == row[0] for r in C_RUNS)]


@pytest.mark.parametrize("row", C_ROWS, ids=["x".join(map(str, HB.A_TABLE[i][0])) for i in C_ROWS])
def test_head_bwd_three_launch_form_vs_oracle_and_separate_calls(dev, row):
    """The runs of section A whose heads all have three rows and own every channel of mid, together with the 1x1 stage, with and
    without dx: head3x3_bwd_data_kernel + head_bwd_stage2_kernel + head_bwd_reduce2_kernel against the oracle, and bit for bit
    against the two separate calls."""
    shape = HB.A_TABLE[row][0]
    chk = Checks("C %dx%dx%d" % shape)
    for i, (_s, name, pad, act) in enumerate(r for r in C_RUNS if r[0] == shape):
        for with_dx in (True, False):
            run_both(dev, chk, shape, HB.LAYOUTS[name], name, pad, act, HB.ACTS[(i + row) % 3], HB.C_LAYOUT_C[name], with_dx, expect="three")
    chk.done()


def test_head_bwd_stage2_with_three_different_extents(dev):
    """4099 tiles: 256 blocks of the 3x3 weight stage, 512 of the 1x1 weight stage and 1024 of the 1x1 data gradient in one launch,
    every one of their loops wrapping"""
    lp = HB.classify(*HB.C_EXTRA)["loops"]
    assert (lp["w3"]["blocks"], lp["w1"]["blocks"], lp["d_merged"]["blocks"]) == (256, 512, 1024) and min(lp[k]["wraps"] for k in ("w3", "w1", "d_merged")) >= 1
    chk = Checks("C %dx%dx%d" % HB.C_EXTRA)
    for i, (pad, with_dx) in enumerate((("reflect", True), ("replicate", False), ("zero", True))):
        run_both(dev, chk, HB.C_EXTRA, HB.LAYOUTS["n8"], "n8", pad, HB.ACTS[i], HB.ACTS[(i + 1) % 3], 8, with_dx, expect="three")
    chk.done()


def test_head_bwd_refuses_a_low_pass_head(dev):
    run_both(dev, None, (2, 5, 7), HB.LAYOUTS["ll"], "ll", "reflect", "leaky", "elu", 16, status=UNSUPPORTED)


def d_layout(name):
    n_out, heads = HB.D_LAYOUTS[name]
    return dict(Ct=64, n_out=n_out, heads=heads)


def run_fused_shape(dev, k, expect="fused"):
    shape, why = HB.D_SHAPES[k]
    assert HB.row_reaches(shape, why) == [], "%s no longer reaches %s" % (shape, why)
    chk = Checks("D %dx%dx%d" % shape)
    names = list(HB.D_LAYOUTS)
    pairs = [(a, x) for a in HB.ACTS for x in HB.ACTS] if k < 2 else [(HB.ACTS[(k + i) % 3], HB.ACTS[(2 * k + i) % 3]) for i in range(len(names))]
    for i, (act, x_act) in enumerate(pairs):
        name = names[(i + k) % len(names)]
        run_both(dev, chk, shape, d_layout(name), name, "reflect", act, x_act, 32, expect=expect, separate=False)
    chk.done()


@pytest.mark.parametrize("k", range(len(HB.D_SHAPES)), ids=["x".join(map(str, r[0])) for r in HB.D_SHAPES])
def test_head_bwd_fused32_kernel_vs_oracle(dev, k):
    """head_bwd_fused32_kernel: one tile without an inner group, inner groups, groups that straddle rows, and 2051 tiles (the 512
    blocks wrap, remainder 3); all nine (act, x_act) pairs on the first two; ch0 = (0, 32) and (32, 0); n_out = 6 with rows (0, 3),
    7 with rows (1, 4) and (4, 1).  The profile names the kernel, and dzmid is still all NaN."""
    run_fused_shape(dev, k, "fused" if FUSED_SWITCH else "three")


def test_head_bwd_short_workspace_takes_the_three_launch_form(dev):
    """a 3x3 workspace one float short of the fused form's need (but not of the three-launch form's): three launches, right results"""
    chk = Checks("D short workspace")
    run_both(dev, chk, (2051, 4, 16), d_layout("r14"), "r14", "reflect", "leaky", "elu", 32, ws3_floats="fused-1" if FUSED_SWITCH else None, expect="three")
    chk.done()


def test_head_bwd_not_admitted_runs_three_launches(dev):
    """W % 4 != 0, H*W % 64 != 0, zero padding and dx == NULL on otherwise admissible levels: the three-launch form, seen in the profile"""
    chk = Checks("D not admitted")
    for i, (shape, pad, with_dx, why) in enumerate(HB.D_NOT_ADMITTED):
        name = list(HB.D_LAYOUTS)[i]
        run_both(dev, chk, shape, d_layout(name), name + " (" + why + ")", pad, "leaky", "elu", 32, with_dx, expect="three")
    chk.done()


def child_fused_off(dev):    # WMD_HEAD_BWD_FUSED=0: admissible levels on the three-launch form
    assert not FUSED_SWITCH
    for k in (0, 1):
        run_fused_shape(dev, k, expect="three")


_CHILD = "import sys, torch, test_gpu_head_bwd as T; getattr(T, sys.argv[1])(torch.device('cuda:0'))"


def test_fused_switch_off_in_a_child_process():
    """WMD_HEAD_BWD_FUSED=0 is read once per process: a fresh one runs the first two fused shapes, on the three-launch form"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env["WMD_HEAD_BWD_FUSED"] = "0"
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(here), here, env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, "-c", _CHILD, "child_fused_off"], env=env, capture_output=True, text=True, timeout=120)
    print("".join("WMD_HEAD_BWD_FUSED=0 %s\n" % line for line in r.stdout.splitlines() if line.startswith("EDGE")), end="")
    assert r.returncode == 0, "WMD_HEAD_BWD_FUSED=0: exit status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
