"""wmd_conv_wino44_fwd (wmd_conv_wino44.hip) held to the float64 contract of wino44_ref.py pass by pass: the weight image of
wino44_pack_kernel, V after wino44_input_kernel, M after wino44_gemm_kernel, y after wino44_output_kernel, and y end to end, on
every row of tests/wino44_cases.py.

One launch per case through ctypes.  U, the workspace (exactly the reported size) and y are views inside NaN-filled buffers with a
guard band on each side (pin_harness.Bufs).  The passes hand over through the workspace -- V, then M -- so after the launch each
pass is compared alone, against the float64 statement of that pass applied to what the device itself handed it:
    U    elementwise: within one float32 ulp of G g G^T in float64, exact zeros in the padding and at the 11 positions an upsampled
         operand does not reach
    V    per position, against B^T d B of the inputs
    M    per position, against the product of the device's own U and V over the kernel's reduction range of that position
    Y    against act(A^T M A + bias) of the device's own M
    E2E  against the direct convolution; oracle32 is the three passes in float32 (wino44_ref.three_pass_f32)
V and M are compared position by position because the 36 positions differ in scale by two orders of magnitude: the denominator
is the position's own max |oracle64|.  A position whose float64 image is identically zero has no scale of its own: M must then be
exactly 0 (a sum of products with exact zeros), and V must stay under 4 * 2^-23 of |B^T| |d| |B| at that position -- (4a - 5a) + a
of a line that clamping made constant is a rounding residue in float32, not 0, and each of the two line transforms is a sum of at
most three products whose rounding errors that scale bounds.

Tolerances are measured, not chosen: e_hip <= F[kind] * e_ref + 4 * 2^-23 with
    e_ref = max |oracle32 - oracle64| / max |oracle64|,   e_hip = max |hip - oracle64| / max |oracle64|."""
import ctypes as C

import numpy as np
import pytest
import torch

import pin_harness as P
import wino44_cases as WC
import wino44_ref as W
from pin_harness import Bufs, untouched, written

pytestmark = pytest.mark.gpu

# per kind, the smallest power of two >= twice the largest need_F of one full run on the MI355X (profiles/wino44_pins.md); 1 where
# no comparison of the kind leaves the floor
F = {"V": 4, "M": 2, "Y": 4, "E2E": 4}
assert max(F.values()) <= 16
NAMES = {"wino44_input_kernel": 1, "wino44_gemm_kernel": 1, "wino44_output_kernel": 1}
RAN = set()
_MEMO = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def oracles(c):
    """the float64 / float32 side that does not depend on what the device computed, once per case"""
    def make():
        x1, w, b, x2 = WC.operands(c)
        V64, un = W.input_image(x1, x2, c["up1"], c["pad"])
        V32, _ = W.input_image(x1, x2, c["up1"], c["pad"], np.float32)
        scale, _ = W.input_image(x1, x2, c["up1"], c["pad"], absolute=True)
        y64 = W.activate(W.direct(x1, w, b, x2=x2, up1=c["up1"], pad=c["pad"]), c["act"], c["slope"])
        y32 = W.three_pass_f32(x1, w, b, x2, c["up1"], c["pad"], c["act"], c["slope"])
        return dict(U64=W.weight_image(w, c["C1"], c["up1"]), V64=V64, V32=V32, un=un, scale=scale.reshape(36, -1).max(1), y64=y64, y32=y32)
    return memo(c["key"], make)


def launch(dev, c, k):
    """pack + one wmd_conv_wino44_fwd into guarded NaN buffers -> U, workspace, y views and their Bufs; asserts the launch set"""
    from wavelet_monodepth_amd import _lib, ops
    l = _lib.lib()
    d = W.dims(c["B"], c["H"], c["W"], c["C1"], c["C2"], c["Cout"])
    a = ops._conv_args(c["B"], c["H"], c["W"], c["C1"], c["up1"], c["C2"], c["Cout"], 3, c["pad"], c["act"], c["slope"])
    assert l.wmd_conv_wino44_supported(C.byref(a)) == 1, l.wmd_last_error()
    n = l.wmd_conv_wino44_workspace_floats(C.byref(a))
    assert n == d.v_floats + d.m_floats and l.wmd_conv_packed_weight_floats_wino44(c["Cout"], c["C1"], c["C2"]) == d.u_floats
    bufs = Bufs(dev)
    U, ws, y = bufs.new("U", d.u_floats), bufs.new("the workspace", n), bufs.new("y", c["B"], c["Cout"], c["H"], c["W"])
    assert U.data_ptr() % 16 == 0 and ws.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    stream = torch.cuda.current_stream().cuda_stream
    _lib.profile_begin()
    _lib.check(l.wmd_conv_pack_weights_wino44(k["w"].data_ptr(), U.data_ptr(), c["Cout"], c["C1"], c["C2"], c["up1"], stream), "wmd_conv_pack_weights_wino44")
    ran = {r["kernel"]: r["calls"] for r in _lib.profile_end()}
    assert ran == {"wino44_pack_kernel": 1}, "%s: the pack's profile shows %s" % (c["key"], ran)
    a.x1, a.x2, a.wp, a.y = k["x1"].data_ptr(), None if k["x2"] is None else k["x2"].data_ptr(), U.data_ptr(), y.data_ptr()
    a.bias = None if k["b"] is None else k["b"].data_ptr()
    a.workspace, a.workspace_floats = ws.data_ptr(), n
    _lib.profile_begin()
    _lib.check(l.wmd_conv_wino44_fwd(C.byref(a), stream), "wmd_conv_wino44_fwd")
    ran = {r["kernel"]: r["calls"] for r in _lib.profile_end()}
    torch.cuda.synchronize()
    assert ran == NAMES, "%s: the profile shows %s, expected %s" % (c["key"], ran, NAMES)
    return U, ws, y, bufs


def to_dev(dev, c):
    x1, w, b, x2 = WC.operands(c)
    return {n: None if v is None else torch.from_numpy(v).to(dev).contiguous() for n, v in (("x1", x1), ("w", w), ("b", b), ("x2", x2))}


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def check_u(c, d, Ud, U64):
    """in double, rounded once: within one float32 ulp where an entry is live, exactly 0 elsewhere (channel-major images)"""
    live = np.zeros(U64.shape, bool)
    live[:, :c["C1"], :c["Cout"]] = True
    live[:, d.C1p:d.C1p + c["C2"], :c["Cout"]] = True
    if c["up1"] == 2:
        live[list(W.SHORT), :d.C1p] = False
    assert np.isfinite(Ud).all(), "%s: U has elements the pack never wrote" % c["key"]
    assert not Ud[~live].any(), "%s: U is not exactly 0 in its padding / at the positions an upsampled operand does not reach" % c["key"]
    ulp = np.spacing(np.abs(U64.astype(np.float32))).astype(np.float64)
    worst = float((np.abs(Ud.astype(np.float64) - U64)[live] / ulp[live]).max())
    print("EDGE %-9s %-34s %-16s worst %.3f ulp" % ("U", c["key"], "live entries", worst))
    assert worst <= 1.0, "%s: U is %.3f float32 ulp from G g G^T in float64" % (c["key"], worst)


def run_case(dev, key):
    c = WC.CASES[key]
    o = oracles(c)
    d = W.dims(c["B"], c["H"], c["W"], c["C1"], c["C2"], c["Cout"])
    k = to_dev(dev, c)
    U, ws, y, bufs = launch(dev, c, k)
    bufs.bands(key)
    written(y, key + ": y")
    wsd = ws.cpu().numpy()
    Ud = W.unpack4(U.cpu().numpy().reshape(36, d.Ktot // 4, d.Coutp, 4))
    Vd = W.unpack4(wsd[:d.v_floats].reshape(36, d.Ktot // 4, d.NTp, 4))
    Md = wsd[d.v_floats:].reshape(36, d.Coutp, d.NTp)
    yd = y.cpu().numpy()
    chk = P.Checks(key, F)
    un, kept = o["un"], ~o["un"]

    check_u(c, d, Ud, o["U64"])

    # V: the input pass alone
    untouched(torch.from_numpy(Vd[un]), key + ": the 11 positions of an upsampled operand's channels in V")
    written(torch.from_numpy(Vd[kept]), key + ": V")
    dead = kept.copy()
    dead[:, :c["C1"], :d.NT] = False
    dead[:, d.C1p:d.C1p + c["C2"], :d.NT] = False
    assert not Vd[dead].any(), "%s: dead channels / dead tiles of V are not exactly 0" % key
    for p in range(36):
        kp = kept[p]
        if not kp.any():
            continue
        if not o["V64"][p][kp].any():
            worst = float(np.abs(Vd[p][kp]).max())
            assert worst <= P.FLOOR * o["scale"][p], "%s: V at position %d should be 0, is %.3e (scale %.3e)" % (key, p, worst, o["scale"][p])
            continue
        chk.add("V", "p%02d" % p, torch.from_numpy(Vd[p]), t64(o["V32"][p]), t64(o["V64"][p]), keep=torch.from_numpy(kp))

    # M: the GEMM alone, from the device's own U and V
    M64 = W.product(Ud, Vd, c["up1"], d.C1p, un)
    M32 = W.product(Ud, Vd, c["up1"], d.C1p, un, np.float32)
    live_m = Md[:, :c["Cout"], :d.NT]
    assert np.isfinite(live_m).all(), "%s: M has live elements no GEMM block wrote (or that read the untouched part of V)" % key
    if c["up1"] == 2 and c["C2"] == 0:
        assert not live_m[list(W.SHORT)].any(), "%s: M is not exactly 0 at the 11 positions without a chunk" % key
    for p in range(36):
        m64 = M64[p, :c["Cout"], :d.NT]
        if not m64.any():
            assert not live_m[p].any(), "%s: M at position %d is a sum of exact zeros and is not 0" % (key, p)
            continue
        chk.add("M", "p%02d" % p, torch.from_numpy(np.ascontiguousarray(live_m[p])), t64(M32[p, :c["Cout"], :d.NT]), t64(m64))

    # Y: the output pass alone, from the device's own M
    b = WC.operands(c)[2]
    geo = (c["B"], c["H"], c["W"], c["Cout"], c["act"], c["slope"])
    chk.add("Y", "y | M", torch.from_numpy(yd), t64(W.output_image(Md, b, *geo, dtype=np.float32)), t64(W.output_image(Md, b, *geo)))
    chk.add("E2E", "y", torch.from_numpy(yd), t64(o["y32"]), t64(o["y64"]))

    if key in WC.REPEAT:
        U2, ws2, y2, bufs2 = launch(dev, c, k)
        bufs2.bands(key + ", second launch")
        for name, t1, t2 in (("U", U, U2), ("V and M", ws, ws2), ("y", y, y2)):
            assert torch.equal(t1.view(torch.int32), t2.view(torch.int32)), "%s: %s differs between two launches" % (key, name)
    RAN.add(key)
    chk.done()


@pytest.mark.parametrize("key", WC.KEYS)
def test_wino44_passes_vs_oracle(dev, key):
    run_case(dev, key)


def test_every_case_ran(dev):
    """(a partial run of the module first runs the rows it has not run)"""
    for key in WC.KEYS:
        if key not in RAN:
            run_case(dev, key)
    assert RAN == set(WC.KEYS)
