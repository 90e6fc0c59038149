"""The plain streaming kernels -- wmd_dwconv.hip, wmd_wavelet.hip, wmd_resample.hip and flip_postprocess_kernel of wmd_eval.hip --
held against the float64 oracle of tests/stream_ref.py at their launch edges.

Every one of them is a grid-stride loop under a block cap; the caps are re-stated below (CAP_*), and for each kernel at least
one case is larger than cap * 256 items, so some thread takes a second trip of the loop (asserted from the case's shape).  The
argument blocks are built here and the C entry points called directly, test_gpu_head_fwd.py's method: every output is a view in a
NaN-filled buffer between guard bands (a store outside an output shows in the bands, an element never written in the output), the
depthwise backward's workspace gets exactly wmd_dwconv3x3_bwd_workspace_floats floats, and the launch profile names what ran.

Tolerances are measured, not chosen: e_hip <= F[kind] * e_ref + 4 * 2^-23 with e_ref the float32 oracle's own error against the
float64 one on the same inputs (tests/pin_harness.py).  Every backward takes its gate from a tensor the entry point is given
(y, out, depth), so no element is excluded anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import stream_ref as S
from pin_harness import Bufs, Checks, untouched, written
from wavelet_monodepth_amd import synth

pytestmark = pytest.mark.gpu

# per tensor kind, the smallest power of two >= twice the largest e_hip / e_ref measured on the MI355X among the comparisons whose
# e_hip exceeds the floor (profiles/stream_ops_pins.md; the table and the case that set each entry are in DESIGN.md §4.6.2); 1 where
# no comparison of the kind exceeds the floor
F = {"dw_y": 1, "dw_dx": 1, "dw_dw": 1, "idwt_out": 1, "idwt_disp": 1, "haar_yl": 1, "haar_yh": 1, "act_dz": 1, "bil_y": 4, "bil_depth": 4,
     "bil_dx": 4, "flip": 1}
assert max(F.values()) <= 64

BAD_ARG, BAD_SHAPE = -1, -2
BLOCK = 256
NUM_CU = 256
# blocks a launch gets at most; a kernel strides (some thread takes a second trip) when its items exceed CAP * BLOCK
CAP_DW = 64                 # dwconv_fwd_kernel per (b, c) plane of H W pixels; dwconv_bwd_data_kernel per padded plane of (H+2)(W+2)
CAP_HAAR = NUM_CU * 8       # idwt_haar_fwd_kernel (pairs), its scalar form, haar_analysis_kernel, the reflect form (coefficients), act_bwd_kernel
CAP_BIL = NUM_CU * 16       # upsample_bilinear_fwd_kernel (outputs), upsample_bilinear_bwd_kernel (inputs)
CAP_FLIP = 4096             # flip_postprocess_kernel (pixels)
TINY = float(np.float32(2.0 ** -126))       # the smallest positive normal float
DENORM = float(np.float32(2.0 ** -149))     # the smallest positive float


def strides(items, cap):
    return items > cap * BLOCK


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def lib():
    from wavelet_monodepth_amd import _lib
    return _lib.lib()


def ptr(v):
    return None if v is None else v.data_ptr()


def nrm(shape, name, std=1.0):
    return torch.from_numpy(synth.normal(shape, "so_" + name, 31, std))


def uni(shape, name, lo=-1.0, hi=1.0):
    return torch.from_numpy(synth.uniform(shape, "so_" + name, 31, lo, hi))


def gpu(v, dev):
    return None if v is None else v.to(dev).contiguous()


def launch(what, fn, *args):
    """-> (status, kernel names in launch order); every kernel of an accepted launch ran once, a refused one launched nothing"""
    from wavelet_monodepth_amd import _lib
    _lib.profile_begin()
    st = fn(*args, torch.cuda.current_stream().cuda_stream)
    prof = _lib.profile_end()
    names = [r["kernel"] for r in prof]
    if st == 0:
        assert all(r["calls"] == 1 for r in prof), "%s: %s" % (what, prof)
    else:
        assert names == [], "%s: status %d, yet %s ran" % (what, st, names)
    return st, names


_ORACLES = {}


def oracle(key, fn):
    """(float32, float64) oracle results, computed once per key and left unchanged"""
    if key not in _ORACLES:
        _ORACLES[key] = (fn(torch.float32), fn(torch.float64))
    return _ORACLES[key]


def checks(case):
    return Checks(case, F)


# ---- A. wmd_dwconv3x3_fwd / wmd_dwconv3x3_bwd --------------------------------------------------------------------------------------
PADS = ("zero", "reflect", "replicate")
DATA, FOLD, WGT = "dwconv_bwd_data_kernel", "conv_dgrad_fold_kernel", "dwconv_bwd_weight_kernel"
# name -> (B, C1, C2, up1, H, W); C1 >= 1 always: dw_check refuses a null x1 (conv_check_problem: C1 <= 0 is a shape error)
DW_SMALL = {"6x10_up_skip": (2, 5, 7, 2, 6, 10), "5x7_c19": (1, 19, 0, 1, 5, 7), "4x6_skip_noup": (3, 3, 4, 1, 4, 6), "2x2_up": (1, 3, 0, 2, 2, 2)}
DW_STRIDE = {"130x128_up_skip": (1, 2, 1, 2, 130, 128), "129x128": (1, 3, 0, 1, 129, 128), "126x128_up_skip": (1, 2, 1, 2, 126, 128)}
DW_REDUCE = {"3x5_15terms": (1, 3, 0, 1, 3, 5), "9x11_99terms": (1, 2, 2, 1, 9, 11), "7x13_273terms": (3, 2, 2, 1, 7, 13)}
DW_ALL = dict(DW_SMALL, **DW_STRIDE, **DW_REDUCE)
_DW = {}


def dw_case(name):
    """inputs of a depthwise case, drawn once (the `y` a backward is given is the float32 oracle's forward of them)"""
    if name not in _DW:
        B, C1, C2, up1, H, W = DW_ALL[name]
        c = dict(B=B, C1=C1, C2=C2, up1=up1, H=H, W=W, x1=nrm((B, C1, H // up1, W // up1), name + "x1"),
                 x2=nrm((B, C2, H, W), name + "x2") if C2 else None, w=uni((C1 + C2, 1, 3, 3), name + "w", -0.25, 0.4),
                 dy=nrm((B, C1 + C2, H, W), name + "dy"))
        _DW[name] = c
    return _DW[name]


def dw_args(dev, c, pad):
    from wavelet_monodepth_amd import _lib
    keep = [gpu(c["x1"], dev), gpu(c["x2"], dev), gpu(c["w"], dev)]
    a = _lib.DwConvArgs(B=c["B"], H=c["H"], W=c["W"], C1=c["C1"], up1=c["up1"], C2=c["C2"], pad_mode=_lib.PAD[pad], x1=ptr(keep[0]),
                        x2=ptr(keep[1]), w=ptr(keep[2]))
    return a, keep


def dw_forward(dev, name, pad, chk):
    c = dw_case(name)
    what = "%s %s fwd" % (name, pad)
    o32, o64 = oracle(("dwf", name, pad), lambda dt: S.dwconv_fwd(c["x1"], c["x2"], c["w"], c["up1"], pad, dt))
    assert int((o64 > 0).sum()) > 0, what
    a, keep = dw_args(dev, c, pad)
    bufs = Bufs(dev)
    y = bufs.new("y", *o64.shape)
    st, kernels = launch(what, lib().wmd_dwconv3x3_fwd, C.byref(a), ptr(y))
    assert st == 0 and kernels == ["dwconv_fwd_kernel"], "%s: status %d, %s" % (what, st, kernels)
    bufs.bands(what)
    written(y, what + ": y")
    chk.add("dw_y", what, y, o32, o64)
    return o32


def dw_backward(dev, name, pad, chk, want=None, y=None, dy=None, tag="", workspace="exact", status=0):
    """one wmd_dwconv3x3_bwd launch; want: the outputs asked for (the others are passed as null; default: all); y / dy: replacements of the
    case's own (the float32 oracle's forward, the case's dy); workspace: "exact", "null" (with workspace_floats = 0) or "given"
    (exact, for a launch that must not touch it) -> the outputs by name"""
    c = dw_case(name)
    B, C1, C2, up1, H, W = (c[k] for k in ("B", "C1", "C2", "up1", "H", "W"))
    Cc = C1 + C2
    want = want or (("dx1", "dx2", "dw") if C2 else ("dx1", "dw"))        # every gradient the case has
    what = "%s %s bwd %s%s" % (name, pad, "+".join(want), tag)
    if y is None:
        y = oracle(("dwf", name, pad), lambda dt: S.dwconv_fwd(c["x1"], c["x2"], c["w"], up1, pad, dt))[0]
    dy = c["dy"] if dy is None else dy

    def ref(dt):
        dx1, dx2, dw = S.dwconv_bwd(c["x1"], c["x2"], c["w"], y, dy, up1, pad, dt)
        return dict(dx1=dx1, dx2=dx2, dw=dw)
    o32, o64 = oracle(("dwb", name, pad, tag), ref)
    a, keep = dw_args(dev, c, pad)
    yd, dyd = gpu(y, dev), gpu(dy, dev)
    bufs = Bufs(dev)
    o = dict(dx1=bufs.new("dx1", B, C1, H // up1, W // up1) if "dx1" in want else None,
             dx2=bufs.new("dx2", B, max(C2, 1), H, W) if "dx2" in want else None,
             dw=bufs.new("dw", Cc, 1, 3, 3) if "dw" in want else None)
    n = lib().wmd_dwconv3x3_bwd_workspace_floats(C.byref(a))
    assert n == B * Cc * (H + 2) * (W + 2), "%s: %d workspace floats" % (what, n)
    ws = bufs.new("workspace", n) if workspace != "null" else None
    st, kernels = launch(what, lib().wmd_dwconv3x3_bwd, C.byref(a), ptr(yd), ptr(dyd), ptr(o["dx1"]), ptr(o["dx2"]), ptr(o["dw"]), ptr(ws),
                         n if ws is not None else 0)
    assert st == status, "%s: status %d" % (what, st)
    bufs.bands(what)
    if status:
        for k, v in o.items():
            if v is not None:
                untouched(v, "%s: %s of a refused launch" % (what, k))
        return o
    data = "dx1" in want or "dx2" in want
    assert kernels == ([DATA, FOLD] if data else []) + ([WGT] if "dw" in want else []), "%s: %s" % (what, kernels)
    if ws is not None:
        (written if data else untouched)(ws, what + ": the workspace")
    for k in want:
        written(o[k], "%s: %s" % (what, k))
        if chk is not None:
            chk.add("dw_dw" if k == "dw" else "dw_dx", "%s %s" % (what, k), o[k], o32[k], o64[k])
    return o


@pytest.mark.parametrize("name", list(DW_SMALL) + list(DW_STRIDE))
def test_dwconv_fwd_and_bwd_vs_oracle(dev, name):
    """Forward, then the backward with all three gradients, under all three pad modes: up1 = 2 with and without a skip tensor, a
    skip tensor without the up-sampling, 2 x 2 (both ring rows fold onto one source row), and the planes at which
    dwconv_fwd_kernel (H W > 16 384) and dwconv_bwd_data_kernel ((H+2)(W+2) > 16 384) take a second trip."""
    B, C1, C2, up1, H, W = DW_ALL[name]
    if name in ("130x128_up_skip", "129x128"):
        assert strides(H * W, CAP_DW) and strides((H + 2) * (W + 2), CAP_DW)
    if name == "126x128_up_skip":      # the data kernel strides where the forward is still one trip
        assert not strides(H * W, CAP_DW) and strides((H + 2) * (W + 2), CAP_DW)
    chk = checks("A " + name)
    for pad in PADS:
        dw_forward(dev, name, pad, chk)
        dw_backward(dev, name, pad, chk)
    chk.done()


@pytest.mark.parametrize("name", list(DW_REDUCE) + ["130x128_up_skip"])
def test_dwconv_bwd_weight_reduction(dev, name):
    """dwconv_bwd_weight_kernel alone (dw only: no workspace): 15 terms (three waves of the four-wave LDS reduction idle), 99 and 273
    (no multiple of 64), and 16 640 (65 trips per thread)."""
    B, C1, C2, up1, H, W = DW_ALL[name]
    assert B * H * W == {"3x5_15terms": 15, "9x11_99terms": 99, "7x13_273terms": 273, "130x128_up_skip": 16640}[name]
    chk = checks("A " + name)
    for pad in PADS:
        dw_backward(dev, name, pad, chk, want=("dw",), workspace="null")
    chk.done()


def test_dwconv_bwd_null_combinations(dev):
    """What needs_input_grad can ask for on the 6 x 10 case: dx1 alone, dx2 alone, dw alone with a null workspace and
    workspace_floats = 0 (must succeed) or with a workspace (which must stay untouched), all three; a dx2 with C2 = 0 is an
    argument error and launches nothing."""
    chk = checks("A null combinations")
    for pad in PADS:
        full = dw_backward(dev, "6x10_up_skip", pad, chk)
        for want, wsp in ((("dx1",), "exact"), (("dx2",), "exact"), (("dw",), "null"), (("dw",), "given"), (("dx1", "dw"), "exact")):
            part = dw_backward(dev, "6x10_up_skip", pad, chk, want=want, workspace=wsp)
            for k in want:
                assert torch.equal(part[k], full[k]), "%s %s depends on which other gradients are asked for" % (pad, k)
    dw_backward(dev, "5x7_c19", "zero", None, want=("dx1", "dx2"), status=BAD_ARG)
    chk.done()


def test_dwconv_bwd_gate_at_zero(dev):
    """y planted at interior, corner and ring-adjacent pixels of every plane: exactly 0 (the gradient must not pass: y > 0 is
    strict) and the smallest positive float / the smallest positive normal (it must pass).  A dy that lives on the y == 0 plants
    alone gives gradients that are exactly zero; one on the positive plants alone gives the oracle's, which are not."""
    name = "6x10_up_skip"
    c = dw_case(name)
    chk = checks("A gate")
    spots = [(2, 4), (0, 0), (5, 9), (0, 3), (3, 0), (5, 4), (2, 9), (0, 9), (5, 0), (3, 5)]
    for pad in PADS:
        y = oracle(("dwf", name, pad), lambda dt: S.dwconv_fwd(c["x1"], c["x2"], c["w"], c["up1"], pad, dt))[0].clone()
        at0, atp = torch.zeros_like(y, dtype=torch.bool), torch.zeros_like(y, dtype=torch.bool)
        for i, (yy, xx) in enumerate(spots):
            if i % 2 == 0:
                y[:, :, yy, xx], at0[:, :, yy, xx] = 0.0, True
            else:
                y[:, :, yy, xx], atp[:, :, yy, xx] = (DENORM if i % 4 == 1 else TINY), True
        assert bool((y[at0] == 0).all()) and bool((y[atp] > 0).all())
        dw_backward(dev, name, pad, chk, y=y, tag=" planted")
        o = dw_backward(dev, name, pad, None, y=y, dy=torch.where(at0, c["dy"], torch.zeros(())), tag=" dy on y==0")
        for k, v in o.items():
            assert bool((v == 0).all()), "%s: %s is not zero although dy lives where y == 0" % (pad, k)
        o = dw_backward(dev, name, pad, chk, y=y, dy=torch.where(atp, c["dy"], torch.zeros(())), tag=" dy on y>0")
        for k, v in o.items():
            assert bool((v != 0).any()), "%s: %s is zero although dy lives where y > 0" % (pad, k)
    chk.done()


# ---- B. wmd_wavelet.hip ------------------------------------------------------------------------------------------------------------
SCALE = 0.5      # a power of two: out * SCALE is exact, so a planted out of 0 or 2 sits exactly on the clamp's edge
IDWT_SHAPES = [(1, 1, 2), (3, 5, 6), (2, 7, 5), (1, 257, 4096), (1, 129, 4097)]
# coefficients (a, b, c, d) whose four outputs (a +- b +- c +- d) / 2 are all 0, all 2 (disp exactly 1), all 4 (above), all -2 (below)
PLANTS = [(0.0, 0.0), (4.0, 1.0), (8.0, 1.0), (-4.0, 0.0)]      # (a, clamped disp)
_IDWT = {}


def idwt_case(shape):
    if shape not in _IDWT:
        N, h, w = shape
        tag = "idwt%dx%dx%d" % shape
        yl, yh = nrm((N, h, w), tag + "yl") + 1.0, nrm((N, 3, h, w), tag + "yh", 0.7)
        flat = [(n, y, x) for n in (0, N - 1) for y in (0, h - 1) for x in (0, w - 1)]
        spots = sorted(set(flat))[:len(PLANTS)]
        for (n, y, x), (a, _) in zip(spots, PLANTS):
            yl[n, y, x], yh[n, :, y, x] = a, 0.0
        _IDWT[shape] = (yl, yh, spots)
    return _IDWT[shape]


@pytest.mark.parametrize("shape", IDWT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_idwt_fwd_vs_oracle(dev, shape):
    """wmd_idwt_haar_fwd with disp null, with disp and the clamp, with disp and no clamp: one coefficient pair, ragged small shapes,
    an odd w (the scalar kernel) and the second trip of either kernel; coefficients planted so that out * scale is exactly 0,
    exactly 1, above 1 and below 0."""
    N, h, w = shape
    yl, yh, spots = idwt_case(shape)
    kernel = "idwt_haar_fwd_scalar_kernel" if w % 2 else "idwt_haar_fwd_kernel"
    if shape == (1, 257, 4096):
        assert strides(N * h * (w // 2), CAP_HAAR)
    if shape == (1, 129, 4097):
        assert strides(N * h * w, CAP_HAAR)
    chk = checks("B idwt %dx%dx%d" % shape)
    yld, yhd = gpu(yl, dev), gpu(yh, dev)
    for form, clamp01 in (("out", 0), ("disp clamp", 1), ("disp", 0)):
        what = "%dx%dx%d %s" % (shape + (form,))
        o32, o64 = oracle(("idwt", shape, clamp01), lambda dt: S.idwt(yl, yh, SCALE, bool(clamp01), dt))
        bufs = Bufs(dev)
        out = bufs.new("out", N, 2 * h, 2 * w)
        disp = bufs.new("disp", N, 2 * h, 2 * w) if form != "out" else None
        st, kernels = launch(what, lib().wmd_idwt_haar_fwd, ptr(yld), ptr(yhd), ptr(out), ptr(disp), N, h, w, SCALE, clamp01)
        assert st == 0 and kernels == [kernel], "%s: status %d, %s" % (what, st, kernels)
        bufs.bands(what)
        written(out, what + ": out")
        chk.add("idwt_out", what, out, o32[0], o64[0])
        if disp is not None:
            written(disp, what + ": disp")
            chk.add("idwt_disp", what, disp, o32[1], o64[1])
            for (n, y, x), (a, clamped) in zip(spots, PLANTS):
                got = disp[n, 2 * y:2 * y + 2, 2 * x:2 * x + 2].cpu()
                want = clamped if clamp01 else a * 0.5 * SCALE
                assert bool((got == want).all()), "%s: disp of the planted a = %g is %s, not %g" % (what, a, got.tolist(), want)
    chk.done()


BWD_SHAPES = [(6, 6, 10), (1, 1, 1), (1, 129, 4096)]       # (6, 6, 10): B = 2, C = 3 folded into N
# out values on the clamp's edge: exactly 0 and exactly 1 / SCALE pass the gradient, one ulp above 1 / SCALE and the smallest
# negative normal (its product with SCALE is a negative subnormal) do not
EDGE_OUT = [(0.0, True), (1.0 / SCALE, True), (float(np.nextafter(np.float32(1.0 / SCALE), np.float32(9.0))), False), (-TINY, False)]


@pytest.mark.parametrize("shape", BWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_idwt_bwd_vs_oracle(dev, shape):
    """wmd_idwt_haar_bwd: d_out alone, d_disp alone, both with the clamp, both without; channels folded into N, one coefficient,
    and the second trip of haar_analysis_kernel.  The clamp gate is inclusive: a d_disp that lives on the planted pixels alone
    passes at out * scale == 0 and == 1 and is stopped one ulp outside."""
    N, h, w = shape
    tag = "ibwd%dx%dx%d" % shape
    if shape == (1, 129, 4096):
        assert strides(N * h * w, CAP_HAAR)
    out = nrm((N, 2 * h, 2 * w), tag + "out", 1.5) + 1.0
    spots = [(0, 0, 0), (N - 1, 2 * h - 1, 2 * w - 1), (0, 0, 1), (N - 1, 2 * h - 1, 0)]
    assert len(set(spots)) == 4
    for s, (v, _) in zip(spots, EDGE_OUT):
        out[s] = v
    gate = S.clamp_gate(out, SCALE)
    assert [bool(gate[s]) for s in spots] == [p for _, p in EDGE_OUT]
    assert int(gate.sum()) > 4 or N * h * w == 1
    d_out, d_disp = nrm((N, 2 * h, 2 * w), tag + "do"), nrm((N, 2 * h, 2 * w), tag + "dd")
    only = torch.zeros_like(d_disp)
    for s in spots:
        only[s] = 2.0
    chk = checks("B idwt bwd %dx%dx%d" % shape)
    od = gpu(out, dev)
    for form, go, gd, clamp01 in (("d_out", d_out, None, 1), ("d_disp clamp", None, d_disp, 1), ("both clamp", d_out, d_disp, 1),
                                  ("both", d_out, d_disp, 0), ("planted d_disp clamp", None, only, 1)):
        what = "%dx%dx%d %s" % (shape + (form,))
        o32, o64 = oracle(("ibwd", shape, form), lambda dt: S.idwt_bwd(go, gd, out, SCALE, bool(clamp01), dt))
        bufs = Bufs(dev)
        d_yl, d_yh = bufs.new("d_yl", N, h, w), bufs.new("d_yh", N, 3, h, w)
        god, gdd = gpu(go, dev), gpu(gd, dev)
        st, kernels = launch(what, lib().wmd_idwt_haar_bwd, ptr(god), ptr(gdd), ptr(od), ptr(d_yl), ptr(d_yh), N, h, w, SCALE, clamp01)
        assert st == 0 and kernels == ["haar_analysis_kernel"], "%s: status %d, %s" % (what, st, kernels)
        bufs.bands(what)
        written(d_yl, what + ": d_yl")
        written(d_yh, what + ": d_yh")
        chk.add("haar_yl", what, d_yl, o32[0], o64[0])
        chk.add("haar_yh", what, d_yh, o32[1], o64[1])
        if form.startswith("planted"):      # the analysis of a plane that is zero but for the four plants: exact in float32
            assert torch.equal(d_yl.cpu().double(), o64[0]) and torch.equal(d_yh.cpu().double(), o64[1]), what
            assert float(o64[0][0, 0, 0]) != 0.0
    chk.done()


@pytest.mark.parametrize("shape", [(3, 4, 6), (1, 129, 4096)], ids=lambda s: "x".join(map(str, s)))
def test_dwt_fwd_vs_oracle(dev, shape):
    """wmd_dwt_haar_fwd (haar_analysis_kernel without gradients' arguments), small and on its second trip"""
    N, h, w = shape
    if shape == (1, 129, 4096):
        assert strides(N * h * w, CAP_HAAR)
    x = nrm((N, 2 * h, 2 * w), "dwt%dx%dx%d" % shape)
    what = "dwt %dx%dx%d" % shape
    o32, o64 = oracle(("dwt", shape), lambda dt: S.dwt(x, dt))
    bufs = Bufs(dev)
    yl, yh = bufs.new("yl", N, h, w), bufs.new("yh", N, 3, h, w)
    xd = gpu(x, dev)
    st, kernels = launch(what, lib().wmd_dwt_haar_fwd, ptr(xd), ptr(yl), ptr(yh), N, h, w)
    assert st == 0 and kernels == ["haar_analysis_kernel"], "%s: status %d, %s" % (what, st, kernels)
    bufs.bands(what)
    written(yl, what + ": yl")
    written(yh, what + ": yh")
    chk = checks("B " + what)
    chk.add("haar_yl", what, yl, o32[0], o64[0])
    chk.add("haar_yh", what, yh, o32[1], o64[1])
    chk.done()


@pytest.mark.parametrize("shape", [(2, 7, 9), (2, 2, 3), (2, 3, 2), (2, 8, 9), (1, 1025, 2049)], ids=lambda s: "x".join(map(str, s)))
def test_dwt_reflect_vs_oracle(dev, shape):
    """wmd_dwt_haar_reflect_fwd: both axes odd, the smallest odd axes beside an even one, one odd axis, the second trip"""
    N, H, W = shape
    h, w = (H + 1) // 2, (W + 1) // 2
    if shape == (1, 1025, 2049):
        assert strides(N * h * w, CAP_HAAR)
    x = nrm(shape, "dwtr%dx%dx%d" % shape)
    what = "dwt reflect %dx%dx%d" % shape
    o32, o64 = oracle(("dwtr", shape), lambda dt: S.dwt_reflect(x, dt))
    bufs = Bufs(dev)
    yl, yh = bufs.new("yl", N, h, w), bufs.new("yh", N, 3, h, w)
    xd = gpu(x, dev)
    st, kernels = launch(what, lib().wmd_dwt_haar_reflect_fwd, ptr(xd), ptr(yl), ptr(yh), N, H, W)
    assert st == 0 and kernels == ["haar_analysis_reflect_kernel"], "%s: status %d, %s" % (what, st, kernels)
    bufs.bands(what)
    written(yl, what + ": yl")
    written(yh, what + ": yh")
    chk = checks("B " + what)
    chk.add("haar_yl", what, yl, o32[0], o64[0])
    chk.add("haar_yh", what, yh, o32[1], o64[1])
    chk.done()


def test_dwt_reflect_rejects_an_odd_axis_of_one(dev):
    """reflection needs two samples: an odd axis of 1 is a shape error, nothing is launched or written"""
    for H, W in ((1, 4), (4, 1), (1, 1), (1, 3)):
        bufs = Bufs(dev)
        yl, yh = bufs.new("yl", 1, (H + 1) // 2, (W + 1) // 2), bufs.new("yh", 1, 3, (H + 1) // 2, (W + 1) // 2)
        xd = torch.ones((1, H, W), device=dev)
        st, _ = launch("%dx%d" % (H, W), lib().wmd_dwt_haar_reflect_fwd, ptr(xd), ptr(yl), ptr(yh), 1, H, W)
        assert st == BAD_SHAPE, "%dx%d: status %d" % (H, W, st)
        bufs.bands("%dx%d" % (H, W))
        untouched(yl, "yl of a refused launch")
        untouched(yh, "yh of a refused launch")


ACT_F32 = {S.ACT_NONE: lambda v: v, S.ACT_ELU: torch.nn.functional.elu, S.ACT_LEAKY: lambda v: torch.nn.functional.leaky_relu(v, 0.1),
           S.ACT_SIGMOID: torch.sigmoid}
SLOPE = float(np.float32(0.1))


@pytest.mark.parametrize("act", list(ACT_F32))
def test_act_bwd_vs_oracle(dev, act):
    """wmd_act_bwd for each activation code at n = 1, 255, 257 (a ragged block on either side of 256) and 525 313 (second trip);
    y on both sides of the kink and exactly at it (0, the smallest positive float, the smallest normals of either sign; for
    the sigmoid 0 and 1, where the derivative vanishes)."""
    chk = checks("B act %d" % act)
    for n in (1, 255, 257, 525313):
        if n == 525313:
            assert strides(n, CAP_HAAR)
        tag = "act%d_%d" % (act, n)
        y = ACT_F32[act](nrm((n,), tag + "x", 2.0))
        plants = [0.0, DENORM, -TINY, TINY, -DENORM] if act != S.ACT_SIGMOID else [0.5, 0.0, 1.0, DENORM, TINY]
        y[:min(n, len(plants))] = torch.tensor(plants[:n])
        dy = nrm((n,), tag + "dy")
        what = "act %d n %d" % (act, n)
        o32, o64 = oracle(("act", act, n), lambda dt: S.act_bwd(dy, y, act, SLOPE, dt))
        bufs = Bufs(dev)
        dz = bufs.new("dz", n)
        yd, dyd = gpu(y, dev), gpu(dy, dev)
        st, kernels = launch(what, lib().wmd_act_bwd, ptr(dyd), ptr(yd), ptr(dz), n, act, SLOPE)
        assert st == 0 and kernels == ["act_bwd_kernel"], "%s: status %d, %s" % (what, st, kernels)
        bufs.bands(what)
        written(dz, what + ": dz")
        chk.add("act_dz", what, dz, o32, o64)
        k = min(n, len(plants))         # at the plants the derivative is a constant of the piece (or y (1 - y) of an exact y): exact
        assert torch.equal(dz[:k].cpu(), o32[:k]), "%s: dz at the planted y %s is %s, the oracle's %s" % (what, plants[:k], dz[:k].tolist(), o32[:k].tolist())
    chk.done()


# ---- C. wmd_upsample_bilinear_fwd / _bwd -------------------------------------------------------------------------------------------
DEPTH_RANGE = (0.125, 80.0)
BIL_CASES = {     # name -> ((N, h, w), (H, W)); N = B C folded
    "up_5x7_11x9": ((6, 5, 7), (11, 9)), "up_6x20_24x80": ((1, 6, 20), (24, 80)),
    "down_24x40_7x9": ((2, 24, 40), (7, 9)), "down_9x9_4x9": ((1, 9, 9), (4, 9)),
    "in_1x1_5x6": ((1, 1, 1), (5, 6)), "out_1x1": ((1, 4, 5), (1, 1)), "out_1x7": ((1, 4, 5), (1, 7)), "identity_12x40": ((1, 12, 40), (12, 40)),
    "fwd_stride_1025x1031": ((1, 33, 41), (1025, 1031)), "bwd_stride_to_37x29": ((1, 1025, 1031), (37, 29)),
    "bwd_stride_to_1030x1040": ((1, 1025, 1031), (1030, 1040)),
}


@pytest.mark.parametrize("align", [False, True], ids=["half_pixel", "align_corners"])
@pytest.mark.parametrize("name", list(BIL_CASES))
def test_bilinear_vs_oracle(dev, name, align):
    """The loss front-end, forward (y alone, depth alone, both) and backward (dy alone, ddepth alone, both; the depth term from the
    GIVEN depth): up-sampling, down-sampling (the backward's inverted window spans several outputs), an input axis of 1, an
    output axis of 1 (scale 0 under align_corners: the window is the whole axis), identity, and the second trips of either
    kernel.  The cases that exist for the backward's second trip run the forward with both outputs only."""
    (N, h, w), (H, W) = BIL_CASES[name]
    if name == "fwd_stride_1025x1031":
        assert strides(N * H * W, CAP_BIL)
    if name.startswith("bwd_stride"):
        assert strides(N * h * w, CAP_BIL)
    what = "%s %s" % (name, "ac" if align else "hp")
    x = uni((N, h, w), "bil" + name, 0.0, 1.0)
    o32, o64 = oracle(("bil", name, align), lambda dt: S.bilinear(x, (H, W), align, DEPTH_RANGE, dt))
    chk = checks("C " + what)
    xd = gpu(x, dev)
    for form in (("y", "depth"),) if name.startswith("bwd_stride") else (("y",), ("depth",), ("y", "depth")):
        bufs = Bufs(dev)
        y = bufs.new("y", N, H, W) if "y" in form else None
        dp = bufs.new("depth", N, H, W) if "depth" in form else None
        w2 = "%s fwd %s" % (what, "+".join(form))
        st, kernels = launch(w2, lib().wmd_upsample_bilinear_fwd, ptr(xd), ptr(y), ptr(dp), N, h, w, H, W, int(align), *DEPTH_RANGE)
        assert st == 0 and kernels == ["upsample_bilinear_fwd_kernel"], "%s: status %d, %s" % (w2, st, kernels)
        bufs.bands(w2)
        if y is not None:
            written(y, w2 + ": y")
            chk.add("bil_y", w2, y, o32[0], o64[0])
        if dp is not None:
            written(dp, w2 + ": depth")
            chk.add("bil_depth", w2, dp, o32[1], o64[1])
    depth = o32[1]          # the depth the backward is given, device and oracle alike
    dy, dd = nrm((N, H, W), "bildy" + name), nrm((N, H, W), "bildd" + name, 0.01)
    dpd = gpu(depth, dev)
    for form, gy, gd in (("dy", dy, None), ("ddepth", None, dd), ("dy+ddepth", dy, dd)):
        w2 = "%s bwd %s" % (what, form)
        b32, b64 = oracle(("bilb", name, align, form), lambda dt: S.bilinear_bwd(gy, gd, depth, (h, w), align, DEPTH_RANGE, dt))
        bufs = Bufs(dev)
        dx = bufs.new("dx", N, h, w)
        gyd, gdd = gpu(gy, dev), gpu(gd, dev)
        st, kernels = launch(w2, lib().wmd_upsample_bilinear_bwd, ptr(gyd), ptr(gdd), ptr(dpd) if gd is not None else None, ptr(dx), N, h, w, H, W,
                             int(align), *DEPTH_RANGE)
        assert st == 0 and kernels == ["upsample_bilinear_bwd_kernel"], "%s: status %d, %s" % (w2, st, kernels)
        bufs.bands(w2)
        written(dx, w2 + ": dx")
        chk.add("bil_dx", w2, dx, b32, b64)
    chk.done()


# ---- D. wmd_flip_postprocess -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 8, 2), (1, 5, 33), (2, 3, 1), (1, 1025, 1031)], ids=lambda s: "x".join(map(str, s)))
def test_flip_postprocess_vs_oracle(dev, shape):
    """flip_postprocess_kernel: two columns, an odd width, one column (linspace(0, 1, 1) = [0]) and the second trip"""
    B, h, w = shape
    if shape == (1, 1025, 1031):
        assert strides(B * h * w, CAP_FLIP)
    what = "flip %dx%dx%d" % shape
    l, r = uni(shape, what + "l", 0.01, 1.0), uni(shape, what + "r", 0.01, 1.0)
    o32, o64 = oracle(("flip", shape), lambda dt: S.flip_postprocess(l, r, dt))
    bufs = Bufs(dev)
    out = bufs.new("out", B, h, w)
    ld, rd = gpu(l, dev), gpu(r, dev)
    st, kernels = launch(what, lib().wmd_flip_postprocess, ptr(ld), ptr(rd), ptr(out), B, h, w)
    assert st == 0 and kernels == ["flip_postprocess_kernel"], "%s: status %d, %s" % (what, st, kernels)
    bufs.bands(what)
    written(out, what + ": out")
    chk = checks("D " + what)
    chk.add("flip", what, out, o32, o64)
    chk.done()


# ---- E. the pointer contract of wmd_wavelet.hip (include/wmd.h) --------------------------------------------------------------------
def off_by_one(v, dev):
    """v on the device as a contiguous view that starts one float into its storage: data_ptr() is 4 bytes off an 8-byte boundary"""
    buf = torch.zeros((v.numel() + 1,), device=dev)
    buf[1:] = v.reshape(-1).to(dev)
    view = buf[1:].view(v.shape)
    assert view.is_contiguous() and view.data_ptr() % 8 == 4
    return view


def test_misaligned_pointers_are_refused(dev):
    """The vector kernels load float2 and store float4 through the caller's pointers: an entry point handed a pointer off that
    alignment returns the argument error and launches nothing.  An odd w (the scalar kernel) needs a float's alignment only."""
    N, h, w = 2, 3, 4
    yl, yh = off_by_one(nrm((N, h, w), "mis_yl"), dev), off_by_one(nrm((N, 3, h, w), "mis_yh"), dev)
    big = off_by_one(nrm((N, 2 * h, 2 * w), "mis_big"), dev)
    ok_yl, ok_yh, ok_big = yl.clone(), yh.clone(), big.clone()
    l = lib()
    for which in ("yl", "yh", "out", "disp"):
        bufs = Bufs(dev)
        out, disp = bufs.new("out", N * 4 * h * w + 4), bufs.new("disp", N * 4 * h * w + 4)
        a = dict(yl=ok_yl, yh=ok_yh, out=out, disp=disp)
        a.update({"yl": dict(yl=yl), "yh": dict(yh=yh), "out": dict(out=out[1:]), "disp": dict(disp=disp[1:])}[which])
        st, _ = launch("fwd " + which, l.wmd_idwt_haar_fwd, ptr(a["yl"]), ptr(a["yh"]), ptr(a["out"]), ptr(a["disp"]), N, h, w, SCALE, 1)
        assert st == BAD_ARG, "wmd_idwt_haar_fwd with a misaligned %s: status %d" % (which, st)
        bufs.bands("fwd " + which)
        untouched(out, "out of a refused launch")
        untouched(disp, "disp of a refused launch")
    for which in ("d_out", "d_disp", "out"):
        bufs = Bufs(dev)
        d_yl, d_yh = bufs.new("d_yl", N, h, w), bufs.new("d_yh", N, 3, h, w)
        a = dict(d_out=ok_big, d_disp=ok_big, out=ok_big)
        a[which] = big
        st, _ = launch("bwd " + which, l.wmd_idwt_haar_bwd, ptr(a["d_out"]), ptr(a["d_disp"]), ptr(a["out"]), ptr(d_yl), ptr(d_yh), N, h, w, SCALE, 1)
        assert st == BAD_ARG, "wmd_idwt_haar_bwd with a misaligned %s: status %d" % (which, st)
        untouched(d_yl, "d_yl of a refused launch")
        untouched(d_yh, "d_yh of a refused launch")
    bufs = Bufs(dev)
    d_yl, d_yh = bufs.new("yl", N, h, w), bufs.new("yh", N, 3, h, w)
    st, _ = launch("dwt", l.wmd_dwt_haar_fwd, ptr(big), ptr(d_yl), ptr(d_yh), N, h, w)
    assert st == BAD_ARG, "wmd_dwt_haar_fwd with a misaligned x: status %d" % st
    untouched(d_yl, "yl of a refused launch")
    # within the contract: an odd w at a float's alignment runs the scalar kernel
    N, h, w = 2, 7, 5
    yl_c, yh_c = nrm((N, h, w), "mis_yl5"), nrm((N, 3, h, w), "mis_yh5")
    yl, yh = off_by_one(yl_c, dev), off_by_one(yh_c, dev)
    bufs = Bufs(dev)
    out = bufs.new("out", N * 4 * h * w + 1)[1:].view(N, 2 * h, 2 * w)
    st, kernels = launch("odd w", l.wmd_idwt_haar_fwd, ptr(yl), ptr(yh), ptr(out), None, N, h, w, SCALE, 0)
    assert st == 0 and kernels == ["idwt_haar_fwd_scalar_kernel"], (st, kernels)
    bufs.bands("odd w")
    assert torch.equal(out.cpu(), S.idwt(yl_c, yh_c, SCALE, False, torch.float32)[0])


def test_ops_wrappers_copy_a_misaligned_view(dev):
    """ops.idwt_haar, forward and backward, and ops.dwt_haar on contiguous views at an odd element offset of their storage: the
    wrappers hand the entry points an aligned copy, and the results are those of aligned tensors, bit for bit."""
    from wavelet_monodepth_amd import ops
    B, Cc, h, w = 2, 3, 6, 10
    yl_c, yh_c = nrm((B, Cc, h, w), "ops_yl").to(dev) + 1.0, nrm((B, Cc, 3, h, w), "ops_yh", 0.7).to(dev)
    go_c, gd_c = nrm((B, Cc, 2 * h, 2 * w), "ops_go").to(dev), nrm((B, Cc, 2 * h, 2 * w), "ops_gd").to(dev)
    res = []
    for shift in (False, True):
        mk = (lambda v: off_by_one(v, dev)) if shift else (lambda v: v.clone())
        yl, yh = mk(yl_c).requires_grad_(True), mk(yh_c).requires_grad_(True)
        out, disp = ops.idwt_haar(yl, yh, SCALE, True)
        g_yl, g_yh = torch.autograd.grad([out, disp], [yl, yh], [mk(go_c), mk(gd_c)])
        ll, hh = ops.dwt_haar(mk(go_c))
        res.append([out.detach(), disp.detach(), g_yl, g_yh, ll, hh[0]])
    for name, a, b in zip(("out", "disp", "d_yl", "d_yh", "dwt yl", "dwt yh"), *res):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), "%s differs between an aligned tensor and a view at an odd offset" % name
