"""CPU: the F(4x4,3x3) contract (tests/wino44_ref.py) in float64 against a direct convolution, the structured form of an
upsampled operand against the full one, what the library answers without a GPU call: sizes and refusals, and the case table of the
pass-by-pass pins (tests/wino44_cases.py) with the three images of wino44_ref.images, before any GPU run."""
import ctypes as C

import numpy as np
import pytest

import wino44_cases as WC
import wino44_ref as W
from wavelet_monodepth_amd import _lib


def _rng(seed):
    return np.random.default_rng(seed)


def test_line_transform_then_inverse_is_the_three_tap_filter():
    """A^T [(G g) * (B^T d)] = the four outputs of the 1-D correlation, to 1e-12"""
    r = _rng(0)
    d, g = r.standard_normal(6), r.standard_normal(3)
    got = W.AT @ ((W.G @ g) * (W.BT @ d))
    want = np.array([d[i:i + 3] @ g for i in range(4)])
    assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("pad", ["reflect", "zero", "replicate"])
@pytest.mark.parametrize("shape", [(2, 5, 8, 12), (1, 3, 6, 10), (2, 4, 5, 7), (1, 2, 2, 3)])
def test_pure_layer_equals_direct_convolution(shape, pad):
    B, Cin, H, Wd = shape
    r = _rng(1)
    x, w, b = r.standard_normal(shape), r.standard_normal((6, Cin, 3, 3)), r.standard_normal(6)
    want = W.direct(x, w, b, pad=pad)
    got = W.wino44(x, w, b, pad=pad)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("pad", ["reflect", "zero", "replicate"])
@pytest.mark.parametrize("hw", [(12, 20), (6, 10), (4, 8), (2, 2)])
def test_up_and_skip_layer_equals_direct_convolution(hw, pad):
    """H, W = 2 mod 4 included: the low-resolution sample that clamping replaces only reaches discarded outputs"""
    H, Wd = hw
    r = _rng(2)
    x1, x2 = r.standard_normal((2, 3, H // 2, Wd // 2)), r.standard_normal((2, 5, H, Wd))
    w, b = r.standard_normal((7, 8, 3, 3)), r.standard_normal(7)
    want = W.direct(x1, w, b, x2=x2, up1=2, pad=pad)
    for structured in (True, False):
        got = W.wino44(x1, w, b, x2=x2, up1=2, pad=pad, structured=structured)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), structured


def test_structured_form_equals_the_full_form_on_a_replicated_patch_exactly():
    """On integer data every product and sum below is exact in float64: the 25 positions computed from the 4x4 low-resolution
    patch are bit for bit the 36 positions of the replicated 6x6 patch, whose row and column 2 hold exactly 0 -- and so are the
    outputs.  Positions 3 and 4 hold the same datum (x -3), but columns 3 and 4 of A differ in sign on the odd output rows: a
    16-position form with one combined weight row U4 - 3 U3 is NOT the same operator (asserted below)."""
    r = _rng(3)
    s = r.integers(-8, 9, size=(4, 4)).astype(np.float64)
    idx = [0, 1, 1, 2, 2, 3]
    d = s[np.ix_(idx, idx)]
    Vf = W.BT @ d @ W.BT.T
    Vu = W.BT_UP @ s @ W.BT_UP.T
    pos = np.ix_(W.UP_POS, W.UP_POS)
    assert np.array_equal(Vf[pos], Vu)
    assert np.array_equal(Vf[2], np.zeros(6)) and np.array_equal(Vf[:, 2], np.zeros(6))
    assert np.array_equal(Vf[3], -3.0 * Vf[4]) and np.array_equal(Vf[:, 3], -3.0 * Vf[:, 4])
    # weights whose transformed image is exact too (multiples of 24^2 make every entry of G g G^T an integer)
    g = 576.0 * r.integers(-4, 5, size=(3, 3)).astype(np.float64)
    Uf = np.round(W.G @ g @ W.G.T)
    assert np.abs(Uf - W.G @ g @ W.G.T).max() < 1e-9
    full = W.AT @ (Uf * Vf) @ W.AT.T
    assert np.array_equal(full, W.AT[:, W.UP_POS] @ (Uf[pos] * Vu) @ W.AT[:, W.UP_POS].T)
    want = np.array([[(d[i:i + 3, j:j + 3] * g).sum() for j in range(4)] for i in range(4)])
    assert np.array_equal(full, want)
    k4 = [0, 1, 4, 5]
    Gc = np.stack([W.G[0], W.G[1], W.G[4] - 3.0 * W.G[3], W.G[5]])
    folded = W.AT[:, k4] @ (np.round(Gc @ g @ Gc.T) * Vf[np.ix_(k4, k4)]) @ W.AT[:, k4].T
    assert np.array_equal(folded[::2, ::2], want[::2, ::2]) and not np.array_equal(folded, want)


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def _args(**kw):
    base = dict(B=12, H=12, W=40, C1=256, up1=2, C2=256, Cout=256, ksize=3, pad_mode=1, act=1, slope=0.0, x1=1, x2=1, wp=1,
                bias=None, y=1, workspace=None, workspace_floats=0, tune_cfg=0, tune_ksplit=0)
    base.update(kw)
    return _lib.ConvArgs(**base)


@pytest.mark.parametrize("B,H,Wd,C1,up,C2,Cout", [(12, 12, 40, 256, 2, 256, 256), (12, 24, 80, 128, 2, 128, 128),
                                                  (12, 12, 40, 256, 1, 0, 128), (1, 5, 7, 24, 1, 0, 8), (3, 12, 20, 8, 2, 8, 19)])
def test_workspace_and_weight_sizes(lib, B, H, Wd, C1, up, C2, Cout):
    a = _args(B=B, H=H, W=Wd, C1=C1, up1=up, C2=C2, Cout=Cout, x2=1 if C2 else None)
    assert lib.wmd_conv_wino44_supported(C.byref(a)) == 1
    assert lib.wmd_conv_wino44_workspace_floats(C.byref(a)) == W.workspace_floats(B, H, Wd, C1, C2, Cout)
    assert lib.wmd_conv_packed_weight_floats_wino44(Cout, C1, C2) == W.weight_floats(C1, C2, Cout)


def test_the_two_coarse_layers_are_360_and_1440_tiles():
    assert W.tiles(12, 12, 40) == 360 and W.tiles(12, 24, 80) == 1440 and W.tiles(12, 6, 20) == 120


@pytest.mark.parametrize("change,status,text", [
    (dict(ksize=1), -3, b"3x3 only"),
    (dict(gate=1), -3, b"gate"),
    (dict(in_mask=1), -3, b"in_mask"),
    (dict(out_mask=1), -3, b"out_mask"),
    (dict(out_tiles=1, out_tile_count=1), -3, b"out_tiles"),
    (dict(tune_cfg=1), -3, b"tune_cfg"),
    (dict(tune_ksplit=2), -3, b"tune_ksplit"),
    (dict(up1=3), -1, b"up1"),
    (dict(H=13), -2, b"even"),
    (dict(H=1, up1=1), -2, b"reflect"),
    (dict(B=4096, H=512, W=512), -3, b"tiles"),
    (dict(B=64, H=96, W=320), -3, b"2 GiB"),
])
def test_refusals_before_any_launch(lib, change, status, text):
    a = _args(**change)
    assert lib.wmd_conv_wino44_supported(C.byref(a)) == 0
    assert text in lib.wmd_last_error()
    assert lib.wmd_conv_wino44_workspace_floats(C.byref(a)) == 0
    assert lib.wmd_conv_wino44_fwd(C.byref(a), None) == status
    assert text in lib.wmd_last_error()


def test_the_shape_queries_need_no_tensor_pointer_and_a_launch_does(lib):
    a = _args(x1=None, x2=None, wp=None, y=None)
    assert lib.wmd_conv_wino44_supported(C.byref(a)) == 1
    n = lib.wmd_conv_wino44_workspace_floats(C.byref(a))
    assert n == W.workspace_floats(12, 12, 40, 256, 256, 256)
    a.workspace, a.workspace_floats = 1, n
    assert lib.wmd_conv_wino44_fwd(C.byref(a), None) == -1 and b"null tensor pointer" in lib.wmd_last_error()
    a.x1 = a.wp = a.y = 1
    assert lib.wmd_conv_wino44_fwd(C.byref(a), None) == -1 and b"x2" in lib.wmd_last_error()


def test_workspace_one_float_short_is_refused(lib):
    a = _args()
    n = lib.wmd_conv_wino44_workspace_floats(C.byref(a))
    a.workspace, a.workspace_floats = 1, n - 1
    assert lib.wmd_conv_wino44_fwd(C.byref(a), None) == -5
    assert b"workspace" in lib.wmd_last_error()
    a.workspace = None
    a.workspace_floats = n
    assert lib.wmd_conv_wino44_fwd(C.byref(a), None) == -5


def test_pack_refusals(lib):
    assert lib.wmd_conv_pack_weights_wino44(None, 1, 8, 8, 0, 1, None) == -1
    assert lib.wmd_conv_pack_weights_wino44(1, 1, 8, 8, 0, 3, None) == -1
    assert lib.wmd_conv_pack_weights_wino44(1, 1, 0, 8, 0, 1, None) == -2
    assert lib.wmd_conv_packed_weight_floats_wino44(8, 0, 8) == 0


# ---- the case table of the pins (tests/wino44_cases.py) and the three images (wino44_ref.images), before any GPU run -------------------
def _direct_act(c):
    x1, w, b, x2 = WC.operands(c)
    return W.activate(W.direct(x1, w, b, x2=x2, up1=c["up1"], pad=c["pad"]), c["act"], c["slope"])


@pytest.mark.parametrize("key", WC.KEYS)
def test_images_reassemble_to_the_direct_convolution(key):
    """U and V in the kernels' layouts, multiplied per position over the kernel's reduction range (every channel; c >= C1p at the
    11 short positions of a split layer), then A^T . A, bias and activation: the direct convolution to 1e-12.  M is that product."""
    c = WC.CASES[key]
    x1, w, b, x2 = WC.operands(c)
    d = W.dims(c["B"], c["H"], c["W"], c["C1"], c["C2"], c["Cout"])
    U, V, M, un = W.images(x1, w, b, x2, c["up1"], c["pad"])
    assert U.shape == (36, d.Ktot // 4, d.Coutp, 4) and U.size == d.u_floats
    assert V.shape == un.shape == (36, d.Ktot // 4, d.NTp, 4) and V.size == d.v_floats
    assert M.shape == (36, d.Coutp, d.NTp) and M.size == d.m_floats
    poisoned = np.where(un, np.nan, V)                      # what the contract leaves untouched is never read
    got_m = np.zeros_like(M)
    for p in range(36):
        g0 = W.kbeg(p, c["up1"], d.C1p) // 4
        got_m[p] = np.einsum("gok,gtk->ot", U[p, g0:], poisoned[p, g0:])
    assert np.isfinite(got_m).all() and np.abs(got_m - M).max() <= 1e-12 * max(1.0, np.abs(M).max())
    assert int(un.sum()) == (11 * d.C1p * d.NTp if c["up1"] == 2 else 0)
    # padded rows / columns, dead channels and dead tiles are zero
    Uc, Vc = W.unpack4(U), W.unpack4(np.where(un, 0.0, V))
    for lo, hi in ((c["C1"], d.C1p), (d.C1p + c["C2"], d.Ktot)):
        assert not Uc[:, lo:hi].any() and not Vc[:, lo:hi].any()
    assert not Uc[:, :, c["Cout"]:].any() and not Vc[:, :, d.NT:].any()
    if c["up1"] == 2:
        assert not Uc[list(W.SHORT), :d.C1p].any()
        if c["C2"] == 0:
            assert not M[list(W.SHORT)].any()
    got = W.output_image(got_m, b, c["B"], c["H"], c["W"], c["Cout"], c["act"], c["slope"])
    want = _direct_act(c)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("key", WC.KEYS)
def test_the_library_agrees_with_dims(lib, key):
    c = WC.CASES[key]
    d = W.dims(c["B"], c["H"], c["W"], c["C1"], c["C2"], c["Cout"])
    a = _args(B=c["B"], H=c["H"], W=c["W"], C1=c["C1"], up1=c["up1"], C2=c["C2"], Cout=c["Cout"], x2=1 if c["C2"] else None,
              pad_mode=_lib.PAD[c["pad"]], act=_lib.ACT[c["act"]], slope=c["slope"], bias=1 if c["bias"] else None)
    assert lib.wmd_conv_wino44_supported(C.byref(a)) == 1, lib.wmd_last_error()
    assert lib.wmd_conv_wino44_workspace_floats(C.byref(a)) == d.v_floats + d.m_floats == W.workspace_floats(c["B"], c["H"], c["W"], c["C1"], c["C2"], c["Cout"])
    assert lib.wmd_conv_packed_weight_floats_wino44(c["Cout"], c["C1"], c["C2"]) == d.u_floats == W.weight_floats(c["C1"], c["C2"], c["Cout"])


@pytest.mark.parametrize("key", WC.KEYS)
def test_three_pass_f32_is_usable_as_a_reference(key):
    """the float32 restatement against the float64 direct convolution: a finite, non-zero e_ref, far below the flat 5e-5"""
    c = WC.CASES[key]
    x1, w, b, x2 = WC.operands(c)
    got = W.three_pass_f32(x1, w, b, x2, c["up1"], c["pad"], c["act"], c["slope"])
    want = _direct_act(c)
    assert got.dtype == np.float32 and got.shape == want.shape
    e_ref = np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()
    print("E_REF %-20s %.3e" % (key, e_ref))
    assert np.isfinite(e_ref) and 0.0 < e_ref < 5e-5


def test_the_case_table_reaches_every_edge():
    """by predicate on dims() / blocks(): every row of the edge table of DESIGN.md §4.6.7"""
    rows = []
    for c in WC.TABLE:
        d = W.dims(c["B"], c["H"], c["W"], c["C1"], c["C2"], c["Cout"])
        rows.append((c, d, W.blocks(d, c["up1"])))
        assert d.NT < 200 and (max(c["C1"], c["C2"]) < 100 or c["key"] == "chunks_16")      # small: per operand under 100 channels

    def some(pred):
        return any(pred(c, d, g) for c, d, g in rows)

    # one GEMM block, NTp = 32 below both block widths, pure 32 -> 32
    assert some(lambda c, d, g: g["nbm"] == g["nbn_long"] == g["nbn_short"] == 1 and d.NTp == 32 and c["up1"] == 1 and (c["C1"], c["C2"], c["Cout"]) == (32, 0, 32))
    # two out-channel blocks, the second ragged -- with 8 and with 1 live rows in its 32
    assert some(lambda c, d, g: g["nbm"] == 2 and d.Coutp % 64 == 32 and c["Cout"] == 72)
    assert some(lambda c, d, g: g["nbm"] == 2 and d.Coutp % 64 == 32 and c["Cout"] == 65)
    # several tile blocks of both widths with a ragged last one, dead tiles, a batch decode that is no shift
    assert some(lambda c, d, g: g["split"] and g["nbn_long"] == 3 and g["nbn_short"] == 2 and d.NTp % 64 == 32 and d.NT % 32 != 0 and g["nbm"] == 2
                and c["B"] > 1 and (d.th * d.tw) & (d.th * d.tw - 1))
    # dead channels in both operands, above 32; a single live channel
    assert some(lambda c, d, g: 32 < c["C1"] < d.C1p and 0 < c["C2"] < d.C2p)
    assert some(lambda c, d, g: 32 < c["C1"] < d.C1p and 32 < c["C2"] < d.C2p)
    assert some(lambda c, d, g: c["C1"] == 1)
    # chunk counts
    assert {1, 2, 3, 16} <= {g["chunks_full"] for c, d, g in rows}
    assert {1, 3} <= {g["chunks_short"] for c, d, g in rows if g["split"]}
    assert some(lambda c, d, g: g["split"] and g["chunks_full"] % 2 == 1 and g["chunks_full"] > 1 and g["chunks_short"] == 1)
    assert some(lambda c, d, g: g["split"] and g["chunks_short"] % 2 == 1 and g["chunks_short"] > 1)
    assert some(lambda c, d, g: g["split"] and g["chunks_short"] == 0)          # up2 without a skip tensor
    # sizes mod 4
    assert {(0, 0), (1, 3), (2, 2), (3, 1)} <= {(c["H"] % 4, c["W"] % 4) for c, d, g in rows if c["up1"] == 1}
    assert {(0, 0), (2, 2)} <= {(c["H"] % 4, c["W"] % 4) for c, d, g in rows if c["up1"] == 2 and c["H"] > 2}
    # one row, one column: zero and replicate
    for hw in ((1, 9), (7, 1)):
        assert {"zero", "replicate"} == {c["pad"] for c, d, g in rows if (c["H"], c["W"]) == hw}
    # H = 2 / W = 2 under up2, all paddings
    for hw in ((2, 2), (2, 6)):
        assert {"zero", "reflect", "replicate"} == {c["pad"] for c, d, g in rows if (c["H"], c["W"]) == hw and c["up1"] == 2 and c["C2"] > 0}
    # 16-byte stores with a ragged last tile row
    assert some(lambda c, d, g: c["W"] % 4 == 0 and c["H"] % 4 != 0 and c["H"] > 4)
    # paddings: under up1, and under up2 with a skip tensor
    assert {"zero", "reflect", "replicate"} == {c["pad"] for c, d, g in rows if c["up1"] == 1 and min(c["H"], c["W"]) > 1}
    assert {"zero", "reflect", "replicate"} == {c["pad"] for c, d, g in rows if c["up1"] == 2 and c["C2"] > 0 and c["H"] > 2}
    # activations and bias = NULL, on 6x10 up2 and on 5x7 up1
    for hw, up in (((6, 10), 2), ((5, 7), 1)):
        mine = [c for c, d, g in rows if (c["H"], c["W"], c["up1"]) == hw + (up,) and c["bias"]]
        assert {"none", "elu", "leaky", "sigmoid"} == {c["act"] for c in mine}
        assert all(c["slope"] == 0.1 for c in mine if c["act"] == "leaky")
        assert any(not c["bias"] for c, d, g in rows if (c["H"], c["W"], c["up1"]) == hw + (up,))
    assert all(k in WC.CASES for k in WC.REPEAT)
