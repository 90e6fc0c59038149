"""The oracle of tests/sparse_conv_ref.py checked without a GPU: against the reference's sparse_conv3x3 restated in
oracle/decoder_ref.py on the committed primitive golden, against the masked dense formula tests/test_gpu_sparse.py uses (in float64),
and against itself in float32; and the case table of tests/test_gpu_sparse_conv.py against the mirror of the host's launch rules:
all 12 instantiations, the device-side task loop at default settings and under split_waves = 1."""
import numpy as np
import torch
import torch.nn.functional as F

import sparse_conv_ref as SR
from oracle import decoder_ref as R
from wavelet_monodepth_amd import synth
from util import load_golden, t


def _close(a, b, tol, what):
    err = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)
    assert err <= tol, "%s: %.3e > %.1e" % (what, err, tol)


def test_oracle_matches_the_reference_primitive_on_the_golden():
    """sparse_conv3x3 of the reference (restated: R.sparse_conv3x3_ref + R.scatter_dense) and the recorded result of the reference's
    own run, both index paddings, on the hand-made mask pair of kitti_sparse_primitives.npz"""
    g = load_golden("kitti_sparse_primitives.npz")
    mask, omask = t(g["mask"])[0, 0], t(g["omask"])[0, 0]
    H, W = mask.shape
    cin, cout = 5, 4
    nnz = int(mask.sum())
    vals = t(synth.normal((cin * nnz,), "pv", 5)).reshape(cin, nnz)
    bound = 1.0 / np.sqrt(cin * 9)
    w = t(synth.uniform((cout, cin, 3, 3), "conv.weight", 5, -bound, bound))
    b = t(synth.uniform((cout,), "conv.bias", 5, -bound, bound))
    dense_in = R.scatter_dense(vals, mask)[0]
    coords, counts = SR.raster_lists(omask[None] > 0.5)
    listed = (omask > 0.5)[None].expand(cout, -1, -1)
    for pad, name in (("reflect", "reflect"), ("zero", "constant")):
        got = SR.sparse_conv_oracle(dense_in, w, b, coords[0], counts[0], H * W, H, W, 3, torch.float64, in_mask=(mask > 0.5).to(torch.uint8), pad=pad)
        assert bool(torch.isnan(got[~listed]).all()) and bool(torch.isfinite(got[listed]).all())
        ref = R.scatter_dense(R.sparse_conv3x3_ref(vals.double(), R.mask_to_idxmap(mask), omask, w.double(), b.double(), pad), omask)[0]
        _close(got[listed], ref[listed], 1e-14, "oracle vs sparse_conv3x3_ref, " + pad)
        _close(got[listed], t(g["sconv_dense_" + name])[0].double()[listed], 2e-6, "oracle vs the recorded reference run, " + pad)


def _dense64(c, d, pad):
    """the masked dense formula of test_gpu_sparse.py in float64: mask the virtual input, pad it, F.conv2d, activation -> [B,Cout,H,W]"""
    def one(wt, bs, off):
        x = d["x1"][:, off:off + c["C1"]].double()
        if c["up1"] == 2:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        if d["x2"] is not None:
            x = torch.cat([x, d["x2"].double()], 1)
        if c["ksize"] == 3:
            if d["in_mask"] is not None:
                x = x * d["in_mask"][:, None].double()
            x = F.pad(x, (1, 1, 1, 1), mode={"reflect": "reflect", "zero": "constant"}[pad])
        return c["out_scale"] * SR._act(F.conv2d(x, wt.double(), bs.double()), c["act"], c["slope"])
    y = one(d["w"], d["b"], c["c1_off"])
    return y - one(d["w2"], d["b2"], c["c1_off2"]) if c["dual"] else y


def test_oracle_matches_the_masked_dense_formula_in_float64():
    """random masks with up1 = 2 + concat, a batched and a ragged 3x3, a 1x1, the dual form in all three families, a slice, no mask"""
    for key in ("rows_w1_3", "rows_mr4", "rows_mr2", "narrow_w1_2", "k1_mr1", "dual_rows", "dual_narrow", "dual_k1", "dual_gap", "slice", "no_mask", "up2_no_x2"):
        c = SR.CASES[key]
        d = SR.inputs(c)
        for pad in c["pads"]:
            ref = _dense64(c, d, pad)
            for density in ("30", "all", "none"):
                om = SR.out_mask(c, density)
                coords, counts = SR.raster_lists(om)
                got = SR.oracle(c, d, coords, counts, c["H"] * c["W"], pad, torch.float64)
                listed = om[:, None].expand_as(got)
                assert bool(torch.isnan(got[~listed]).all()), (key, pad, density)
                if density != "none":
                    _close(got[listed], ref[listed], 1e-13, "%s %s %s" % (key, pad, density))
                hc, hn = SR.hand_lists(c, om, density)       # the order of the list and what lies behind the count change nothing
                assert hn == counts
                again = SR.oracle(c, d, hc, hn, c["H"] * c["W"], pad, torch.float64)
                assert torch.equal(torch.nan_to_num(again, nan=-77.0), torch.nan_to_num(got, nan=-77.0)), (key, pad, density)


def test_oracle_clamps_the_count_and_ignores_poison():
    c = SR.CASES["rows_w1_3"]
    d = SR.inputs(c)
    om = SR.out_mask(c, "all")
    coords, counts = SR.raster_lists(om)
    full = SR.oracle(c, d, coords, counts, 36, "reflect", torch.float64)
    part = SR.oracle(c, d, coords[:, :20], [25], 20, "reflect", torch.float64)          # a count above max_out: the first max_out entries
    assert torch.equal(part.reshape(1, 17, 36)[:, :, :20], full.reshape(1, 17, 36)[:, :, :20]) and bool(torch.isnan(part.reshape(1, 17, 36)[:, :, 20:]).all())
    c = SR.CASES["rows_mr4"]        # up1 = 2: 2 x 19 x 18 coarse pixels, a few of them with all four fine pixels masked
    d = SR.inputs(c)
    coords, counts = SR.raster_lists(SR.out_mask(c, "all"))
    q = SR.poisoned(c, d)
    assert not bool(torch.isfinite(q["x2"]).all()) and not bool(torch.isfinite(q["x1"]).all())
    assert torch.equal(SR.oracle(c, q, coords, counts, 38 * 36, "reflect", torch.float64), SR.oracle(c, d, coords, counts, 38 * 36, "reflect", torch.float64))


def test_float32_oracle_differs_from_float64():
    """e_ref > 0 on a multi-channel case: the float32 run is a separate computation, not the float64 result rounded"""
    c = SR.CASES["rows_mr4"]
    d = SR.inputs(c)
    om = SR.out_mask(c, "30")
    coords, counts = SR.raster_lists(om)
    o32, o64 = [SR.oracle(c, d, coords, counts, c["H"] * c["W"], "reflect", dt) for dt in (torch.float32, torch.float64)]
    assert o32.dtype == torch.float32 and o64.dtype == torch.float64
    listed = om[:, None].expand_as(o64)
    e_ref = float((o32.double() - o64)[listed].abs().max()) / float(o64[listed].abs().max())
    assert 0 < e_ref < 1e-5, e_ref


def test_case_table_reaches_every_instantiation_and_the_task_loop():
    names = set()
    for c in SR.TABLE:
        s = SR.case_select(c)
        assert s["name"] == SR.want_name(c), "%s selects %s, the table says %s" % (c["key"], s["name"], SR.want_name(c))
        names.add(s["name"])
    assert len(SR.ALL_INSTANTIATIONS) == 12 and names == set(SR.ALL_INSTANTIATIONS), sorted(set(SR.ALL_INSTANTIATIONS) - names)   # (a)
    # the rows the plan spells out
    assert SR.case_select(SR.CASES["rows_mr2"])["tiles"] * 3 * 2 == 540 and SR.case_select(SR.CASES["rows_mr4"])["groups"] == 2
    assert SR.case_select(SR.CASES["rows_mr4"])["ncot"] == 5 and SR.case_select(SR.CASES["k1_mr4"])["ncot"] == 3
    assert SR.case_select(SR.CASES["narrow_mr2"])["tiles"] == 260
    # (b) default settings, S = WK: more tiles than blocks, so blocks 0..3 take a second task
    s = SR.case_select(SR.CASES["loop_default"])
    assert (s["tiles"], s["grid_x"]) == (260, 256) and SR.k_slices(s["tiles"], s["WK"]) == s["WK"]
    # (c) split_waves = 1: S = 1, WK tiles per block, 33 tasks over 32 blocks
    c = SR.CASES["loop_s1"]
    s = SR.case_select(c)
    S = SR.k_slices(s["tiles"], s["WK"], c["split_waves"])
    tpb = s["WK"] // S
    assert S == 1 and tpb == 8 and s["grid_x"] == 32 and -(-s["tiles"] // tpb) == 33 > s["grid_x"]
    # the middle switch point of the K-slice tests: ntile + 1 gives S = 2 in both block shapes
    for WK in (8, 4):
        for ntile in (1, 27, 90, 260):
            assert [SR.k_slices(ntile, WK, sw) for sw in (1, ntile + 1, 2 ** 30)] == [1, 2, WK]
    # the children's switches
    for key in ("rows_mr2", "rows_mr4", "rows_w3"):
        assert SR.case_select(SR.CASES[key], rows_on=False)["name"].endswith(",false>")
        assert SR.case_select(SR.CASES[key], grid_target=3)["grid_x"] == 1
