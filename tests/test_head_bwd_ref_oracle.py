"""The float64 oracle of the wavelet heads' backward (head_bwd_ref.py) against an independent formulation, and the shape rules
that test_gpu_head_bwd.py relies on: every table row reaches the forms it names, and the re-derived block counts reproduce the
workspace answers pinned in test_host_logic.py.  No GPU."""
import pytest
import torch

import head_bwd_ref as HB


@pytest.mark.parametrize("shape,pad", [(s, p) for s in [(2, 2), (1, 5), (3, 4), (5, 7)] for p in HB.pads_of((1,) + s)],
                         ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
def test_oracle_agrees_with_explicit_tap_and_ring_loops(shape, pad):
    """autograd over decoder_ref.conv3x3 == the explicit sum over taps and over the padded positions that fold onto each pixel, to
    1e-12 of the largest value, for a 3-row and a 1-row head at non-zero row and channel offsets; dz carries the gate.  (Reflection
    needs two rows and two columns: the 1 x 5 map runs under zero and replicate.)"""
    H, W = shape
    heads = [(4, 3, 5, 6), (1, 1, 13, 4)]
    for act in HB.ACTS:
        c = HB.case3x3("loops%dx%d%s%s" % (H, W, pad, act), 2, H, W, 19, 7, heads, act)
        o = HB.oracle3x3(c, pad, torch.float64)
        mid, dy = c["mid"].double(), c["dy3"].double()
        own = torch.zeros(19, dtype=torch.bool)
        for k, (row0, nrows, ch0, nch) in enumerate(heads):
            m = mid[:, ch0:ch0 + nch]
            dmid, dw, db = HB.head3x3_bwd_loops(dy[:, row0:row0 + nrows], m, c["w3"][k].double(), pad)
            g = torch.ones_like(m) if act == "none" else torch.where(m > 0, torch.ones_like(m), 0.1 * torch.ones_like(m) if act == "leaky" else 1 + m)
            for name, got, want in (("dz", o["dz"][:, ch0:ch0 + nch], dmid * g), ("dw3", o["dw3"][k], dw), ("db3", o["db3"][k], db)):
                err = float((got - want).abs().max()) / float(want.abs().max())
                assert err <= 1e-12, "%s %s head %d %s: %.3e" % (pad, act, k, name, err)
            own[ch0:ch0 + nch] = True
        assert bool(torch.isnan(o["dz"][:, ~own]).all()), "the oracle writes channels of no head"


def test_gate_takes_the_nonpositive_branch_at_both_zeros():
    m = torch.tensor([0.0, -0.0, 0.5, -0.5], dtype=torch.float64)
    assert HB.gate(m, "none").tolist() == [1, 1, 1, 1]
    assert HB.gate(m, "leaky").tolist() == [0.1, 0.1, 1, 0.1]
    assert HB.gate(m, "elu").tolist() == [1, 1, 1, 0.5]
    c = HB.case3x3("zeros", 2, 5, 7, 8, 3, [(0, 3, 0, 8)], "elu")
    z = c["mid"] == 0
    assert int(z.sum()) >= 2 and bool(torch.signbit(c["mid"][z]).any()) and not bool(torch.signbit(c["mid"][z]).all())


def test_oracle_1x1_agrees_with_the_plain_sums():
    for act in HB.ACTS:
        c = HB.case1x1("plain1x1" + act, 2, 3, 5, 6, 8, act)
        o = HB.oracle1x1(c, torch.float64)
        dz, x, w1 = c["dz"].double(), c["x"].double(), c["w1"].double()
        dx = torch.einsum("kc,bkhw->bchw", w1, dz) * HB.gate(x, act)
        for name, want in (("dx", dx), ("dw1", torch.einsum("bkhw,bchw->kc", dz, x)), ("db1", dz.sum((0, 2, 3)))):
            assert float((o[name] - want).abs().max()) <= 1e-12 * float(want.abs().max()), (act, name)


# ---- the table rows reach the forms they are there for ---------------------------------------------------------------------------
def test_every_table_row_reaches_the_forms_it_names():
    for shape, why, _layouts in HB.A_TABLE:
        assert HB.row_reaches(shape, why) == [], shape
    for shape, why in HB.B_WRAPS + HB.D_SHAPES:
        assert HB.row_reaches(shape, why) == [], shape
    c = HB.classify(2, 6, 40)
    assert c["groups"] == dict(inner=2 * 2, edge=2 * 13, tiny=0) and (c["whole"], c["ragged"]) == (6, 2)     # rows 2 and 3, columns 16..31
    assert HB.classify(3, 8, 48)["groups"]["inner"] == 3 * 4                                                 # rows 2..5, columns 16..31
    assert HB.classify(129, 8, 64)["loops"]["w3"] == dict(blocks=256, wraps=1, remainder=8)
    assert HB.classify(16387, 2, 2)["loops"]["d"] == dict(blocks=4096, wraps=1, remainder=3)
    lp = HB.classify(*HB.C_EXTRA)["loops"]
    assert (lp["w3"]["blocks"], lp["w1"]["blocks"], lp["d_merged"]["blocks"]) == (256, 512, 1024)
    assert lp["w3"]["wraps"] == 4 and lp["w1"]["wraps"] == 2 and lp["d_merged"]["wraps"] == 1 and lp["d_merged"]["remainder"] == 3
    assert [HB.head3x3_blocks(t) for t in HB.REDUCE3_TILES] == [1, 1, 1, 2, 3, 5]
    assert [HB.head1x1_blocks(t) for t in HB.REDUCE1_TILES] == [1, 1, 5, 9]


def test_layouts_and_activations_cover_what_the_issue_asks():
    runs = HB.a_runs()
    kind = lambda s: "tiny" if HB.classify(*s)["tiny"] else ("inner" if HB.classify(*s)["groups"]["inner"] else "edge")
    for name in HB.CROSSED:
        assert {kind(s) for s, n, _p, _a in runs if n == name} == {"tiny", "edge", "inner"}, name
    for pad in HB.PADS:
        for act in HB.ACTS:
            mine = [HB.classify(*s) for s, _n, p, a in runs if (p, a) == (pad, act)]
            assert any(c["vec"] and not c["tiny"] for c in mine) and any(not c["vec"] for c in mine) and any(c["tiny"] for c in mine), (pad, act)
    for shape, _n, pad, _a in runs:
        assert pad != "reflect" or min(shape[1:]) >= 2
    assert {p for s, _n, p, _a in runs if s == (2, 1, 7)} == {"zero", "replicate"} == {p for s, _n, p, _a in runs if s == (2, 5, 1)}
    L = HB.LAYOUTS
    assert HB.n_slices(L["s24"]["heads"]) == HB.HB_MAX_SLICES and HB.n_slices(L["s25"]["heads"]) == HB.HB_MAX_SLICES + 1
    assert HB.n_slices(L["n80"]["heads"]) == 4 and HB.n_slices(L["ll"]["heads"]) == 3
    for name, l in L.items():       # rows and channels of the heads lie inside the tensors and do not overlap
        rows, chans = [], []
        for row0, nrows, ch0, nch in l["heads"]:
            rows += range(row0, row0 + nrows)
            chans += range(ch0, ch0 + nch)
        assert len(set(rows)) == len(rows) and max(rows) < l["n_out"] and len(set(chans)) == len(chans) and max(chans) < l["Ct"], name
    assert sorted(L["ll"]["heads"]) == sorted(L["ll_reordered"]["heads"]) and L["ll"]["heads"] != L["ll_reordered"]["heads"]
    for name, C in HB.C_LAYOUT_C.items():     # the three-launch form: every channel of mid belongs to a 3-row head; Ct a multiple of 8
        l = L[name]
        assert all(h[1] == 3 for h in l["heads"]) and sum(h[3] for h in l["heads"]) == l["Ct"] and l["Ct"] % 8 == 0, name
    assert {C - (C - 1) // 16 * 16 for C, _ct in HB.B_CHANNELS} >= {2, 8}           # last channel groups of 2 and 8 channels
    assert max(((C + 63) // 64) * ((Ct + 63) // 64) for C, Ct in HB.B_CHANNELS) == 9


def test_fused_admission_rule():
    for shape, _why in HB.D_SHAPES:
        for n_out, heads in HB.D_LAYOUTS.values():
            assert HB.head_bwd_fused_ok(*shape, heads, 64, 32, "reflect"), (shape, heads)
    for shape, pad, with_dx, why in HB.D_NOT_ADMITTED:
        assert not HB.head_bwd_fused_ok(*shape, HB.D_LAYOUTS["r03"][1], 64, 32, pad, with_dx), why
        B, H, W = shape       # ... for the one reason the row names
        assert (W % 4 != 0, (H * W) % 64 != 0, pad != "reflect", not with_dx).count(True) == 1 and H >= 4 and W >= 4, why
    assert not HB.head_bwd_fused_ok(1, 4, 16, HB.D_LAYOUTS["r03"][1], 64, 32, "reflect", switch=False)
    for name, C in HB.C_LAYOUT_C.items():
        l = HB.LAYOUTS[name]
        assert not HB.head_bwd_fused_ok(2, 8, 64, l["heads"], l["Ct"], C, "reflect"), name
    # a 3x3 workspace one float short of the fused need still holds the three-launch form's at the shape that test uses
    q, need3, fused = HB.workspace3x3(2051, 4, 16, HB.D_LAYOUTS["r03"][1])
    assert q == fused and need3 <= fused - 1


# a copy of test_host_logic._HEAD_BWD_WORKSPACE_PINS: (B, H, W, heads, Ct, C) -> the 3x3 query, the 3x3 stage's own need, the 1x1 query
_PINS = [
    ((12, 96, 320, [(0, 3, 0, 32), (3, 3, 32, 32)], 64, 32), 2113536, 1056768, 2129920),
    ((12, 48, 160, [(0, 3, 0, 64), (3, 3, 64, 64)], 128, 64), 1486080, 1056768, 2995200),
    ((12, 24, 80, [(0, 3, 0, 128), (3, 3, 128, 128)], 256, 128), 743040, 743040, 2995200),
    ((2, 6, 20, [(0, 1, 0, 64), (1, 3, 64, 256), (4, 3, 320, 256)], 576, 256), 18576, 18576, 149760),
    ((1, 8, 8, [(0, 3, 0, 32)], 64, 32), 2064, 2064, 4160),
]


def test_rederived_block_counts_reproduce_the_pinned_workspace_answers():
    for (B, H, W, heads, Ct, C), q3, need3, q1 in _PINS:
        got = HB.workspace3x3(B, H, W, heads)
        assert got[:2] == (q3, need3) and HB.workspace1x1(B, H, W, C, Ct) == q1, (B, H, W)
