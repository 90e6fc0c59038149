"""The 6x20 tile of the quarter-position Winograd family (conv_wino32q_kernel<6,20,8>), checked without a GPU.

W32QTile used to ask for TW % 8 == 0; the 6x20 tile has TXB = TW / 2 = 10 Winograd tiles per tile row and 30 of the 32 tile slots
of an MFMA operand.  The kernel's slot arithmetic is restated here (wmd_conv_wino32q.hip: "operand addressing" and store_lines) and
walked exhaustively: what the relaxed assert (TW % 4 == 0, i.e. TXB even) has to guarantee is that every output pixel of the tile
is stored exactly once, inside the tile, in 16-byte pieces that never leave their row and sit on a 16-byte boundary.  8x16 and 4x32
are the controls; a 4x10 tile (TXB = 5, refused by the assert) shows that the walk does catch a slot pair that straddles tile rows.
"""
import collections
import ctypes as C

import pytest

NEW = "conv_wino32q_kernel<6,20,8>"


def operand_slot(lane, TH, TW):
    """lane -> (tyy, txx): the Winograd tile whose patch the lane feeds into row lane & 31 of the MFMA's pixel operand"""
    TXB, NTILES = TW // 2, (TH // 2) * (TW // 2)
    tslot = min(lane & 31, NTILES - 1)
    return tslot // TXB, tslot % TXB


def store_lines(R, lane, i, TH, TW):
    """Quarter R's store instruction i of lane `lane` -> (channel of the slab, oy, ox, [tile slot, pixel column] of the four floats) or
    None when the piece is beyond the tile's slots.  Quarter R finishes output row A = R >> 1 of the tile slots [16 (R & 1), +16);
    piece pc holds the slot pair (2 pc, 2 pc + 1): float4(slot0[A][0], slot0[A][1], slot1[A][0], slot1[A][1])."""
    TXB, NTILES = TW // 2, (TH // 2) * (TW // 2)
    A = R >> 1
    cc, pc = 8 * i + (lane >> 3), lane & 7
    ts = 16 * (R & 1) + 2 * pc
    if ts >= NTILES:
        return None
    oy, ox = (ts // TXB) * 2 + A, (ts % TXB) * 2
    return cc, oy, ox, [(ts, 0), (ts, 1), (ts + 1, 0), (ts + 1, 1)]


def walk(TH, TW):
    """-> list of defects of the store pattern of one block (empty: every pixel of every channel exactly once, in place)"""
    TXB, NTILES = TW // 2, (TH // 2) * (TW // 2)
    bad, written = [], collections.Counter()
    for R in range(4):
        for i in range(4):
            for lane in range(64):
                st = store_lines(R, lane, i, TH, TW)
                if st is None:
                    continue
                cc, oy, ox, src = st
                if ox % 4:
                    bad.append("piece at column %d is not on a 16-byte boundary" % ox)
                if ox + 3 >= TW or oy >= TH:
                    bad.append("piece (%d, %d..%d) leaves the %dx%d tile" % (oy, ox, ox + 3, TH, TW))
                for e, (slot, col) in enumerate(src):
                    if slot >= NTILES:
                        bad.append("piece of slots %d, %d reads slot %d of %d" % (src[0][0], src[2][0], slot, NTILES))
                        continue
                    # where the slot's pixel (row A = R >> 1, column col) really lies -- the operand side's tslot / TXB, tslot % TXB
                    ty, tx = slot // TXB, slot % TXB
                    want = (ty * 2 + (R >> 1), tx * 2 + col)
                    if want != (oy, ox + e):
                        bad.append("slot %d pixel %s stored at %s" % (slot, want, (oy, ox + e)))
                    written[(cc, oy, ox + e)] += 1
    for cc in range(32):
        for y in range(TH):
            for x in range(TW):
                if written[(cc, y, x)] != 1:
                    bad.append("channel %d pixel (%d, %d) stored %d times" % (cc, y, x, written[(cc, y, x)]))
    if len(written) != 32 * TH * TW:
        bad.append("%d distinct stores for %d outputs" % (len(written), 32 * TH * TW))
    return bad


@pytest.mark.parametrize("TH,TW", [(6, 20), (8, 16), (4, 32)], ids=["6x20", "8x16", "4x32"])
def test_store_lines_writes_every_pixel_of_the_tile_once(TH, TW):
    bad = walk(TH, TW)
    assert not bad, "%dx%d: %s" % (TH, TW, bad[:5])


def test_the_walk_catches_a_slot_pair_that_straddles_tile_rows():
    """TXB = 5 (a 4x10 tile, which W32QTile's assert refuses): the pair (4, 5) is the end of one tile row and the start of the next"""
    bad = walk(4, 10)
    assert any("stored at" in b or "leaves" in b for b in bad)


@pytest.mark.parametrize("TH,TW", [(6, 20), (8, 16), (4, 32)], ids=["6x20", "8x16", "4x32"])
def test_operand_slots_cover_the_tile_and_match_the_accumulator_layout(TH, TW):
    """Every Winograd tile of the pixel tile is some lane's operand row, the rows past NTILES repeat the last tile (their results are
    never stored), both 32-lane halves (the two channels of a K-step) address the same tile, and the patch reads stay inside the
    staged (TH + 2) x (TW + 2) patch."""
    TXB, TYB = TW // 2, TH // 2
    tiles = [operand_slot(l, TH, TW) for l in range(64)]
    assert tiles[:32] == tiles[32:]
    assert set(tiles) == {(y, x) for y in range(TYB) for x in range(TXB)}
    for s, (ty, tx) in enumerate(tiles[:32]):
        assert (ty, tx) == (min(s, TXB * TYB - 1) // TXB, min(s, TXB * TYB - 1) % TXB)
        assert 2 * ty + 3 < TH + 2 and 2 * tx + 3 < TW + 2       # rows RA / RB <= 3, two 8-byte reads of columns 0..3


def test_6x20_geometry_and_patch_read_banks():
    """W32QTile<6,20,8> restated: an even patch row stride and plane (8-byte reads), dword staging (no 16-byte row groups), under the
    three-blocks-per-CU bound; and the 8-byte patch reads of a 32-lane half -- floats 44 tyy + 2 txx (+ a lane-independent offset),
    banks (address / 4) % 64 -- touch 60 distinct banks: the three tile rows fall on banks 0-19, 44-63 and 24-43."""
    TH, TW, CK = 6, 20, 8
    PWS, PH = TW + 2, TH + 2
    PSF = PH * PWS
    assert (PWS, PSF) == (22, 176) and PWS % 2 == 0 and PSF % 2 == 0 and TW % 16 != 0
    B_FLOATS = -(-CK * PSF // 256) * 256
    A_FLOATS = 2 * (CK * 256 + 16)
    TAB = -(-(PH + PWS + TH // 2 + 2 + TW // 2 + 2) // 4) * 4
    lds_bytes = 4 * (2 * (B_FLOATS + A_FLOATS) + TAB + 8)
    assert lds_bytes == 45536 and lds_bytes <= 53 * 1024
    banks = collections.Counter()
    for ty, tx in set(operand_slot(l, TH, TW) for l in range(32)):     # identical addresses broadcast
        a = 2 * PWS * ty + 2 * tx
        banks[a % 64] += 1
        banks[(a + 1) % 64] += 1
    assert len(banks) == 60 and max(banks.values()) == 1


def test_the_entry_is_in_the_table_and_the_cost_model_takes_it_on_the_coarsest_map():
    """tuner.config_names() lists the entry; with nothing forced (what a stream capture on a tuner miss and WMD_AUTOTUNE=0 run) the
    coarsest layer of the 640x192 forward at batch 12 -- twelve 6x20 maps -- goes to it, split: every other 32x32x2 tile executes
    at least twice its tile slots there, and the model charges executed slots."""
    from wavelet_monodepth_amd import _lib, tuner
    names = tuner.config_names()
    assert NEW in names and len(set(names)) == len(names)
    a = _lib.ConvArgs(ksize=3, pad_mode=1, act=1, x1=1, wp=1, y=1, wp_wino=1, B=12, H=6, W=20, C1=512, up1=1, C2=0, Cout=256)
    ks = C.c_int(0)
    i = _lib.lib().wmd_conv_fwd_plan(C.byref(a), C.byref(ks))
    assert names[i] == NEW and ks.value > 1, (names[i], ks.value)
    # forced by index with the split the issue's layer table names: accepted, eight slices
    a.tune_cfg, a.tune_ksplit = names.index(NEW) + 1, 8
    assert _lib.lib().wmd_conv_fwd_plan(C.byref(a), C.byref(ks)) == names.index(NEW) and ks.value == 8
    assert _lib.lib().wmd_conv_fwd_workspace_floats(C.byref(a)) == 8 * 12 * 256 * 120
    a.tune_cfg = len(names) + 1
    assert _lib.lib().wmd_conv_fwd_plan(C.byref(a), None) == -1
