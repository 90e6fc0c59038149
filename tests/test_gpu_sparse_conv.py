"""wmd_sparse_conv (wmd_sparse.hip, sparse_conv_kernel<MR, TAPS, DUAL, WK, UN, ROWS>) held against the float64 oracle of
sparse_conv_ref.py, instantiation by instantiation: the 3x3 with row windows, the 3x3 on maps narrower than a window and the 1x1,
each at MR = 1, 2, 4 and in the dual form -- the 12 instantiations the host launches.

Every output is a view inside a NaN-filled buffer with a guard band on each side (pin_harness.Bufs): a store outside y shows in the
bands, a listed pixel that is never written stays NaN inside y, and every pixel that is not listed must still be NaN.  The launch
profile names the instantiation that ran, and every run asserts the one the mirror of the host's rules (sparse_conv_ref.select)
expects.  Pixel lists come from the compaction kernel (raster order) and, by hand, in a random order with the entries past the
count pointing at pixels that are not listed.

Tolerances are measured, not chosen: for every compared tensor, on the same inputs,
    e_ref = max |oracle32 - oracle64| / max |oracle64|     the oracle in float32 against itself in float64
    e_hip = max |hip      - oracle64| / max |oracle64|
over every listed pixel of every channel, and the assertion is e_hip <= F[kind] * e_ref + 4 * 2^-23."""
import os
import re
import subprocess
import sys

import pytest
import torch

import pin_harness as P
import sparse_conv_ref as SR
from pin_harness import Bufs, untouched, written

pytestmark = pytest.mark.gpu

# per kind, the smallest power of two >= twice the largest need_F measured on the MI355X (profiles/sparse_conv_pins.md; DESIGN.md
# §4.6.5); 1 where no comparison of the kind exceeds the floor
F = {"y3": 1, "y1": 1, "ydual": 1}
assert max(F.values()) <= 16
# the host's switches, read once per process there: the mirror follows them (the children below run under two of them)
def _atoi(name, default):
    if name not in os.environ:
        return default
    m = re.match(r"\s*[-+]?\d+", os.environ[name])
    return int(m.group()) if m else 0


GRID, MR_FORCE, SPLIT_WAVES = _atoi("WMD_SPARSE_GRID", 2048), _atoi("WMD_SPARSE_MR", 0), _atoi("WMD_SPARSE_SPLIT_WAVES", 2048)
ROWS_ON = _atoi("WMD_SPARSE_ROWS", 1) != 0
SEEN, RAN = set(), set()          # the instantiations the profile has named, the table rows that ran


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


class Checks(P.Checks):
    """pin_harness.Checks on this module's F table"""

    def __init__(self, case):
        super().__init__(case, F)


_MEMO = {}


def memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def operands(c):
    return memo(("in", c["key"]), lambda: SR.inputs(c))


def to_dev(dev, d):
    """a case's operands on the device, in the wrapper's form (no batch dimension at B = 1), weights packed"""
    from wavelet_monodepth_amd import ops
    k = {}
    for n in ("x1", "x2", "in_mask"):
        v = d[n]
        k[n] = None if v is None else (v[0] if v.shape[0] == 1 else v).to(dev).contiguous()
    for n in ("w", "w2"):
        k[n] = None if d[n] is None else ops.pack_weights(d[n].to(dev))
    for n in ("b", "b2"):
        k[n] = None if d[n] is None else d[n].to(dev)
    return k


def expected(c, max_out):
    return SR.case_select(c, max_out, grid_target=GRID, rows_on=ROWS_ON, mr_force=MR_FORCE)


def launch(dev, c, k, coords, counts, max_out, pad, split_waves=0, nnz_stride=1):
    """one wmd_sparse_conv call into a guarded NaN buffer -> (y [B,Cout,H,W] view, bufs); the profile must name exactly the expected
    instantiation, once.  coords: device int32 [B,max_out] (or [max_out]); counts: a device int32 tensor, frame f's count at f * nnz_stride."""
    from wavelet_monodepth_amd import _lib, sparse_ops as S
    B = c["B"]
    bufs = Bufs(dev)
    y = bufs.new("y", B, c["Cout"], c["H"], c["W"])
    assert y.data_ptr() % 16 == 0 and coords.dtype == torch.int32 and counts.dtype == torch.int32 and coords.numel() >= B * max_out
    assert counts.numel() >= (B - 1) * nnz_stride + 1
    _lib.profile_begin()
    S.sparse_conv(y if B > 1 else y[0], k["x1"], k["w"], k["b"], c["Cout"], c["ksize"], coords, counts.data_ptr(), max_out, x2=k["x2"], up1=c["up1"],
                  in_mask=k["in_mask"], pad=pad, act=c["act"], slope=c["slope"], out_scale=c["out_scale"], c1=c["C1"], c1_off=c["c1_off"], wp2=k["w2"],
                  bias2=k["b2"], c1_off2=c["c1_off2"], split_waves=split_waves, nnz_stride=nnz_stride if B > 1 else 0)
    ran = {r["kernel"]: r["calls"] for r in _lib.profile_end()}
    want = {expected(c, max_out)["name"]: 1} if max_out > 0 else {}
    assert ran == want, "%s: the profile shows %s, expected %s" % (c["key"], ran, want)
    # ... and the host's own answer for the same call (wmd_sparse_conv_plan) names it too, with the mirror's grid
    planned = S.sparse_conv_plan(c["H"], c["W"], c["C1"], c["Cout"], c["ksize"], max_out, B=B, up1=c["up1"], C2=c["C2"], C1tot=c["C1tot"], c1_off=c["c1_off"],
                                 dual=c["dual"], c1_off2=c["c1_off2"], pad=pad, act=c["act"], split_waves=split_waves)
    assert planned == ((expected(c, max_out)["name"], expected(c, max_out)["grid_x"]) if max_out > 0 else (None, 0)), (c["key"], planned)
    SEEN.update(ran)
    return y, bufs


def compare(chk, c, what, y, bufs, o32, o64):
    """every listed pixel of every channel against the oracle; everything else must still be NaN, the guard bands intact"""
    bufs.bands(what)
    listed = ~torch.isnan(o64)
    assert bool((listed == listed[:, :1]).all())
    got = y.cpu()
    untouched(got[~listed], what + ": pixels that are not listed")
    if bool(listed.any()):
        written(got[listed], what + ": listed pixels")
        chk.add(c["kind"], what, got, o32, o64, keep=listed)
    return got


def lists_on_device(dev, c, density):
    """-> {order: (coords, counts) on the device}, the CPU raster lists for the oracle.  "compact": the compaction kernel's raster
    lists (what lies past the count is whatever the allocation held); "hand": random order, stale entries at unlisted pixels."""
    from wavelet_monodepth_amd import sparse_ops as S
    om = SR.out_mask(c, density)
    rc, rn = SR.raster_lists(om)
    md = om.to(torch.uint8).to(dev)
    (cc,), cn = S.compact_multi([md if c["B"] > 1 else md[0]])
    assert cn.cpu().reshape(-1).tolist() == rn
    for f in range(c["B"]):
        assert torch.equal(cc.reshape(c["B"], -1)[f, :rn[f]].cpu(), rc[f, :rn[f]])
    out = {"compact": (cc, cn.reshape(-1))}
    if density in ("30", "17"):
        hc, hn = SR.hand_lists(c, om, density)
        out["hand"] = (hc.to(dev), torch.tensor(hn, dtype=torch.int32, device=dev))
    return out, (rc, rn)


def oracles(c, d, rc, rn, max_out, pad, key):
    return memo(("o", c["key"], pad) + key, lambda: tuple(SR.oracle(c, d, rc, rn, max_out, pad, dt) for dt in (torch.float32, torch.float64)))


def run_case(dev, key, chk=None):
    """every padding x density x list order of a table row"""
    c = SR.CASES[key]
    if (ROWS_ON, MR_FORCE) == (True, 0):
        assert expected(c, c["H"] * c["W"])["name"] == SR.want_name(c), "%s no longer selects %s" % (key, SR.want_name(c))
    own = chk is None
    chk = Checks(key) if own else chk
    d = operands(c)
    k = memo(("dev", key), lambda: to_dev(dev, d))
    npix = c["H"] * c["W"]
    for density in c["dens"]:
        lists, (rc, rn) = lists_on_device(dev, c, density)
        for pad in c["pads"]:
            o32, o64 = oracles(c, d, rc, rn, npix, pad, (density,))
            for order, (coords, counts) in lists.items():
                what = "%s %s %s" % (pad, density, order)
                y, bufs = launch(dev, c, k, coords, counts, npix, pad, split_waves=c["split_waves"])
                compare(chk, c, what, y, bufs, o32, o64)
    RAN.add(key)
    if own:
        chk.done()


SMALL = [c["key"] for c in SR.TABLE if not c["key"].startswith("loop_")]


@pytest.mark.parametrize("key", SMALL)
def test_sparse_conv_vs_oracle(dev, key):
    """Every row of the table but the two task-loop rows: every pixel, about 30 %, one pixel, 17 pixels (two tiles, the second with one
    live lane) and none (y stays NaN), raster lists from the compaction kernel and hand-made lists in a random order."""
    run_case(dev, key)


def test_task_loop_at_default_settings(dev):
    """8 frames of 66x63 at full density: grid.x = 256 < 260 tiles, so blocks 0..3 fetch the pixels of a second task (S = WK)"""
    c = SR.CASES["loop_default"]
    s = expected(c, c["H"] * c["W"])
    if (GRID, SPLIT_WAVES) == (2048, 2048):
        assert s["grid_x"] == 256 < s["tiles"] == 260 and SR.k_slices(260, 8, SPLIT_WAVES) == 8
    run_case(dev, "loop_default")


def test_task_loop_with_merged_k_slices(dev):
    """64 frames of 66x63 under split_waves = 1: S = 1, 8 tiles per block, 33 tasks over grid.x = 32 blocks"""
    c = SR.CASES["loop_s1"]
    s = expected(c, c["H"] * c["W"])
    assert SR.k_slices(260, 8, 1) == 1
    if GRID == 2048:
        assert s["grid_x"] == 32 < -(-s["tiles"] // 8) == 33
    run_case(dev, "loop_s1")


# ---- count and list edges, on the 40x36 row ------------------------------------------------------------------------------------------
def test_a_count_above_max_out_is_clamped(dev):
    """the device count says max_out + 5 and the lists are longer than max_out: exactly the first max_out entries are written"""
    c = SR.CASES["rows_mr2"]
    d = operands(c)
    k = memo(("dev", c["key"]), lambda: to_dev(dev, d))
    om = SR.out_mask(c, "30")
    hc, hn = SR.hand_lists(c, om, "30")
    max_out = min(hn) - 37
    assert max_out > 16 and max_out % 16 != 0
    coords = hc[:, :max_out].contiguous()                      # out_coords [B,max_out]: every frame's list is cut at max_out
    counts = [max_out + 5] * c["B"]
    chk = Checks("count > max_out")
    for pad in c["pads"]:
        o32, o64 = oracles(c, d, coords, counts, max_out, pad, ("clamp",))
        assert int((~torch.isnan(o64[:, 0])).sum()) == c["B"] * max_out
        y, bufs = launch(dev, c, k, coords.to(dev), torch.tensor(counts, dtype=torch.int32, device=dev), max_out, pad)
        compare(chk, c, pad, y, bufs, o32, o64)
    chk.done()


def test_batched_counts_n_0_1_through_a_count_stride(dev):
    """frames with counts n, 0 and 1, three int32 apart; the words between them say `every pixel`"""
    c = SR.CASES["rows_mr2"]
    d = operands(c)
    k = memo(("dev", c["key"]), lambda: to_dev(dev, d))
    npix = c["H"] * c["W"]
    hc, hn = SR.hand_lists(c, SR.out_mask(c, "30"), "30")
    counts = [hn[0], 0, 1]
    cnt = torch.full((c["B"], 3), npix, dtype=torch.int32)
    cnt[:, 0] = torch.tensor(counts, dtype=torch.int32)
    chk = Checks("counts n,0,1")
    for pad in c["pads"]:
        o32, o64 = oracles(c, d, hc, counts, npix, pad, ("n01",))
        assert [int((~torch.isnan(o64[f, 0])).sum()) for f in range(3)] == counts
        y, bufs = launch(dev, c, k, hc.to(dev), cnt.to(dev), npix, pad, nnz_stride=3)
        compare(chk, c, pad, y, bufs, o32, o64)
    chk.done()


def test_entries_past_the_count_are_never_used(dev):
    """a raster list whose entries past the count are overwritten with in-range indices of pixels that are not listed, at a count that
    is no multiple of 16 (dead lanes borrow a live pixel): those pixels stay NaN"""
    from wavelet_monodepth_amd import sparse_ops as S
    c = SR.CASES["rows_mr2"]
    d = operands(c)
    k = memo(("dev", c["key"]), lambda: to_dev(dev, d))
    npix = c["H"] * c["W"]
    om = SR.out_mask(c, "30")
    rc, rn = SR.raster_lists(om)
    (cc,), cn = S.compact_multi([om.to(torch.uint8).to(dev)])
    stale, _n = SR.hand_lists(c, om, "30")
    cc = cc.clone()
    assert rn[0] % 16 != 0 and rn[1] % 16 != 0
    for f in range(c["B"]):
        cc[f, rn[f]:] = stale[f, rn[f]:].to(dev)
        assert not bool(om[f].reshape(-1)[stale[f, rn[f]:].long()].any())
    chk = Checks("stale entries")
    o32, o64 = oracles(c, d, rc, rn, npix, "reflect", ("30",))
    y, bufs = launch(dev, c, k, cc, cn.reshape(-1), npix, "reflect")
    compare(chk, c, "reflect", y, bufs, o32, o64)
    chk.done()


# ---- selection, not multiplication ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["rows_mr2", "rows_mr4", "rows_w1_3", "narrow_w1_2", "narrow_w2", "dual_rows", "dual_narrow", "dual_gap", "slice"])
def test_masked_inputs_are_selected_not_multiplied(dev, key):
    """NaN / +-Inf in x2 and x1 wherever in_mask is 0 (up1 = 2: the coarse pixels whose four fine pixels are all masked) and in the x1
    channels no slice owns: the output has the bits of the run on clean operands (every consumer selects on its mask)"""
    c = SR.CASES[key]
    d = operands(c)
    q = SR.poisoned(c, d)
    assert not bool(torch.isfinite(q["x1"][:, c["c1_off"]:c["c1_off"] + c["C1"]]).all()) or c["up1"] == 2
    assert q["x2"] is None or not bool(torch.isfinite(q["x2"]).all())
    k, kq = memo(("dev", key), lambda: to_dev(dev, d)), to_dev(dev, q)
    npix = c["H"] * c["W"]
    chk = Checks(key + " poisoned")
    for density in ("all", "30"):
        if density not in c["dens"]:
            continue
        lists, (rc, rn) = lists_on_device(dev, c, density)
        coords, counts = lists["compact"]
        for pad in c["pads"]:
            o32, o64 = oracles(c, d, rc, rn, npix, pad, (density,))
            clean, _b = launch(dev, c, k, coords, counts, npix, pad)
            y, bufs = launch(dev, c, kq, coords, counts, npix, pad)
            compare(chk, c, "%s %s poisoned" % (pad, density), y, bufs, o32, o64)
            assert torch.equal(y.view(torch.int32), clean.view(torch.int32)), "%s %s %s: poison behind the mask changed the output" % (key, pad, density)
    chk.done()


# ---- K-slice modes -------------------------------------------------------------------------------------------------------------------
def run_modes(dev, key, chk):
    """split_waves = 1, ntile + 1 and 2^30 -> 1, 2 and WK K slices per tile (frame 0; the device decides per frame): each within the
    bound, two runs of a mode bit-identical (the LDS reduction has a fixed order)"""
    c = SR.CASES[key]
    d = operands(c)
    k = memo(("dev", key), lambda: to_dev(dev, d))
    npix = c["H"] * c["W"]
    lists, (rc, rn) = lists_on_device(dev, c, "30")
    coords, counts = lists["compact"]
    ntile, WK = -(-rn[0] // 16), expected(c, npix)["WK"]
    modes = (1, ntile + 1, 2 ** 30)
    assert [SR.k_slices(ntile, WK, sw) for sw in modes] == [1, 2, WK]
    pad = c["pads"][0]
    o32, o64 = oracles(c, d, rc, rn, npix, pad, ("30",))
    for sw in modes:
        y, bufs = launch(dev, c, k, coords, counts, npix, pad, split_waves=sw)
        compare(chk, c, "%s split_waves=%d" % (pad, sw), y, bufs, o32, o64)
        again, bufs2 = launch(dev, c, k, coords, counts, npix, pad, split_waves=sw)
        bufs2.bands("the second run")
        assert torch.equal(y.view(torch.int32), again.view(torch.int32)), "%s split_waves=%d: two runs differ" % (key, sw)


@pytest.mark.parametrize("key", ["rows_mr2", "k1_mr2", "dual_rows"])
def test_every_k_slice_mode_vs_oracle_and_run_to_run(dev, key):
    chk = Checks(key + " modes")
    run_modes(dev, key, chk)
    chk.done()


# ---- the host's switches, in child processes (they are read once per process) ----------------------------------------------------------
def child_grid3(dev):      # WMD_SPARSE_GRID=3: one to three blocks per frame and out-channel group, every block walks many tasks
    assert GRID == 3 and ROWS_ON
    for key in ("rows_w3", "rows_mr2", "rows_mr4", "k1_mr4", "dual_rows"):
        assert expected(SR.CASES[key], SR.CASES[key]["H"] * SR.CASES[key]["W"])["grid_x"] <= 3
        run_case(dev, key)


def child_rows_off(dev):   # WMD_SPARSE_ROWS=0: the per-tap gather on maps wide enough for row windows
    assert not ROWS_ON and GRID == 2048
    for key in ("rows_w3", "rows_mr2", "rows_mr4"):
        assert expected(SR.CASES[key], SR.CASES[key]["H"] * SR.CASES[key]["W"])["name"].endswith(",false>")
        run_case(dev, key)
    assert SEEN == {"sparse_conv_kernel<%d,9,false,8,2,false>" % mr for mr in (1, 2, 4)}, SEEN


_CHILD = "import sys, torch, test_gpu_sparse_conv as T; getattr(T, sys.argv[1])(torch.device('cuda:0'))"


def run_child(fn, switch, value):
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if not k.startswith("WMD_SPARSE_")}
    env[switch] = value
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(here), here, env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, "-c", _CHILD, fn], env=env, capture_output=True, text=True, timeout=120)
    print("".join("%s=%s %s\n" % (switch, value, line) for line in r.stdout.splitlines() if line.startswith("EDGE")), end="")
    assert r.returncode == 0, "%s=%s: exit status %d\n%s\n%s" % (switch, value, r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_three_block_grid_in_a_child_process():
    """WMD_SPARSE_GRID=3: the MR 1 / 2 / 4 ROWS rows, the 1x1 MR 4 row and the dual ROWS row with every block walking many tasks"""
    run_child("child_grid3", "WMD_SPARSE_GRID", "3")


def test_row_windows_off_in_a_child_process():
    """WMD_SPARSE_ROWS=0: the three ROWS rows on the per-tap gather, pinned to the same oracle; the profile shows ROWS = false"""
    run_child("child_rows_off", "WMD_SPARSE_ROWS", "0")


def test_every_instantiation_ran(dev):
    """All 12 instantiations appear in the profile records of this module's run (a partial run of the module first runs the table rows
    it has not run)."""
    for c in SR.TABLE:
        if c["key"] not in RAN:
            run_case(dev, c["key"])
    if (GRID, ROWS_ON, MR_FORCE) == (2048, True, 0):
        assert SEEN == set(SR.ALL_INSTANTIATIONS), sorted(set(SR.ALL_INSTANTIATIONS) ^ SEEN)
