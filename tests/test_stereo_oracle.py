"""CPU: the numpy oracle of the semi-global matcher (tests/stereo_ref.py) does what a matcher should on a pair whose answer is
known, its stages obey their rules on hand-made inputs, and the library's two stereo entries refuse bad arguments before any
HIP call.  The bounds of the synthetic pair are conditions set with the feature, not measurements."""
import numpy as np
import pytest

import stereo_cases
import stereo_ref as R
from wavelet_monodepth_amd import _lib, stereo


@pytest.mark.parametrize("directions", [5, 8])
@pytest.mark.parametrize("reverse", [False, True])
def test_synthetic_pair_is_recovered(directions, reverse):
    left, right, true = R.synthetic_pair()
    s = R.reference_like(16, 3, directions=directions)
    # reverse: the base image is the right view; mirrored, it is the left view of a pair with the same shifts
    out = R.sgbm(right if reverse else left, left if reverse else right, s, reverse=reverse)
    disp = out["disp"].astype(np.int64)
    band, rect = (disp[:, -16:], disp[:, :-16]) if reverse else (disp[:, :16], disp[:, 16:])
    assert (band == -16).all()
    valid = rect != -16
    near = np.abs(rect - 16 * true[:, None]) <= 8
    print("directions %d reverse %d: %.1f %% valid, %.1f %% of them within 8/16 px" % (directions, reverse, 100 * valid.mean(),
                                                                                     100 * (near & valid).sum() / valid.sum()))
    assert valid.mean() >= 0.95
    assert (near & valid).sum() >= 0.97 * valid.sum()


def test_reverse_is_the_mirror_of_the_plain_run():
    left, right, _ = R.synthetic_pair()
    s = R.reference_like(16, 3)
    a = R.sgbm(left, right, s)
    b = R.sgbm(left[:, ::-1], right[:, ::-1], s, reverse=True)
    assert np.array_equal(a["disp"], b["disp"][:, ::-1]) and np.array_equal(a["S"], b["S"])


@pytest.mark.parametrize("minD", [0, 3])
def test_constant_images(minD):
    img = np.full((9, 40, 3), 77, dtype=np.uint8)
    s = R.reference_like(16, 3, minDisparity=minD, directions=8)
    out = R.sgbm(img, img, s)
    assert not out["cost"].any() and not out["S"].any()
    x0 = minD + 16
    assert (out["disp"][:, x0:] == minD * 16).all() and (out["disp"][:, :x0] == (minD - 1) * 16).all()


@pytest.mark.parametrize("directions", [5, 8])
@pytest.mark.parametrize("block,C", [(1, 3), (3, 3), (3, 1), (5, 1)])
def test_s_bound(directions, block, C):
    """S <= directions * (win^2 C (2 cap + 63) + P2): on noise against noise the observed maximum stays below it, and the
    reference's settings give the 43,128 that DESIGN.md quotes"""
    assert R.s_bound(R.reference_like(160, 3, directions=8), 3) == 43128
    rng = np.random.default_rng(5)
    left, right = (rng.integers(0, 256, (8, 30, C)).astype(np.uint8) for _ in range(2))
    s = R.reference_like(16, block, directions=directions)
    out = R.sgbm(left, right, s)
    win = 2 * (block // 2) + 1
    print("max C %d of %d, max S %d of %d" % (out["cost"].max(), win * win * C * 189, out["S"].max(), R.s_bound(s, C)))
    assert out["cost"].max() <= win * win * C * (2 * 63 + 63)
    assert 0 < out["S"].max() <= R.s_bound(s, C)


def test_trunc_div_rounds_toward_zero():
    assert [R.trunc_div(a, 4) for a in (-9, -8, -7, -1, 0, 1, 7, 9)] == [-2, -2, -1, 0, 0, 0, 1, 2]


@pytest.mark.parametrize("name", stereo_cases.SPECKLE_CASES)
def test_speckle_oracle_on_hand_made_maps(name):
    case = stereo_cases.speckle_case(name)
    out = R.filter_speckles(case["disp"].astype(np.int64), case["invalid"], case["max_size"], case["max_diff"])
    kept = out != case["invalid"]
    assert np.array_equal(kept, case["kept"]), name
    assert np.array_equal(out[kept], case["disp"][kept])


def test_the_gpu_cases_cover_what_they_claim():
    """what the GPU tests compare against: the plain pairs are mostly valid before the speckle stage, the noise cases mostly
    invalid with speckles that are removed and others that stay, the uniqueness case differs from the base case"""
    out = {n: R.sgbm(*stereo_cases.sgbm_inputs(n), stereo_cases.settings(n)) for n in stereo_cases.SGBM_CASES}
    for n in stereo_cases.TABLE:
        s = stereo_cases.settings(n)
        x0 = s.minDisparity + s.numDisparities
        assert (out[n]["raw"][:, x0:] != (s.minDisparity - 1) * 16).mean() > 0.8, n       # one_column_6x17: five of its six pixels
    for n in ("right_view_noise", "speckles_bite"):
        raw, disp = out[n]["raw"], out[n]["disp"]
        assert (raw == -16).mean() > 0.5 and 0 < (raw != disp).sum() < (raw != -16).sum(), n
    assert not np.array_equal(out["uniqueness_0"]["disp"], out["base_20x72_d16_b3_5"]["disp"])
    assert np.array_equal(out["speckles_off"]["raw"], out["speckles_off"]["disp"])
    assert np.array_equal(out["speckles_off"]["raw"], out["base_20x72_d16_b3_5"]["raw"])


def test_reference_settings_are_the_twelve():
    ss = stereo.reference_settings()
    assert [(s.blockSize, s.numDisparities) for s in ss] == [(b, n) for b in (1, 2, 3) for n in (64, 96, 128, 160)]
    assert all((s.P1, s.P2, s.preFilterCap, s.uniquenessRatio, s.speckleWindowSize, s.speckleRange, s.minDisparity, s.directions)
               == (36, 288, 63, 10, 100, 16, 0, 5) for s in ss)
    assert ss[0].invalid == -16 and [s.window for s in ss[::4]] == [1, 3, 3]


def sgbm_call(lib, left=1, right=1, disp=1, ws=1, ws_bytes=None, B=1, H=8, W=40, C=3, minD=0, D=16, block=3, P1=36, P2=288, cap=63,
              uniq=10, sw=100, sr=16, d12=0, dirs=5):
    need = lib.wmd_stereo_sgbm_workspace_bytes(B, H, W, C, minD, D, block)
    return lib.wmd_stereo_sgbm(left, right, None, disp, None, None, B, H, W, C, minD, D, block, P1, P2, cap, uniq, sw, sr, d12, dirs,
                               ws if ws is None else 256, need if ws_bytes is None else ws_bytes, None)


def test_sgbm_refusals_without_gpu():
    """dummy non-null pointers never reach a kernel: every call below returns before the first HIP call"""
    lib = _lib.lib()
    BAD_ARG, BAD_SHAPE, UNSUPPORTED, WORKSPACE = -1, -2, -3, -5
    assert lib.wmd_stereo_sgbm_workspace_bytes(1, 8, 40, 3, 0, 16, 3) > 0
    for kw in (dict(left=None), dict(right=None), dict(disp=None), dict(ws=None)):
        assert sgbm_call(lib, **kw) == BAD_ARG, kw
        assert b"null" in lib.wmd_last_error()
    for kw in (dict(C=2), dict(C=4), dict(minD=-1), dict(D=24), dict(D=0), dict(D=272), dict(P1=300), dict(P1=-1), dict(dirs=4),
               dict(block=0), dict(uniq=101), dict(sw=-1), dict(cap=-1)):
        assert sgbm_call(lib, **kw) == BAD_ARG, kw
    for kw in (dict(W=16), dict(W=10), dict(W=19, minD=3), dict(H=0), dict(B=0)):
        assert sgbm_call(lib, **kw) == BAD_SHAPE, kw
        assert lib.wmd_stereo_sgbm_workspace_bytes(kw.get("B", 1), kw.get("H", 8), kw["W"] if "W" in kw else 40, 3, kw.get("minD", 0), 16, 3) == 0
    # S would not fit 16 bits: 8 * (25 * 3 * 189 + 288) and a P2 of 60000; the reference's own settings at 8 directions fit
    for kw in (dict(block=5, dirs=8), dict(P2=60000), dict(cap=128), dict(W=70000, D=16)):
        assert sgbm_call(lib, **kw) == UNSUPPORTED, kw
    assert sgbm_call(lib, ws_bytes=lib.wmd_stereo_sgbm_workspace_bytes(1, 8, 40, 3, 0, 16, 3) - 1) == WORKSPACE
    assert b"workspace" in lib.wmd_last_error()


def test_filter_speckles_refusals_without_gpu():
    lib = _lib.lib()
    need = lib.wmd_stereo_filter_speckles_workspace_bytes(2, 5, 7)
    assert need >= 2 * 5 * 7 * 8 and lib.wmd_stereo_filter_speckles_workspace_bytes(2, 0, 7) == 0
    assert lib.wmd_stereo_filter_speckles(None, 2, 5, 7, -16, 10, 16, 256, need, None) == -1
    assert lib.wmd_stereo_filter_speckles(256, 2, 5, 7, -16, 10, 16, None, need, None) == -1
    assert lib.wmd_stereo_filter_speckles(256, 2, 0, 7, -16, 10, 16, 256, need, None) == -2
    assert lib.wmd_stereo_filter_speckles(256, 2, 5, 7, -16, -1, 16, 256, need, None) == -1
    assert lib.wmd_stereo_filter_speckles(256, 2, 5, 7, -16, 10, 16, 256, need - 1, None) == -5


def test_python_layer_refuses_cpu_tensors():
    import torch
    img = torch.zeros(1, 4, 40, 3, dtype=torch.uint8)
    with pytest.raises(_lib.WmdError):
        stereo.sgbm(img, img, stereo.reference_settings()[0])
    with pytest.raises(_lib.WmdError):
        stereo.filter_speckles(torch.zeros(4, 4, dtype=torch.int16), -16, 3, 16)
    with pytest.raises(_lib.WmdError):
        stereo.depth_hint_candidates(img, img, False)
