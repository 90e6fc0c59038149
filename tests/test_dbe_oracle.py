"""CPU: tests/dbe_ref.py (numpy + scipy.ndimage, float64) against tests/golden/dbe_reference.npz -- the output of the
reference's own compute_depth_boundary_error with the detector bound to dbe_ref's (tests/golden/make_golden_dbe.py) -- the
condition on the inputs that makes an exact comparison of edge maps fair, and cases small enough to check by hand."""
import numpy as np
import pytest

import dbe_cases
import dbe_ref
from util import load_golden
from wavelet_monodepth_amd import evaluation as ev

MIN_MARGIN = 1e-6


@pytest.fixture(scope="module")
def gold():
    return load_golden("dbe_reference.npz")


def unpack(gold, name, shape):
    return np.unpackbits(gold[name + "|edges"])[:int(np.prod(shape))].reshape(shape).astype(bool)


@pytest.mark.parametrize("name", dbe_cases.CASES)
def test_ref_reproduces_the_fixture_and_keeps_its_margin(gold, name):
    case = dbe_cases.build(name)
    B = case["pred"].shape[0]
    want = unpack(gold, name, case["pred"].shape)
    for b in range(B):
        mask = None if case["mask"] is None else case["mask"][b]
        acc, com, edges, margin = dbe_ref.compute_depth_boundary_error(case["edges_gt"][b], case["pred"][b], mask, dbe_cases.LOW, dbe_cases.HIGH)
        assert np.array_equal(edges, want[b]), "%s[%d]: %d pixels differ" % (name, b, int((edges != want[b]).sum()))
        np.testing.assert_allclose([acc, com], gold[name + "|scores"][b], rtol=1e-12, equal_nan=True)
        # float32 (the reference) or float64 (this project) normalisation: both sides of every decision stay >= 1e-6 apart
        assert min(margin, gold[name + "|margin"][b]) >= MIN_MARGIN, (name, b, margin, gold[name + "|margin"][b])


@pytest.mark.parametrize("name,H,W,sigma,low,high", dbe_cases.CANNY_CASES)
def test_canny_cases_keep_their_margin(gold, name, H, W, sigma, low, high):
    st = dbe_ref.canny_stages(dbe_cases.canny_image(name, H, W), sigma, low, high)
    assert np.array_equal(st["edges"], unpack(gold, name, (H, W)))
    assert st["edges"].sum() > 40
    assert min(st["margin"], float(gold[name + "|margin"][0])) >= MIN_MARGIN


def test_fixture_covers_what_the_gpu_test_relies_on(gold):
    """the special scores are the special scores, truncation bites somewhere, and the scene scores are ordinary"""
    np.testing.assert_array_equal(gold["mixed|scores"][1], [10.0, 10.0])
    assert np.isnan(gold["mixed|scores"][2]).all()
    assert not unpack(gold, "mixed", (3, 40, 56))[1:].any()
    for name in dbe_cases.SCENE_CASES:
        s = gold[name + "|scores"]
        assert ((s > 0.5) & (s < 8)).all(), (name, s)
    assert np.isfinite(gold["hole|scores"]).all()
    assert ev.NYU_EDGE_NAMES == ("dbe_acc", "dbe_com")


def test_vertical_step_gives_one_edge_column():
    """a step centred on column 9 (the column itself takes the middle value): the ridge of the gradient is that column,
    on every row off the border ring"""
    img = np.zeros((16, 20))
    img[:, 9] = 0.5
    img[:, 10:] = 1.0
    edges = dbe_ref.canny(img, np.sqrt(2), 0.15, 0.3)
    want = np.zeros((16, 20), bool)
    want[1:-1, 9] = True
    assert np.array_equal(edges, want)
    assert not dbe_ref.canny(np.full((16, 20), 0.3), np.sqrt(2), 0.15, 0.3).any()


def test_normalise_turns_zeros_into_holes_and_a_constant_map_into_nan():
    p = dbe_ref.normalise(np.array([[0.0, 2.0], [4.0, 3.0]], np.float32))
    assert np.isnan(p[0, 0]) and p[0, 1] == 0.0 and p[1, 0] == 1.0 and p[1, 1] == 0.5
    assert np.isnan(dbe_ref.normalise(np.full((3, 3), 2.5, np.float32))).all()


def test_chamfer_scores_by_hand():
    """ten predicted edge pixels in column 10, rows 5..14; one ground-truth pixel at (9, 13), three columns away"""
    est = np.zeros((20, 30), bool)
    est[5:15, 10] = True
    gt = np.zeros((20, 30), bool)
    gt[9, 13] = True
    d = np.sqrt(9.0 + (np.arange(5, 15) - 9.0) ** 2)
    acc, com = dbe_ref.chamfer_scores(gt, est)
    np.testing.assert_allclose(acc, d.mean(), rtol=1e-14)
    np.testing.assert_allclose(com, (d.sum() + 3.0) / 11.0, rtol=1e-14)
    # a mask over rows 0..9 keeps five predicted pixels in F; the others count as distance 0 in dbe_com, like the reference
    mask = np.zeros((20, 30), np.uint8)
    mask[:10] = 1
    acc, com = dbe_ref.chamfer_scores(gt, est, mask)
    np.testing.assert_allclose(acc, d[:5].mean(), rtol=1e-14)
    np.testing.assert_allclose(com, (d[:5].sum() + 3.0) / 11.0, rtol=1e-14)
    # truncation: the same line 12 columns away is outside every 10-pixel neighbourhood
    gt[:] = False
    gt[9, 22] = True
    assert dbe_ref.chamfer_scores(gt, est) == (10.0, 10.0)
    # ... and with one pixel inside, the far ones are cut to 10 in dbe_com only
    est[9, 20] = True
    acc, com = dbe_ref.chamfer_scores(gt, est)
    np.testing.assert_allclose(acc, 2.0, rtol=1e-14)
    np.testing.assert_allclose(com, (2.0 + 10 * 10.0 + 2.0) / 12.0, rtol=1e-14)


def test_reach_image_is_what_it_claims():
    """the first step is strong at one end and between the thresholds over at least 64 columns, and kept whole; the second
    is between the thresholds everywhere, survives the suppression and is dropped by the hysteresis"""
    img, _ = dbe_cases.reach_image()
    st = dbe_ref.canny_stages(dbe_ref.normalise(img), np.sqrt(2), dbe_cases.LOW, dbe_cases.HIGH)
    r1, r2, W = dbe_cases.REACH["kept_row"], dbe_cases.REACH["dropped_row"], dbe_cases.REACH["W"]
    m1, m2 = st["mag"][r1, 1:W - 1], st["mag"][r2, 1:W - 1]
    assert m1[0] > dbe_cases.HIGH
    between = (m1 > dbe_cases.LOW) & (m1 < dbe_cases.HIGH)
    assert between.sum() >= 64 and between[-64:].all()
    assert st["edges"][r1, 1:W - 1].all()
    assert ((m2 > dbe_cases.LOW) & (m2 < dbe_cases.HIGH)).all()
    assert st["weak"][r2, 1:W - 1].all() and not st["edges"][r2 - 3:r2 + 4].any()
