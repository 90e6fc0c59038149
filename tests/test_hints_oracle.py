"""CPU: tests/hints_ref.py (float64, on oracle/photo_ref.py) against tests/golden/hints_reference.npz -- the float32 output
of the reference's own BackprojectDepth, Project3D, SSIM and compute_reprojection_loss in the order of
precompute_depth_hints.py's run (tests/golden/make_golden_hints.py) -- and the condition on the inputs that makes comparing
selected depths fair: nearly every pixel's best candidate wins by more than any float32 evaluation can err."""
import numpy as np
import pytest

import hints_cases
import hints_ref
from util import load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("hints_reference.npz")


@pytest.fixture(scope="module")
def oracle():
    memo = {}

    def get(name):
        if name not in memo:
            case = hints_cases.build(name)
            memo[name] = (case, hints_ref.losses(case))
        return memo[name]
    return get


def test_tol_loss_is_twice_the_references_own_error(gold):
    deltas = [float(gold[n + "|delta_ref"][0]) for n in hints_cases.CASES]
    assert float(gold["tol_loss"][0]) == 2.0 * max(deltas)
    assert 1e-6 < max(deltas) < 1e-4, deltas          # float32 SSIM on [0,1] images: E[x^2] - mu^2 cancels a few digits


@pytest.mark.parametrize("name", hints_cases.CASES)
def test_oracle_losses_are_within_delta_ref_of_the_fixture(gold, oracle, name):
    case, l64 = oracle(name)
    assert gold[name + "|losses"].shape == case["cand"].shape and gold[name + "|losses"].dtype == np.float32
    err = float(np.abs(gold[name + "|losses"].astype(np.float64) - l64).max())
    print(name, "max |reference float32 - oracle float64| = %.3e, delta_ref = %.3e" % (err, float(gold[name + "|delta_ref"][0])))
    assert err <= float(gold[name + "|delta_ref"][0]) + 1e-12      # the stored maximum itself, up to float64 rounding
    assert np.isfinite(l64).all()


@pytest.mark.parametrize("name", hints_cases.CASES)
def test_oracle_depth_equals_the_references_at_decisive_pixels(gold, oracle, name):
    case, l64 = oracle(name)
    dec = hints_ref.decisive(l64, case["depths"], float(gold["tol_loss"][0]))
    ours = hints_ref.gather(case["depths"], hints_ref.first_argmin(l64))
    theirs = hints_ref.gather(case["depths"], gold[name + "|index"].astype(np.int64))
    print(name, "decisive %.1f %%, depths equal at %.1f %% of all pixels" % (100 * dec.mean(), 100 * (ours == theirs).mean()))
    assert np.array_equal(ours[dec], theirs[dec])
    if name in hints_cases.SHARE_CASES:
        assert dec.mean() >= 0.85, dec.mean()


def test_the_reference_picks_the_first_of_the_duplicate_pair_and_zero_in_the_zero_block(gold):
    for name in hints_cases.CASES:
        case = hints_cases.build(name)
        index = gold[name + "|index"]
        if case["duplicate"]:
            assert np.array_equal(case["cand"][:, 0], case["cand"][:, 1])
            assert not (index == 1).any(), name
        if case["zero_block"]:
            y0, y1, x0, x1 = case["zero_block"]
            assert not case["depths"][:, :, y0:y1, x0:x1].any()
            assert not index[:, y0 + 1:y1 - 1, x0 + 1:x1 - 1].any(), name      # whole windows tie: the first index
            assert not hints_ref.gather(case["depths"], index.astype(np.int64))[:, y0:y1, x0:x1].any()


def test_cases_are_what_they_claim():
    assert len(hints_cases.SHARE_CASES) == len(hints_cases.CASES) - 1          # all but the 2 x 2 map
    for name, (B, M, H, W, as_disp) in hints_cases.CASES.items():
        case = hints_cases.build(name)
        assert case["cand"].shape == (B, M, H, W) and case["disparities"] == as_disp
        for k in ("base", "lookup"):
            assert case[k].shape == (B, 3, H, W) and case[k].min() >= 0.0 and case[k].max() <= 1.0
        assert case["base"].std() > 0.1                                           # texture, not a flat image
        assert np.allclose(case["K"][:, 0, 0], 0.58 * W) and np.allclose(case["K"][:, 1, 1], 1.92 * H)
        assert np.allclose(np.abs(case["T"][:, 0, 3]), 0.1) and np.array_equal(case["T"][:, :3, :3], np.tile(np.eye(3, dtype=np.float32), (B, 1, 1)))
        assert set(np.sign(case["T"][:, 0, 3]).tolist()) == ({-1.0, 1.0} if B > 1 else {-1.0})
        if H * W >= 256:
            missing = (case["depths"] == 0).mean()
            assert 0.1 < missing < 0.3, (name, missing)          # 15 % per map plus the zero block
        if as_disp:
            d = case["cand"]
            assert np.array_equal(d * 4, np.round(d * 4))                         # quarter pixels
            np.testing.assert_allclose(hints_ref.disparity_to_depth(d, case["fbl"]), case["depths"], rtol=3e-7)
