"""CPU: the float64 numpy oracle of the LiDAR depth maps (tests/lidar_ref.py) against the reference's own
generate_depth_map (tests/golden/lidar_reference.npz, written by tests/golden/make_golden_lidar.py), and the conditions that
keep the cases honest: an exact case must tell the reference's bucket rule from the two simpler readings of it, round a tie
and land a negative p_2 in the image.  The module is imported so that these tests belong to the feature they pin."""
import numpy as np
import pytest

import lidar_cases
import lidar_ref
from util import load_golden
from wavelet_monodepth_amd import kitti_utils  # noqa: F401

MODES = (("cam", False), ("vel", True))


@pytest.fixture(scope="module")
def gold():
    return load_golden("lidar_reference.npz")


def dense(gold, name, mode, shape):
    if name != lidar_cases.FULL:
        return gold["%s|%s" % (name, mode)]
    flat = np.zeros(shape[0] * shape[1], np.float32)
    flat[gold["%s|%s|index" % (name, mode)]] = gold["%s|%s|value" % (name, mode)]
    return flat.reshape(shape)


@pytest.mark.parametrize("name", lidar_cases.EXACT_CLASS)
def test_oracle_equals_the_reference_in_float64(gold, name):
    case = lidar_cases.build(name)
    for mode, vel in MODES:
        ours = lidar_ref.depth_map(case["points"], case["P"], case["shape"], vel)
        ref = gold["%s|%s" % (name, mode)]
        assert ref.dtype == np.float64 and ref.shape == case["shape"]
        assert np.array_equal(ours, ref), (name, mode, int((ours != ref).sum()))


@pytest.mark.parametrize("name", lidar_cases.GENERAL_CLASS + (lidar_cases.FULL,))
def test_oracle_against_the_reference_on_general_calibrations(gold, name):
    """vel_depth=True: the identical map (x is a float32 number, no arithmetic touches it).  Camera mode: the identical
    non-zero support; the values may differ in the last float64 bits, where the reference's BLAS sums in another order."""
    case = lidar_cases.build(name)
    ours = {mode: lidar_ref.depth_map(case["points"], case["P"], case["shape"], vel) for mode, vel in MODES}
    ref = {mode: dense(gold, name, mode, case["shape"]) for mode, _ in MODES}
    assert np.array_equal(ours["vel"], ref["vel"].astype(np.float64))
    assert np.array_equal(ours["cam"] != 0, ref["cam"] != 0)
    close = np.abs(ours["cam"] - ref["cam"]) <= np.abs(ref["cam"]) * 2.0 ** -23    # float32 storage of the full-size case included
    assert close.all()


@pytest.mark.parametrize("name", list(lidar_cases.EXACT))
def test_exact_cases_cover_the_rules(name):
    case = lidar_cases.build(name)
    cov = lidar_ref.coverage(case["points"], case["P"], case["shape"])
    print(name, cov)
    assert cov["ties"] >= 1 and cov["negative_p2"] >= 1 and cov["zero_p2"] >= 1
    assert cov["duplicate_pixels"] >= 1 and cov["joined_buckets"] >= 1
    for _, vel in MODES:
        full = lidar_ref.depth_map(case["points"], case["P"], case["shape"], vel)
        for rule in ("pixel_min", "last_wins"):
            other = lidar_ref.depth_map(case["points"], case["P"], case["shape"], vel, rule=rule)
            assert (other != full).any(), "%s does not tell the bucket rule from %s" % (name, rule)


def test_special_case_holds_what_it_says():
    pts = lidar_cases.build(lidar_cases.SPECIAL)["points"][:, :3]
    for col in range(3):
        assert np.isnan(pts[:, col]).any() and (pts[:, col] == np.inf).any() and (pts[:, col] == -np.inf).any()
        assert ((pts[:, col] == 0) & np.signbit(pts[:, col])).any()


def test_ragged_batch_sizes():
    assert [len(lidar_cases.build(n)["points"]) for n in lidar_cases.RAGGED] == [0, 1, 255, 256, 1025]
    Ps = [lidar_cases.build(n)["P"] for n in lidar_cases.RAGGED]
    assert all(not np.array_equal(Ps[i], Ps[j]) for i in range(5) for j in range(i))
