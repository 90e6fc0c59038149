"""CPU: the numpy oracle of the KITTI training inputs (tests/inputs_ref.py) against the fixture that the reference's own
MonoDataset.preprocess wrote over Pillow (tests/golden/make_golden_inputs.py): every level and every jittered level bit for
bit, and the hue op over all 2^24 colours by SHA-256.  scaled_intrinsics and stereo_T against the reference's numpy lines
(KITTI/datasets/mono_dataset.py:202-211, :228-234), restated here."""
import hashlib
import os

import numpy as np
import pytest

import inputs_cases
import inputs_ref as R
from wavelet_monodepth_amd import kitti_inputs as ki

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputs_reference.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_fixture_names_its_pillow(golden):
    assert str(golden["pillow"]).startswith("12.2")
    for shift in inputs_cases.CUBE_SHIFTS:
        assert len(str(golden["cube|%d" % shift])) == 64


@pytest.mark.parametrize("name", inputs_cases.CASES)
def test_oracle_equals_the_reference_chain(golden, name):
    case = inputs_cases.build(name)
    j = case["jitter"]
    for i in range(len(case["frames"])):
        levels = R.pyramid(case["frames"][i], case["height"], case["width"], case["num_scales"], bool(case["flip"][i]))
        for s, level in enumerate(levels):
            assert level.dtype == np.uint8 and np.array_equal(level, golden["%s|color|%d" % (name, s)][i]), (i, s)
            aug = R.jitter(level, j["order"][i], j["factors"][i], j["hue_shift"][i]) if j is not None and j["enable"][i] else level
            assert np.array_equal(aug, golden["%s|aug|%d" % (name, s)][i]), (i, s)


def test_cases_cover_what_they_claim(golden):
    sat = inputs_cases.build("saturate_48x64")["frames"]
    assert set(np.unique(sat).tolist()) == {0, 255}
    bounds, coeffs = R.lanczos_table(64, 8)
    below = above = 0
    for xx, (xmin, n) in enumerate(bounds):                                          # the horizontal pass before clip8
        acc = (np.tensordot(sat[:, :, xmin:xmin + n].astype(np.int64), coeffs[xx, :n].astype(np.int64), axes=([2], [0])) + (1 << 21)) >> 22
        below, above = below + int((acc < 0).sum()), above + int((acc > 255).sum())
    assert below > 100 and above > 100                                               # clip8 on both sides
    case = inputs_cases.build("same_12x20")
    assert np.array_equal(golden["same_12x20|color|0"], case["frames"])             # the identity
    b, _ = R.lanczos_table(7, 3)
    assert (b[:, 0] == 0).all() and (b[:, 0] + b[:, 1] == 7).all()                  # both borders clipped at once
    orders = inputs_cases.build("orders_random")
    assert sorted(map(tuple, orders["jitter"]["order"][orders["jitter"]["enable"] == 1][:24].tolist())) == sorted(map(tuple, inputs_cases.PERMS))
    assert orders["jitter"]["enable"][5] == 0 and np.array_equal(golden["orders_random|aug|0"][5], orders["frames"][5])
    half = orders["frames"][25]
    assert 2 * int(R.grey(half).astype(np.int64).sum()) == 21 * half.shape[0] * half.shape[1] and R.grey_mean(half) == 11
    # contrast 0.8 about 11 keeps this image (10.2 -> 10, 11 -> 11); about a mean rounded down to 10 the 11s would fall to 10
    assert np.array_equal(golden["orders_random|aug|0"][25], half)
    assert not np.array_equal(R.blend(np.full_like(half, 10), half, 0.8), half)
    edges = inputs_cases.build("orders_edges")["jitter"]
    assert set(np.unique(edges["factors"]).tolist()) == {np.float32(0.8).item(), 1.0, np.float32(1.2).item()}
    assert set(edges["hue_shift"].tolist()) == {0, 25, 231}


@pytest.fixture(scope="module")
def cube():
    return R.colour_cube()


@pytest.mark.parametrize("shift", inputs_cases.CUBE_SHIFTS)
def test_hue_over_the_full_colour_cube(golden, cube, shift):
    assert hashlib.sha256(R.hue(cube, shift).tobytes()).hexdigest() == str(golden["cube|%d" % shift])


def test_to_tensor_is_a_float32_division():
    u8 = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)
    t = R.to_tensor(u8)
    assert t.dtype == np.float32 and t.shape == (3, 16, 16)
    exact = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)           # one rounding of the exact quotient
    assert np.array_equal(t[0].ravel(), exact)
    assert (t[0].ravel() != (np.arange(256, dtype=np.float32) * np.float32(1.0 / 255.0))).any()   # a reciprocal multiply is not it


def test_hue_shift_truncates_toward_zero():
    assert [R.hue_shift_of(h) for h in (0.1, -0.1, 0.05, -0.004, 0.0)] == [25, 231, 12, 255, 0]
    p = ki.sample_color_jitter(64, p=0.5)
    assert len(p) == 64 and p.order.shape == (64, 4) and p.factors.dtype.is_floating_point
    assert (np.sort(p.order.numpy(), axis=1) == np.arange(4)).all()
    assert 0 < int(p.enable.sum()) < 64
    assert float(p.factors.min()) >= 0.8 and float(p.factors.max()) <= 1.2
    s = p.hue_shift.numpy()
    assert ((s <= 25) | (s >= 231)).all()


def test_scaled_intrinsics_and_stereo_T_follow_the_reference_lines():
    K = np.array([[0.58, 0, 0.5, 0], [0, 1.92, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)   # kitti_dataset.py:36-39
    height, width = 192, 640
    got = ki.scaled_intrinsics(K, height, width, range(4))
    for scale in range(4):
        Ks = K.copy()
        Ks[0, :] *= width // (2 ** scale)
        Ks[1, :] *= height // (2 ** scale)
        inv_K = np.linalg.pinv(Ks)
        assert got[("K", scale)].numpy().dtype == np.float32 and np.array_equal(got[("K", scale)].numpy(), Ks)
        assert got[("inv_K", scale)].numpy().dtype == np.float32 and np.array_equal(got[("inv_K", scale)].numpy(), inv_K)
    assert np.array_equal(K, np.array([[0.58, 0, 0.5, 0], [0, 1.92, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32))   # untouched
    for side in ("l", "r"):
        for do_flip in (False, True):
            T = np.eye(4, dtype=np.float32)
            T[0, 3] = (-1 if side == "l" else 1) * (-1 if do_flip else 1) * 0.1
            assert np.array_equal(ki.stereo_T(side, do_flip).numpy(), T)
    assert ki.stereo_T("l", False)[0, 3] == np.float32(-0.1)
