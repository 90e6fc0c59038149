"""CPU: tests/viz_ref.py -- the numpy statement of the colour-image rules -- reproduces every case of the fixture
tests/golden/viz_reference.npz, which np.percentile, matplotlib and the reference's own colorize / normalize_image wrote
(tests/golden/make_golden_viz.py), byte for byte; and the shipped colormap tables are matplotlib's."""
import hashlib
import os

import numpy as np
import pytest

import viz_cases
import viz_ref


@pytest.fixture(scope="module")
def golden(golden_dir):
    with np.load(os.path.join(golden_dir, "viz_reference.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def magma():
    return viz_ref.table("magma")


def test_fixture_holds_every_case_and_nothing_else(golden):
    want = set()
    for n in viz_cases.DISPARITY:
        want |= {"disparity|%s|rgb" % n, "disparity|%s|range" % n}
    want |= {"disparity|full|range", "disparity|full|sha256"} | {"disparity|%s|resized" % n for n in viz_cases.RESIZED}
    want |= {"colorize|" + n for n in viz_cases.COLORIZE} | {"normalize|" + n for n in viz_cases.NORMALIZE}
    assert set(golden) == want


@pytest.mark.parametrize("name", [n for n in viz_cases.DISPARITY if n not in viz_cases.RESIZED])
def test_disparity_cases(golden, magma, name):
    case = viz_cases.disparity(name)
    for b, x in enumerate(case["x"]):
        rgb, lo, hi = viz_ref.disparity_image(x, case["q"], magma)
        assert (lo, hi) == tuple(golden["disparity|%s|range" % name][b]), (name, b)
        assert np.array_equal(rgb, golden["disparity|%s|rgb" % name][b]), (name, b)


@pytest.mark.parametrize("name", viz_cases.RESIZED)
def test_resized_disparity_cases(golden, magma, name):
    """on the map the fixture keeps (ATen's resample on the CPU): byte for byte.  On viz_ref.bilinear's map, which equals it
    to rounding: the map within the stated error, the ranges within it, every pixel in the same table row or a neighbour
    (viz_ref.assert_resampled_close) -- the rule the GPU's own resample is held to"""
    case = viz_cases.disparity(name)
    for b, x in enumerate(case["x"]):
        kept = golden["disparity|%s|resized" % name][b]
        rgb, lo, hi = viz_ref.disparity_image(kept, case["q"], magma)
        assert (lo, hi) == tuple(golden["disparity|%s|range" % name][b]), (name, b)
        assert np.array_equal(rgb, golden["disparity|%s|rgb" % name][b]), (name, b)
        own = viz_ref.bilinear(x, *case["size"])
        assert np.abs(own.astype(np.float64) - kept).max() <= viz_ref.resample_tolerance(x, *x.shape)
        rgb, lo, hi = viz_ref.disparity_image(own, case["q"], magma)
        viz_ref.assert_resampled_close(rgb, (lo, hi), golden["disparity|%s|rgb" % name][b], golden["disparity|%s|range" % name][b], x, magma)


def test_full_size_case(golden, magma):
    """375 x 1242: (n - 1) * 0.95f is above 2^18, the weight a multiple of 1/32 -- an index taken in double misses vmax"""
    case = viz_cases.disparity("full")
    rgb, lo, hi = viz_ref.disparity_image(case["x"][0], case["q"], magma)
    assert (lo, hi) == tuple(golden["disparity|full|range"][0])
    assert hashlib.sha256(rgb[None].tobytes()).digest() == golden["disparity|full|sha256"].tobytes()
    n = case["x"][0].size
    k, g = viz_ref.percentile_index(n, 95)
    assert float(g) * 32 == int(float(g) * 32) and (n - 1) * 0.95 - k != float(g)
    s = np.sort(case["x"][0].ravel()).astype(np.float64)
    assert np.float32(s[k] + (s[k + 1] - s[k]) * ((n - 1) * 0.95 - k)) != hi


def test_percentile_branches():
    """the cases sit on both sides of g = 0.5 and on it"""
    g = {n: float(viz_ref.percentile_index(int(np.prod(viz_cases.DISPARITY[n][1][1:])), viz_cases.DISPARITY[n][3])[1])
         for n in ("two", "three", "three_q60", "ragged_7x13", "ragged_37x53")}
    assert g["two"] > 0.5 and g["three"] > 0.5 and g["three_q60"] < 0.5 and g["ragged_7x13"] == 0.5 and g["ragged_37x53"] == 0.0


def test_percentile_is_numpys():
    for name in ("heavy", "quant", "signed", "q99_5", "three_q60", "q100"):
        case = viz_cases.disparity(name)
        assert viz_ref.percentile(case["x"][0], case["q"]) == np.percentile(case["x"][0], case["q"]), name


@pytest.mark.parametrize("name", viz_cases.COLORIZE)
def test_colorize_cases(golden, name):
    case = viz_cases.colorize(name)
    plasma = viz_ref.table("plasma")
    got = np.stack([viz_ref.colorize(p, case["vmin"], case["vmax"], plasma).transpose(2, 0, 1) for p in case["x"]])
    assert np.array_equal(got, golden["colorize|" + name])


def test_colorize_cases_reach_both_ends_and_the_bad_colour(golden):
    plasma, out = viz_ref.table("plasma"), golden["colorize|fixed"]
    px = out.transpose(0, 2, 3, 1).reshape(-1, 3)
    assert (px == plasma[0]).all(1).sum() > 1 and (px == plasma[255]).all(1).sum() > 1
    assert (out[0, :, 3, 4] == 0).all()                                    # the NaN
    assert (golden["colorize|auto_constant"][0].transpose(1, 2, 0) == plasma[0]).all()
    with pytest.raises(ValueError):
        viz_ref.colorize(np.zeros((2, 2), np.float32), None, 1.0, plasma)


@pytest.mark.parametrize("name", viz_cases.NORMALIZE)
def test_normalize_cases(golden, name):
    case = viz_cases.normalize(name)
    got = viz_ref.normalize_image(case["x"], case["per_image"])
    assert np.array_equal(got.view(np.uint32), golden["normalize|" + name].view(np.uint32))


def test_shipped_tables():
    for name in ("magma", "plasma"):
        t = viz_ref.table(name)
        assert t.shape == (256, 3) and t.dtype == np.uint8
        assert len(np.unique(t, axis=0)) == 256                            # rows_of relies on it
    try:
        import matplotlib
    except ImportError:
        return
    for name in ("magma", "plasma"):
        assert np.array_equal(viz_ref.table(name), (matplotlib.colormaps[name](np.arange(256))[:, :3] * 255).astype(np.uint8))
