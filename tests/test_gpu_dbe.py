"""GPU: the depth-boundary errors (csrc/wmd_dbe.hip through evaluation.compute_depth_boundary_error / canny) against
tests/golden/dbe_reference.npz: the reference's own compute_depth_boundary_error around this project's definition of the
detector.  Edge maps bit for bit (every decision of every case is at least 1e-6 wide, tests/test_dbe_oracle.py), scores to
the float32 rounding of the output.  Reads the fixture only."""
import numpy as np
import pytest
import torch

import dbe_cases
from util import load_golden
from wavelet_monodepth_amd import evaluation as ev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return load_golden("dbe_reference.npz")


def unpack(gold, name, shape):
    return np.unpackbits(gold[name + "|edges"])[:int(np.prod(shape))].reshape(shape).astype(bool)


def run(case, dev):
    g = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    scores, edges = ev.compute_depth_boundary_error(g(case["edges_gt"]), g(case["pred"]), g(case["mask"]), dbe_cases.LOW, dbe_cases.HIGH)
    assert scores.dtype == torch.float32 and edges.dtype == torch.bool
    return scores.cpu().numpy(), edges.cpu().numpy()


def check(name, scores, edges, gold):
    want = unpack(gold, name, edges.shape)
    print(name, "scores", scores.tolist(), "reference", gold[name + "|scores"].tolist(), "edge pixels", edges.sum((1, 2)).tolist(),
          "differing", int((edges != want).sum()))
    assert np.array_equal(edges, want), "%s: %d edge pixels differ" % (name, int((edges != want).sum()))
    np.testing.assert_allclose(scores, gold[name + "|scores"], rtol=1e-6, atol=0, equal_nan=True)


@pytest.mark.parametrize("name", dbe_cases.CASES)
def test_dbe_vs_reference_fixture(dev, gold, name):
    """scenes at four ragged sizes and B = 1..3; the mixed batch (ordinary, constant prediction -> (10, 10), no ground-truth
    edges -> (nan, nan) and an empty map); a zero hole; a half-image mask; the hysteresis reach image; B = 2 at 440 x 592"""
    check(name, *run(dbe_cases.build(name), dev), gold)


def test_special_scores_are_exact(dev):
    scores, edges = run(dbe_cases.build("mixed"), dev)
    assert scores[1].tolist() == [10.0, 10.0] and np.isnan(scores[2]).all()
    assert edges[0].any() and not edges[1].any() and not edges[2].any()


def test_reach_keeps_the_long_weak_edge_and_drops_the_other(dev):
    _, edges = run(dbe_cases.build("reach"), dev)
    r1, r2, W = dbe_cases.REACH["kept_row"], dbe_cases.REACH["dropped_row"], dbe_cases.REACH["W"]
    assert edges[0, r1, 1:W - 1].all()
    assert not edges[0, r2 - 3:r2 + 4].any()


def test_edge_map_input_kinds_agree(dev):
    """edges_gt as bool, uint8 and float (any nonzero value) give the same result"""
    case = dbe_cases.build("scene_37x53b2")
    pred = torch.from_numpy(case["pred"]).to(dev)
    gt = torch.from_numpy(case["edges_gt"]).to(dev)
    a = ev.compute_depth_boundary_error(gt, pred)
    for other in (gt.bool(), gt.float() * 0.25):
        b = ev.compute_depth_boundary_error(other, pred)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("name,H,W,sigma,low,high", dbe_cases.CANNY_CASES)
def test_canny_vs_fixture(dev, gold, name, H, W, sigma, low, high):
    img = torch.from_numpy(dbe_cases.canny_image(name, H, W)).to(dev)
    edges = ev.canny(img[None], sigma, low, high)
    assert edges.shape == (1, H, W) and edges.dtype == torch.bool
    want = unpack(gold, name, (H, W))
    assert np.array_equal(edges[0].cpu().numpy(), want), int((edges[0].cpu().numpy() != want).sum())
    assert torch.equal(ev.canny(img, sigma, low, high), edges[0])          # [H,W] in, [H,W] out


@pytest.mark.parametrize("name", ["scene_48x64b3", "full"])
def test_two_calls_give_identical_bits(dev, name):
    case = dbe_cases.build(name)
    s1, e1 = run(case, dev)
    s2, e2 = run(case, dev)
    assert np.array_equal(s1.view(np.uint32), s2.view(np.uint32)) and np.array_equal(e1, e2)
