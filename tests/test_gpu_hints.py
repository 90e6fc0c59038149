"""GPU: the depth-hint fusion (csrc/wmd_hints.hip through depth_hints.fuse_depth_hints) against the float64 oracle
(tests/hints_ref.py) and the reference's own float32 run (tests/golden/hints_reference.npz).

tol_loss comes from the fixture: twice the largest |reference float32 loss - float64 oracle loss| over all cases -- the
kernel is another float32 evaluation of the same formula (another summation order, fused multiply-adds), which errs by the
reference's own amount and independently of it.  Selected depths are compared where the winner is decisive: the float64 gap
to the best candidate of another depth value exceeds 2 tol_loss (tests/test_hints_oracle.py asserts that this is at least
85 % of every case).  Reads the fixture only; every case runs the kernel once and the checks share the result."""
import numpy as np
import pytest
import torch

import hints_cases
import hints_ref
from util import load_golden
from wavelet_monodepth_amd import depth_hints as dh, photometric as ph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return load_golden("hints_reference.npz")


def on(case, dev):
    return {k: torch.from_numpy(case[k]).to(dev) for k in ("cand", "depths", "base", "lookup", "K", "inv_K", "T")}


def fuse(case, g, **kw):
    return dh.fuse_depth_hints(g["cand"], g["base"], g["lookup"], g["K"], g["inv_K"], g["T"], disparities=case["disparities"],
                               focal_times_baseline=case["fbl"], **kw)


@pytest.fixture(scope="module")
def results(dev):
    """name -> (case, device inputs, float64 oracle losses, (best_depth, best_index, losses) as numpy); computed once, read only"""
    memo = {}

    def get(name):
        if name not in memo:
            case = hints_cases.build(name)
            g = on(case, dev)
            out = tuple(t.cpu().numpy() for t in fuse(case, g, return_losses=True))
            memo[name] = (case, g, hints_ref.losses(case), out)
        return memo[name]
    return get


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


@pytest.mark.parametrize("name", hints_cases.CASES)
def test_losses_vs_float64_oracle(results, gold, name):
    case, _, l64, (best_depth, best_index, losses) = results(name)
    B, M, H, W = case["cand"].shape
    assert best_depth.shape == (B, 1, H, W) and best_depth.dtype == np.float32
    assert best_index.shape == (B, H, W) and best_index.dtype == np.int32
    assert losses.shape == (B, M, H, W) and losses.dtype == np.float32
    tol = float(gold["tol_loss"][0])
    err = float(np.abs(losses.astype(np.float64) - l64).max())
    print(name, "max |kernel - oracle64| = %.3e, tol_loss = %.3e, delta_ref = %.3e" % (err, tol, float(gold[name + "|delta_ref"][0])))
    assert np.isfinite(losses).all()
    assert err <= tol


@pytest.mark.parametrize("name", hints_cases.CASES)
def test_outputs_are_self_consistent_bit_for_bit(results, name):
    case, _, _, (best_depth, best_index, losses) = results(name)
    assert np.array_equal(best_index, hints_ref.first_argmin(losses))           # the first minimum of what was compared
    assert np.array_equal(bits(best_depth[:, 0]), bits(hints_ref.gather(case["depths"], best_index)))
    if case["duplicate"]:
        assert not (best_index == 1).any()
    if case["zero_block"]:
        y0, y1, x0, x1 = case["zero_block"]
        assert not best_depth[:, 0, y0:y1, x0:x1].any()
        assert not best_index[:, y0 + 1:y1 - 1, x0 + 1:x1 - 1].any()          # inside the rim whole windows tie: the first index


@pytest.mark.parametrize("name", hints_cases.CASES)
def test_selection_vs_the_reference(results, gold, name):
    case, _, l64, (best_depth, best_index, _) = results(name)
    tol = float(gold["tol_loss"][0])
    chosen = np.take_along_axis(l64, best_index[:, None].astype(np.int64), axis=1)[:, 0]
    excess = float((chosen - l64.min(1)).max())
    dec = hints_ref.decisive(l64, case["depths"], tol)
    theirs = hints_ref.gather(case["depths"], gold[name + "|index"].astype(np.int64))
    print(name, "largest float64 excess of the chosen candidate %.3e (2 tol_loss = %.3e); decisive %.1f %%; depth equals the "
          "reference's at %.2f %% of all pixels" % (excess, 2 * tol, 100 * dec.mean(), 100 * (best_depth[:, 0] == theirs).mean()))
    assert excess <= 2.0 * tol
    assert np.array_equal(bits(best_depth[:, 0][dec]), bits(theirs[dec]))


@pytest.mark.parametrize("name", ["b2_m5_33x70", "b2_m3_17x131", "b3_m1_2x2"])
def test_without_losses_and_twice_give_identical_bits(results, name):
    case, g, _, (best_depth, best_index, losses) = results(name)
    out = fuse(case, g)
    assert len(out) == 2
    assert np.array_equal(bits(out[0].cpu().numpy()), bits(best_depth)) and np.array_equal(out[1].cpu().numpy(), best_index)
    again = fuse(case, g, return_losses=True)
    for a, b in zip(again, (best_depth, best_index, losses)):
        assert np.array_equal(bits(a.cpu().numpy()), bits(b))


@pytest.mark.parametrize("name", ["b1_m12_13x21", "b2_m3_17x131"])
def test_disparity_input_equals_converted_depth_input(results, name):
    case, g, _, want = results(name)
    assert case["disparities"]
    depths = dh.disparity_to_depth(g["cand"], case["K"][0, 0, 0], 0.1)
    assert np.array_equal(bits(depths.cpu().numpy()), bits(case["depths"]))
    got = dh.fuse_depth_hints(depths, g["base"], g["lookup"], g["K"], g["inv_K"], g["T"], return_losses=True)
    for a, b in zip(got, want):
        assert np.array_equal(bits(a.cpu().numpy()), bits(b))


def test_depth_case_ignores_the_disparity_arguments(results):
    case, g, _, want = results("depths_b2_m4_24x40")
    assert not case["disparities"]
    got = dh.fuse_depth_hints(g["depths"], g["base"], g["lookup"], g["K"], g["inv_K"], g["T"], return_losses=True)
    for a, b in zip(got, want):
        assert np.array_equal(bits(a.cpu().numpy()), bits(b))


@pytest.mark.parametrize("name", ["b1_m12_13x21", "b1_m12_64x96"])
def test_single_image_form_equals_batch_of_one(results, name):
    case, g, _, (best_depth, best_index, losses) = results(name)
    d, i, l = dh.fuse_depth_hints(g["cand"][0], g["base"][0], g["lookup"][0], g["K"][0], g["inv_K"][0], g["T"][0],
                                  disparities=True, focal_times_baseline=case["fbl"], return_losses=True)
    H, W = best_index.shape[1:]
    assert d.shape == (1, H, W) and i.shape == (H, W) and l.shape == losses.shape[1:]
    assert np.array_equal(bits(d.cpu().numpy()), bits(best_depth[0])) and np.array_equal(i.cpu().numpy(), best_index[0])
    assert np.array_equal(bits(l.cpu().numpy()), bits(losses[0]))


@pytest.mark.parametrize("name", ["b2_m5_33x70", "b1_m12_64x96", "b3_m1_2x2"])
def test_composition_of_the_existing_operators(results, gold, name):
    """photometric.warp_frame on M-fold expanded inputs, then compute_reprojection_loss: what the fused launch replaces"""
    case, g, _, (_, _, losses) = results(name)
    B, M, H, W = case["cand"].shape
    tol = float(gold["tol_loss"][0])
    worst = 0.0
    for b in range(B):
        rep = lambda t: t[b:b + 1].expand(M, *t.shape[1:]).contiguous()
        warped = ph.warp_frame(rep(g["lookup"]), g["depths"][b][:, None].contiguous(), rep(g["K"]), rep(g["inv_K"]), rep(g["T"]))
        comp = ph.compute_reprojection_loss(warped, rep(g["base"]))[:, 0].cpu().numpy()
        worst = max(worst, float(np.abs(comp.astype(np.float64) - losses[b].astype(np.float64)).max()))
    print(name, "max |composition - fused| = %.3e, tol_loss = %.3e" % (worst, tol))
    assert worst <= tol


def test_no_ssim_is_the_l1_term_alone(results, gold):
    case, g, _, _ = results("b2_m5_33x70")
    _, index, losses = fuse(case, g, return_losses=True, no_ssim=True)
    l64 = hints_ref.losses(case, use_ssim=False)
    assert float(np.abs(losses.cpu().numpy() - l64).max()) <= float(gold["tol_loss"][0])
    assert np.array_equal(index.cpu().numpy(), hints_ref.first_argmin(losses.cpu().numpy()))


def test_hints_feed_the_trainer_loss(dev):
    """fuse_depth_hints -> depth_hint_inputs -> generate_images_pred / compute_losses(use_depth_hints=True)"""
    from util import loss_case
    from wavelet_monodepth_amd import synth
    inp, out = loss_case(hints=True)
    B, _, H, W = inp[("color", 0, 0)].shape
    M = 4
    cand = synth.uniform((B, M, H, W), "hint_cand", 3, 1.0, 40.0).astype(np.float32)
    cand[synth.uniform((B, M, H, W), "hint_miss", 3, 0.0, 1.0) < 0.3] = 0.0
    cand[:, :, 4:9, 5:12] = 0.0                                                 # a patch without any match
    i2 = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    o2 = {k: torch.from_numpy(v).to(dev) for k, v in out.items()}
    best_depth, _ = dh.fuse_depth_hints(torch.from_numpy(cand).to(dev), i2[("color", 0, 0)], i2[("color", "s", 0)], i2[("K", 0)],
                                        i2[("inv_K", 0)], i2["stereo_T"])
    hint = dh.depth_hint_inputs(best_depth)
    assert set(hint) == {"depth_hint", "depth_hint_mask"}
    assert torch.equal(hint["depth_hint_mask"], (best_depth > 0).float()) and not hint["depth_hint_mask"][:, :, 4:9, 5:12].any()
    i2.update(hint)
    opt = ph.LossOptions(height=H, width=W, frame_ids=[0, -1, 1, "s"], use_depth_hints=True)
    ph.generate_images_pred(i2, o2, opt)
    losses = ph.compute_losses(i2, o2, opt, tie_break_noise=0.0)
    assert torch.isfinite(losses["loss"]).all()
    picked = o2["depth_hint_pixels/0"]
    assert 0 < float(picked.sum()) < picked.numel()
    assert not picked[:, :, 4:9, 5:12].any()                                    # no hint there: the 1000 penalty keeps it out
