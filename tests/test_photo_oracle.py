"""CPU: the photometric oracle (oracle/photo_ref.py) against outputs and gradients of the reference's own KITTI/layers.py
(tests/golden/photo_reference.npz, made by tests/golden/make_golden_photo.py)."""
import numpy as np
import torch

from oracle import photo_ref as P
from wavelet_monodepth_amd import synth
from util import load_golden, photo_case


def t(a, g=False):
    return torch.from_numpy(a.copy()).requires_grad_(g)


def test_ssim_and_gradients():
    g = load_golden("photo_reference.npz")
    tgt, src, *_ = photo_case()
    x, y = t(src, True), t(tgt, True)
    s = P.ssim(x, y)
    w = torch.from_numpy(synth.uniform(tuple(s.shape), "ph_w", 31, 0.0, 1.0).astype(np.float32))
    (s * w).sum().backward()
    np.testing.assert_allclose(s.detach().numpy(), g["ssim"], atol=2e-6)
    np.testing.assert_allclose(x.grad.numpy(), g["ssim_dx"], rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(y.grad.numpy(), g["ssim_dy"], rtol=1e-4, atol=2e-5)


def test_warp_and_gradients():
    g = load_golden("photo_reference.npz")
    tgt, src, depth, K, inv_K, T = photo_case()
    d, Tt = t(depth, True), t(T, True)
    pix = P.project(P.backproject(d, t(inv_K)), t(K), Tt, *depth.shape[-2:])
    np.testing.assert_allclose(pix.detach().numpy(), g["pix_coords"], atol=2e-6)
    out = P.warp_frame(t(src), d, t(K), t(inv_K), Tt)
    w = torch.from_numpy(synth.uniform(tuple(out.shape), "ph_w", 31, 0.0, 1.0).astype(np.float32))
    (out * w).sum().backward()
    np.testing.assert_allclose(out.detach().numpy(), g["warp"], atol=2e-5)
    np.testing.assert_allclose(d.grad.numpy(), g["warp_ddepth"], rtol=1e-3, atol=2e-5)
    np.testing.assert_allclose(Tt.grad.numpy(), g["warp_dT"], rtol=1e-3, atol=1e-3)


def test_smooth_loss_and_gradient():
    g = load_golden("photo_reference.npz")
    tgt, src, depth, *_ = photo_case()
    disp = t((1.0 / depth).astype(np.float32), True)
    sm = P.get_smooth_loss(disp, t(tgt))
    sm.backward()
    np.testing.assert_allclose(float(sm), float(g["smooth"]), rtol=1e-6)
    np.testing.assert_allclose(disp.grad.numpy(), g["smooth_ddisp"], rtol=1e-5, atol=1e-8)


# ---- the edge cases of tests/test_gpu_photo_edges.py: what their builders promise, and the oracle against itself ----------

def test_edge_builders_meet_their_conditions():
    """checked here so that no GPU is needed to see that the inputs of the GPU tests are what those tests assume"""
    import util as U
    for c in U.WARP_CASES:
        k = U.warp_edge_case(*c, seed=5)
        assert np.isfinite(k["depth"]).all() and k["depth"].min() >= 2 and k["depth"].max() <= 30, c
        assert k["excl"].mean() <= 0.02, (c, k["excl"].mean())                  # near an integer or a clamp edge
        assert 0.05 <= k["clamped"] <= 0.5, (c, k["clamped"])                   # both branches of the border clamp carry weight
        assert not k["gout"][np.broadcast_to(k["excl"][:, None], k["gout"].shape)].any()
        assert (k["gout"][np.broadcast_to(~k["excl"][:, None], k["gout"].shape)] >= 0).all()
    for c in U.WARP_DEGENERATE:
        assert U.warp_edge_case(*c, seed=5)["clamped"] == 1.0, c                # every sample on the border
    for c in U.SMOOTH_CASES:
        disp, img = U.smooth_tie_case(*c, seed=5)
        assert np.isfinite(disp).all() and disp.min() > 0, c
        d = disp[:, 0]
        assert (d[:, :, :-1] == d[:, :, 1:]).any() or (d[:, :-1] == d[:, 1:]).any(), c      # exact ties
        assert (np.abs(d[:, :, :-1] - d[:, :, 1:]) == np.spacing(np.minimum(d[:, :, :-1], d[:, :, 1:]))).any(), c   # one ulp apart
        assert U.fully_tied(disp).any() or c[2:] == (2, 2), c
        assert np.unique(d).size > 1, c
    for c, smoothed in [(s, sm) for s in U.SSIM_SMALL for sm in (True, False)] + [(s, False) for s, _ in U.SSIM_WRAP]:
        k = U.ssim_edge_case(*c, seed=5, smoothed=smoothed)
        assert k["excl"].mean() <= 1e-3, c                                      # L1 ties
        s64 = U.oracle_ssim(k, "ssim", torch.float64)[0]
        assert s64.min() > 0 and s64.max() < 1, c                               # the clamp is inactive in float64


# The float32 oracle is the yardstick of the GPU tests (their bound is a multiple of its own error against float64), so its
# error has to be rounding and nothing else: 2^-24 per operation, times the size of the projective coordinates (fx X ~ 0.58 W
# x 30, so it grows with W: 4.5e-5 at 513x512) for the warp, times the cancellation of E[x^2] - mu^2 on smoothed frames for SSIM
# (2.6e-5).  A branch taken differently at a pixel that is not excluded would show as 1e-2 or more.
E_REF_MAX = 1e-4


def test_oracle_float32_agrees_with_float64_warp():
    import util as U
    for c in U.WARP_CASES + U.WARP_DEGENERATE:
        k = U.warp_edge_case(*c, seed=5)
        o64, o32 = U.oracle_warp(k, torch.float64), U.oracle_warp(k, torch.float32)
        assert all(v.dtype == np.float64 for v in o64)
        keep = ~k["excl"][:, None]
        errs = U.edge_err(o32[0], o64[0]), U.edge_err(o32[1], o64[1], keep), U.edge_err(o32[2], o64[2])
        assert max(errs) <= E_REF_MAX, (c, errs)


def test_oracle_float32_agrees_with_float64_ssim_and_smooth():
    import util as U
    for c, smoothed in [(s, sm) for s in U.SSIM_SMALL for sm in (True, False)]:
        k = U.ssim_edge_case(*c, seed=5, smoothed=smoothed)
        for mode in ("ssim", "reproj", "l1"):
            o64, o32 = U.oracle_ssim(k, mode, torch.float64), U.oracle_ssim(k, mode, torch.float32)
            errs = U.edge_err(o32[0], o64[0]), U.edge_err(o32[1], o64[1], ~k["excl"]), U.edge_err(o32[2], o64[2], ~k["excl"])
            assert max(errs) <= E_REF_MAX, (c, smoothed, mode, errs)
    for c in U.SMOOTH_CASES[:4]:
        disp, img = U.smooth_tie_case(*c, seed=5)
        o64, o32 = U.oracle_smooth(disp, img, torch.float64), U.oracle_smooth(disp, img, torch.float32)
        errs = U.edge_err(o32[0], o64[0]), U.edge_err(o32[1], o64[1])
        assert max(errs) <= 1e-6, (c, errs)                                     # no cancellation here: a few ulp
        tied = U.fully_tied(disp)
        assert not o64[1][tied].any() and not o32[1][tied].any()                # sgn(0) == 0


def test_oracle_runs_in_float64_and_normalises_by_scales():
    """the whole orchestration in float64 gives float64 losses and gradients; with loss_scales != scales the total is divided
    by len(scales) (the reference's num_scales, trainer.py:47,557)"""
    from types import SimpleNamespace
    from util import loss_case
    inp, out = loss_case()
    opt = SimpleNamespace(height=32, width=64, frame_ids=[0, -1, 1], loss_scales=[0, 2], scales=[0, 1, 2, 3], min_depth=0.1,
                          max_depth=100.0, v1_multiscale=False, avg_reprojection=False, no_ssim=False, use_depth_hints=False,
                          disparity_smoothness=1e-3)
    i2 = {k: torch.from_numpy(v).double() for k, v in inp.items()}
    o2 = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in out.items()}
    P.generate_images_pred(i2, o2, opt)
    losses = P.compute_losses(i2, o2, opt)
    losses["loss"].backward()
    assert all(v.dtype == torch.float64 for v in losses.values())
    assert o2[("disp", 0)].grad.dtype == torch.float64 and o2[("cam_T_cam", 0, 1)].grad.dtype == torch.float64
    assert o2[("color", -1, 2)].dtype == torch.float64 and o2["identity_selection/0"].dtype == torch.float64
    assert abs(float(losses["loss"].detach()) * 4 - float((losses["loss/0"] + losses["loss/2"]).detach())) < 1e-12
