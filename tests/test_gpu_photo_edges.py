"""GPU: the photometric kernels (csrc/wmd_photo.hip) against the float64 oracle at the smallest shapes that reach each launch
edge: the cross-block reduces of the warp and smoothness backward/forward (one block, two, one partial per lane, the
lane-strided finish, the block cap), a source frame of another size than the target, the wrap of the SSIM grid-stride loops,
2-pixel-wide reflection windows, exact ties, and the option paths of the loss orchestration.

Tolerances are measured, not chosen: for every compared tensor, on the same inputs,
    e_ref = max |oracle32 - oracle64| / max |oracle64|     the torch-CPU oracle in float32 against itself in float64
    e_hip = max |hip      - oracle64| / max |oracle64|
over the pixels that are not excluded, and the assertion is e_hip <= F[kind] * e_ref + 4 * 2^-23.  Excluded are the points
where the operation itself is discontinuous (util.warp_edge_case, util.ssim_edge_case), where a rounding that flips a branch
is no kernel error; the upstream gradient is zero there, so sums over pixels do not depend on the branch either."""
import numpy as np
import pytest
import torch

from oracle import photo_ref as P
from wavelet_monodepth_amd import photometric as ph
import util as U

pytestmark = pytest.mark.gpu

FLOOR = 4 * 2.0 ** -23
# per tensor kind, the smallest power of two >= twice the largest e_hip / e_ref measured on the MI355X among the comparisons whose
# e_hip exceeds the floor (below it the bound holds whatever F is, and the ratio of two roundings of a few ulp says nothing);
# the table is in DESIGN.md §4.6.  loss_ddisp / loss_dT: the gradients of the total loss w.r.t. the disparities / the poses.
F = {"ssim_out": 4, "ssim_grad": 4, "warp_out": 4, "ddepth": 4, "dT": 8, "smooth": 2, "ddisp": 4,
     "loss": 64, "loss_ddisp": 4, "loss_dT": 4}
assert max(F.values()) <= 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def t(a, dev, g=False):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev).requires_grad_(g)


def n64(v):
    return v.detach().cpu().double().numpy()


class Checks:
    """Prints e_ref, e_hip and their ratio for every compared tensor, then asserts all of them at once (so that one run
    shows every figure)."""

    def __init__(self, case):
        self.case, self.bad = case, []

    def add(self, kind, what, hip, o32, o64, keep=None, scalar=False):
        if scalar:
            hip, o32, o64 = (float(v.detach()) if torch.is_tensor(v) else float(v) for v in (hip, o32, o64))
            e_ref, e_hip = abs(o32 - o64) / abs(o64), abs(hip - o64) / abs(o64)
        else:
            assert hip.shape == o64.shape, (what, hip.shape, o64.shape)
            e_ref, e_hip = U.edge_err(o32, o64, keep), U.edge_err(hip, o64, keep)
        bound = F[kind] * e_ref + FLOOR
        print("EDGE %-10s %-28s %-22s e_ref %.3e e_hip %.3e ratio %s need_F %.2f" % (
            kind, self.case, what, e_ref, e_hip, "%.2f" % (e_hip / e_ref) if e_ref > 0 else "-",
            max(e_hip - FLOOR, 0.0) / e_ref if e_ref > 0 else (0.0 if e_hip <= FLOOR else float("inf"))))
        if not e_hip <= bound:
            self.bad.append("%s %s: e_hip %.3e > %d * e_ref %.3e + %.1e" % (kind, what, e_hip, F[kind], e_ref, FLOOR))

    def done(self):
        assert not self.bad, "%s: %s" % (self.case, "; ".join(self.bad))


# ---- SSIM / reprojection loss ---------------------------------------------------------------------------------------------

def hip_ssim(case, mode, dev):
    x, y = t(case["x"], dev, True), t(case["y"], dev, True)
    out = ph.SSIM()(x, y) if mode == "ssim" else ph.compute_reprojection_loss(x, y, mode == "reproj")
    (out * t(case["w" if mode == "ssim" else "w1"], dev)).sum().backward()
    return n64(out), n64(x.grad), n64(y.grad)


def check_ssim(shape, smoothed, mode, dev):
    case = U.ssim_edge_case(*shape, seed=5, smoothed=smoothed)
    assert case["excl"].mean() <= 1e-3                                    # L1 ties
    o64, o32 = U.oracle_ssim(case, mode, torch.float64), U.oracle_ssim(case, mode, torch.float32)
    s64 = o64[0] if mode == "ssim" else U.oracle_ssim(case, "ssim", torch.float64)[0]
    assert s64.min() > 0 and s64.max() < 1                                # the clamp is inactive in the float64 reference
    hip = hip_ssim(case, mode, dev)
    c = Checks("%s %s %s" % ("x".join(map(str, shape)), "smoothed" if smoothed else "iid", mode))
    c.add("ssim_out", "out", hip[0], o32[0], o64[0])
    c.add("ssim_grad", "dx", hip[1], o32[1], o64[1], ~case["excl"])
    c.add("ssim_grad", "dy", hip[2], o32[2], o64[2], ~case["excl"])
    c.done()


@pytest.mark.parametrize("mode", ["ssim", "reproj", "l1"])
@pytest.mark.parametrize("smoothed", [True, False], ids=["smoothed", "iid"])
@pytest.mark.parametrize("shape", U.SSIM_SMALL, ids=lambda s: "x".join(map(str, s)))
def test_ssim_small_shapes(dev, shape, smoothed, mode):
    """C == 1, and H == 2 or W == 2, where both reflected taps of a window fall on the same row and the gather multiplicity
    reaches 2 x 2; odd sizes; more than one plane."""
    check_ssim(shape, smoothed, mode, dev)


@pytest.mark.parametrize("shape,mode", U.SSIM_WRAP, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_ssim_grid_wrap(dev, shape, mode):
    """more elements than the 8192 x 256 grid: 1x3x700x1000 wraps the mode-0 forward (indexed by B C H W) and both backward
    kernels, 1x1x1025x2050 the mode-1 forward (indexed by B H W)"""
    assert int(np.prod(shape)) > 8192 * 256
    check_ssim(shape, False, mode, dev)


# ---- warp -----------------------------------------------------------------------------------------------------------------

def hip_warp(case, dev):
    d, T = t(case["depth"], dev, True), t(case["T"], dev, True)
    out = ph.warp_frame(t(case["src"], dev), d, t(case["K"], dev), t(case["inv_K"], dev), T)
    (out * t(case["gout"], dev)).sum().backward()
    return n64(out), n64(d.grad), n64(T.grad)


@pytest.mark.parametrize("shape", U.WARP_CASES, ids=lambda s: "x".join(map(str, s)))
def test_warp_edges(dev, shape):
    """forward at every pixel, ddepth at the pixels that are not excluded, dT (a sum over all pixels, with the upstream
    gradient zero at the excluded ones)"""
    case = U.warp_edge_case(*shape, seed=5)
    assert np.isfinite(case["depth"]).all() and case["depth"].min() >= 2 and case["depth"].max() <= 30
    assert case["excl"].mean() <= 0.02 and 0.05 <= case["clamped"] <= 0.5, (case["excl"].mean(), case["clamped"])
    o64, o32 = U.oracle_warp(case, torch.float64), U.oracle_warp(case, torch.float32)
    hip = hip_warp(case, dev)
    keep = ~case["excl"][:, None]
    c = Checks("x".join(map(str, shape)))
    c.add("warp_out", "out", hip[0], o32[0], o64[0])
    c.add("ddepth", "ddepth", hip[1], o32[1], o64[1], keep)
    c.add("dT", "dT", hip[2], o32[2], o64[2])
    c.done()


@pytest.mark.parametrize("shape", U.WARP_DEGENERATE, ids=lambda s: "x".join(map(str, s)))
def test_warp_all_samples_on_the_border(dev, shape):
    """2x2 -> 2x2: the reference's / (W - 1) with align_corners=False puts x = 0 at -0.5 and x = 1 at 1.5 source pixels; a
    1x1 source: the clamp range is empty.  Either way every sample is clamped: the output is the border pixel itself and
    both gradients are exactly zero, in the oracle as in the kernel."""
    B, C, H, W, Hs, Ws = shape
    case = U.warp_edge_case(*shape, seed=5)
    ux, uy = case["ux"], case["uy"]
    assert (((ux <= 0) | (ux >= Ws - 1)) & ((uy <= 0) | (uy >= Hs - 1))).all() and case["clamped"] == 1.0
    case["gout"] = np.abs(case["gout"]) + (case["gout"] == 0)             # no pixel needs excluding here
    ix, iy = np.where(ux <= 0, 0, Ws - 1), np.where(uy <= 0, 0, Hs - 1)
    want = case["src"][np.arange(B)[:, None, None, None], np.arange(C)[None, :, None, None], iy[:, None], ix[:, None]]
    for out, dd, dT in (U.oracle_warp(case, torch.float64), U.oracle_warp(case, torch.float32), hip_warp(case, dev)):
        assert np.array_equal(out, want.astype(np.float64))
        assert not dd.any() and not dT.any()
    if Hs == 1:
        assert (want == case["src"].reshape(B, C, 1, 1)).all()             # constant per channel


# ---- smoothness -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", U.SMOOTH_CASES, ids=lambda s: "x".join(map(str, s)))
def test_smooth_edges(dev, shape):
    """value and ddisp with exact ties and one-ulp neighbours, at one block, two, the lane-strided finish (65 partials) and
    the 512-block cap (the grid-stride loop runs a second time)"""
    disp, img = U.smooth_tie_case(*shape, seed=5)
    assert np.isfinite(disp).all()
    o64, o32 = U.oracle_smooth(disp, img, torch.float64), U.oracle_smooth(disp, img, torch.float32)
    d = t(disp, dev, True)
    sm = ph.get_smooth_loss(d, t(img, dev))
    (sm * U.SMOOTH_UPSTREAM).backward()
    hip = n64(sm), n64(d.grad)
    c = Checks("x".join(map(str, shape)))
    c.add("smooth", "value", hip[0], o32[0], o64[0], scalar=True)
    c.add("ddisp", "ddisp", hip[1], o32[1], o64[1])
    c.done()
    tied = U.fully_tied(disp)
    assert tied.any() or shape[2:] == (2, 2)
    for g in (o64[1], o32[1], hip[1]):                                    # sgn(0) == 0 from either side: bit for bit
        assert not g[tied].any()


# ---- the loss orchestration -------------------------------------------------------------------------------------------------

ORCH = {"avg_reprojection": dict(avg_reprojection=True), "no_ssim": dict(no_ssim=True), "v1_multiscale": dict(v1_multiscale=True),
        "loss_scales": dict(loss_scales=[0, 2], scales=[0, 1, 2, 3])}


@pytest.mark.parametrize("name", list(ORCH))
def test_trainer_loss_options_vs_oracle(dev, name):
    """generate_images_pred + compute_losses on loss_case() at 32x64 for the options the default run never takes; with
    loss_scales != scales the total is normalised by len(scales) (trainer.py:47,557)."""
    inp, out = U.loss_case()
    for s in range(1, 4):                                                 # v1_multiscale warps at the scale's own size
        inp[("K", s)], inp[("inv_K", s)] = U.scaled_intrinsics(2, 32 >> s, 64 >> s)
    opt = ph.LossOptions(height=32, width=64, **ORCH[name])
    grad_keys = [("disp", s) for s in opt.loss_scales] + [("cam_T_cam", 0, -1), ("cam_T_cam", 0, 1)]

    def run(device, dtype, mod):
        i2 = {k: torch.from_numpy(v).to(device, dtype) for k, v in inp.items()}
        o2 = {k: torch.from_numpy(v).to(device, dtype).requires_grad_(k in grad_keys) for k, v in out.items()}
        mod.generate_images_pred(i2, o2, opt)
        losses = mod.compute_losses(i2, o2, opt, tie_break_noise=0.0) if mod is ph else mod.compute_losses(i2, o2, opt)
        losses["loss"].backward()
        return losses, o2

    l64, o64 = run("cpu", torch.float64, P)
    l32, o32 = run("cpu", torch.float32, P)
    lg, og = run(dev, torch.float32, ph)
    assert set(lg) == set(l64)
    if name == "loss_scales":
        assert abs(float(l64["loss"].detach()) * 4 - float((l64["loss/0"] + l64["loss/2"]).detach())) < 1e-12
    c = Checks(name)
    for k in l64:
        c.add("loss", k, lg[k], l32[k], l64[k], scalar=True)
    for s in opt.loss_scales:
        a, b = og["identity_selection/%d" % s].cpu().double(), o64["identity_selection/%d" % s]
        assert float((a != b).double().mean()) < 2e-3                    # ties within rounding may fall either way
    for k in grad_keys:
        c.add("loss_ddisp" if k[0] == "disp" else "loss_dT", "d" + U.key_str(k), n64(og[k].grad), n64(o32[k].grad), n64(o64[k].grad))
    c.done()
