"""GPU: no data, loss or evaluation kernel stores past the workspace size its query answers, and none reads the workspace before
writing it.

Every operator below allocates through _lib.byte_workspace / _lib.float_workspace.  Here both are replaced by versions that hand out
bytes [G, G + n) of a larger buffer -- exactly the size asked, G = 4096 bytes of guard on either side -- filled once with 0x00 and
once with 0xFF.  The two runs must give the same bits, the same bits as a run on the ordinary allocations, and leave both guard bands
as they were filled.  A self-comparison: what the operators compute is pinned against their oracles by their own tests.  The shapes
are the smallest that reach every region of each layout (csrc/wmd_ws_layouts.h)."""
import numpy as np
import pytest
import torch

import dbe_cases
import inputs_cases
import lidar_cases
import stereo_cases
import viz_cases
from util import photo_case
from wavelet_monodepth_amd import _lib, evaluation as ev, kitti_inputs as ki, kitti_utils as ku, photometric as ph, stereo, synth, visualize as viz

pytestmark = pytest.mark.gpu
G = 4096


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


class Guarded:
    """the two allocators over guarded buffers of one fill; G keeps the 256-byte alignment of a fresh allocation"""

    def __init__(self, fill):
        self.fill, self.handed = fill, []

    def _bytes(self, n, device):
        buf = torch.full((2 * G + n,), self.fill, dtype=torch.uint8, device=device)
        self.handed.append((buf, n))
        return buf[G:G + n]

    def byte_workspace(self, nbytes, device):
        return self._bytes(nbytes, device), nbytes

    def float_workspace(self, nfloats, device):
        return self._bytes(4 * nfloats, device).view(torch.float32) if nfloats else None

    def guards_hold(self):
        return all(bool((buf[:G] == self.fill).all()) and bool((buf[G + n:] == self.fill).all()) for buf, n in self.handed)


def u(tag, shape, lo, hi):
    return synth.uniform(shape, "ws_" + tag, 3, lo, hi).astype(np.float32)


def g(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def kitti(B, h, w, H, W, median):
    def run(dev):
        gt = u("gt", (B, H, W), 0.0, 95.0)
        gt[u("hole", (B, H, W), 0.0, 1.0) < 0.7] = 0
        return ev.kitti_metrics(g(u("disp", (B, h, w), 0.01, 0.3), dev), g(gt, dev), disable_median_scaling=not median)
    return run


def edges(B, H, W):
    def run(dev):
        pred, gt = dbe_cases.scenes(B, H, W, "ws", 5)
        return (ev.canny(g(pred / pred.max(), dev), 1.0, 0.02, 0.05),) + ev.compute_depth_boundary_error(g(gt, dev), g(pred, dev))
    return run


def images(dev):
    x = viz_cases.dist("heavy", (2, 6, 20), "ws")
    y = viz_cases.dist("signed", (2, 11, 37), "ws")
    return (viz.disparity_image(g(x, dev), (11, 37), return_range=True) + viz.disparity_image(g(y, dev), (11, 37), return_range=True) +
            (viz.normalize_image(g(y, dev), per_image=True), viz.normalize_image(g(y, dev)), viz.colorize(g(y, dev), None, None)))


def lidar(name, cuts):
    def run(dev):
        case = lidar_cases.build(name)
        B = len(cuts) - 1
        return ku.project_lidar(g(case["points"], dev), g(np.stack([case["P"]] * B), dev), case["shape"], False, torch.tensor(cuts, device=dev))
    return run


def inputs(dev):
    case = inputs_cases.build("clip_5x7")
    n = case["frames"].shape[0]
    j = inputs_cases.random_jitter("ws", n, 2)
    jit = ki.ColorJitterParams(j["enable"], j["order"], j["factors"], j["hue_shift"]).to(dev)
    frames = g(case["frames"], dev)
    levels = ki.color_pyramid(frames, case["height"], case["width"], case["num_scales"], g(case["flip"], dev), jit)
    return tuple(t for level in levels for t in level) + (ki.color_jitter(frames, jit),)


def sgbm(C):
    def run(dev):
        pairs = [stereo_cases.pair(12, 48, C, 16, 0, seed) for seed in range(3)]
        s = stereo.SGBMSettings(numDisparities=16, blockSize=3, P1=36, P2=288, preFilterCap=63, uniquenessRatio=10, speckleWindowSize=100, speckleRange=16)
        return stereo.sgbm(g(np.stack([l for l, _ in pairs]), dev), g(np.stack([r for _, r in pairs]), dev), s, reverse=[False, True, False])
    return run


def speckles(dev):
    disp = (np.floor(u("speckle", (2, 9, 11), 0.0, 4.0)) * 16 - 16).astype(np.int16)      # levels -16 (invalid) .. 32 in small patches
    return stereo.filter_speckles(g(disp, dev), -16, 3, 16)


def smooth(B, C, H, W):
    def run(dev):
        return ph.get_smooth_loss(g(u("sm_d", (B, 1, H, W), 0.1, 1.0), dev), g(u("sm_i", (B, C, H, W), 0.0, 1.0), dev))
    return run


def ssim_backward(dev):
    x, y = (g(u(tag, (1, 3, 4, 5), 0.0, 1.0), dev).requires_grad_(True) for tag in ("ssim_x", "ssim_y"))
    (ph.SSIM()(x, y) * g(u("ssim_w", (1, 3, 4, 5), 0.0, 1.0), dev)).sum().backward()
    return x.grad, y.grad


def warp_backward(dev):
    _, src, depth, K, inv_K, T = photo_case(B=2, H=6, W=8, seed=7)
    d, Tt = g(depth, dev).requires_grad_(True), g(T, dev).requires_grad_(True)
    out = ph.warp_frame(g(src, dev), d, g(K, dev), g(inv_K, dev), Tt)
    (out * g(u("warp_w", tuple(out.shape), 0.0, 1.0), dev)).sum().backward()
    return out.detach(), d.grad, Tt.grad


OPERATORS = {
    "kitti_metrics_6x20_11x37_median": kitti(2, 6, 20, 11, 37, True),
    "kitti_metrics_6x20_11x37_plain": kitti(2, 6, 20, 11, 37, False),
    "kitti_metrics_48x64_96x128_fp64_partials": kitti(2, 48, 64, 96, 128, True),
    "canny_dbe_23x70": edges(2, 23, 70),
    "canny_dbe_48x64": edges(2, 48, 64),
    "disparity_normalize_colorize": images,
    "project_lidar_3x4x2": lidar("exact_4x2", [0, 60, 130, 200]),
    "project_lidar_2x5x1": lidar("exact_5x1", [0, 90, 200]),
    "color_pyramid_color_jitter": inputs,
    "sgbm_3x12x48_c1": sgbm(1),
    "sgbm_3x12x48_c3": sgbm(3),
    "filter_speckles_2x9x11": speckles,
    "get_smooth_loss_1x3x2x2": smooth(1, 3, 2, 2),
    "get_smooth_loss_2x3x40x32": smooth(2, 3, 40, 32),
    "ssim_backward_1x3x4x5": ssim_backward,
    "warp_frame_backward_2x3x6x8": warp_backward,
}


def bits(out):
    """the outputs' bytes on the host, None kept: bit equality, NaN included"""
    out = out if isinstance(out, (tuple, list)) else (out,)
    return [None if t is None else t.detach().contiguous().reshape(-1).cpu().numpy().view(np.uint8) for t in out]


def same(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y)) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(OPERATORS))
def test_guarded_workspace_gives_the_same_bits(dev, monkeypatch, name):
    run = OPERATORS[name]
    plain = bits(run(dev))
    assert any(t is not None and t.size for t in plain)
    for fill in (0x00, 0xFF):
        guarded = Guarded(fill)
        with monkeypatch.context() as m:
            m.setattr(_lib, "byte_workspace", guarded.byte_workspace)
            m.setattr(_lib, "float_workspace", guarded.float_workspace)
            got = bits(run(dev))
            torch.cuda.synchronize()
        assert guarded.handed, "%s allocated no workspace through _lib" % name
        assert guarded.guards_hold(), "%s wrote outside the %s bytes its query answers (fill 0x%02X)" % (name, [n for _, n in guarded.handed], fill)
        assert same(got, plain), "%s: a workspace filled with 0x%02X changes the result" % (name, fill)
