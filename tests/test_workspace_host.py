"""CPU: the workspace contract of the data, loss and evaluation operators in one place.

QUERIES: what every size query answered before the layouts were written once (csrc/wmd_ws_layouts.h) -- recorded from the library
built at the commit before, not from the code under test; viz, the depth-boundary errors, LiDAR and the pyramid are pinned by
closed forms in their own host tests.  REFUSALS: what every entry answers to a NULL, a short and a misaligned workspace (size
before alignment; the two conventions for a misaligned one are in DESIGN.md, "Workspaces of the data operators"), with dummy
non-null pointers that never reach a kernel: every call below returns before the first HIP call.  And the two Python helpers every
operator allocates and checks with, _lib.byte_workspace / float_workspace and _lib.require_device, on CPU tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

from wavelet_monodepth_amd import _lib

BAD_ARG, WORKSPACE = -1, -5
P = 4096   # a dummy pointer that passes every alignment check

QUERIES = {
    "wmd_eval_workspace_floats": [
        ((2, 11, 37), 28548),
        ((2, 96, 128), 76072),
        ((1, 375, 1242), 944961),
        ((16, 375, 1242), 15119346),
        ((1, 1, 1), 13463),
        ((0, 11, 37), 0),
        ((2, 0, 37), 0),
    ],
    "wmd_stereo_sgbm_workspace_bytes": [
        ((3, 12, 48, 1, 0, 16, 3), 125952),
        ((3, 12, 48, 3, 0, 16, 3), 181248),
        ((1, 375, 1242, 3, 0, 96, 3), 193901312),
        ((16, 375, 1242, 3, 0, 96, 3), 969506560),       # five images to a group: the 1 GiB cap
        ((2, 37, 211, 3, 5, 160, 5), 3147264),
        ((1, 12, 16, 1, 0, 16, 3), 0),
        ((1, 12, 48, 2, 0, 16, 3), 0),
    ],
    "wmd_stereo_filter_speckles_workspace_bytes": [
        ((2, 9, 11), 1792),
        ((3, 12, 48), 13824),
        ((1, 375, 1242), 3726080),
        ((1, 1, 1), 256),
        ((4, 32, 32), 32768),
        ((0, 9, 11), 0),
        ((65536, 256, 128), 0),
    ],
    "wmd_color_jitter_workspace_bytes": [
        ((2, 5, 7), 16),
        ((3, 48, 64), 24),
        ((26, 12, 20), 208),
        ((12, 192, 640), 96),
        ((1, 1, 1), 8),
        ((65535, 2, 2), 524280),
        ((0, 48, 64), 0),
        ((65536, 2, 2), 0),
    ],
    "wmd_ssim_bwd_workspace_floats": [
        ((1, 3, 4, 5), 180),
        ((2, 3, 40, 32), 23040),
        ((12, 3, 192, 640), 13271040),
        ((1, 1, 2, 2), 12),
        ((4, 1, 7, 9), 756),
        ((0, 3, 4, 5), 0),
        ((1, 3, 0, 5), 0),
    ],
    "wmd_warp_bwd_workspace_floats": [                   # (B, C, H, W) of wmd_warp_args; None: a NULL args pointer
        ((2, 3, 6, 8), 24),
        ((1, 3, 33, 31), 12),
        ((12, 3, 192, 640), 17280),
        ((1, 1, 32, 32), 12),
        ((4, 3, 375, 1242), 12288),
        ((3, 3, 1024, 1024), 9216),
        (None, 0),
    ],
    "wmd_smooth_workspace_floats": [
        ((1, 2, 2), 6),
        ((2, 40, 32), 10),
        ((12, 192, 640), 2050),
        ((1, 192, 640), 242),
        ((1, 32, 64), 6),
        ((64, 375, 1242), 2050),
        ((0, 2, 2), 0),
        ((1, 2, 0), 0),
    ],
    "wmd_depth_hints_workspace_floats": [                # nothing is staged in device memory: 0 is the answer, not a refusal
        ((2, 12, 16, 24), 0),
        ((1, 12, 320, 1024), 0),
        ((8, 12, 192, 640), 0),
        ((1, 1, 2, 2), 0),
        ((16, 64, 375, 1242), 0),
        ((0, 12, 16, 24), 0),
    ],
}


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def warp_args(B, Cc, H, W):
    return _lib.WarpArgs(B=B, C=Cc, H=H, W=W, Hs=H, Ws=W, eps=1e-7, src=P, depth=P, K=P, inv_K=P, T=P)


@pytest.mark.parametrize("name", sorted(QUERIES))
def test_queries_answer_what_they_answered(lib, name):
    for shape, want in QUERIES[name]:
        if name == "wmd_warp_bwd_workspace_floats":
            got = lib.wmd_warp_bwd_workspace_floats(C.byref(warp_args(*shape)) if shape else None)
        else:
            got = getattr(lib, name)(*shape)
        assert got == want, (name, shape)


def eval_kitti(lib, ws, n):
    a = _lib.EvalKittiArgs(B=2, h=6, w=20, H=11, W=37, min_depth=1e-3, max_depth=80.0, mask_mode=1, pred_scale=1.0, median_scaling=1,
                           pred_disp=P, gt_depth=P, out=P, workspace=ws, workspace_floats=n)
    return lib.wmd_eval_kitti(C.byref(a), None)


# entry: (call(lib, ws, n), need(lib), unit in bytes, alignment, status for NULL, status for a misaligned workspace or None)
REFUSALS = {
    "wmd_eval_kitti": (eval_kitti, lambda l: l.wmd_eval_workspace_floats(2, 11, 37), 4, 4, BAD_ARG, None),
    "wmd_eval_canny": (lambda l, ws, n: l.wmd_eval_canny(P, P, 2, 48, 64, 1.0, 0.1, 0.2, ws, n, None),
                       lambda l: l.wmd_eval_dbe_workspace_bytes(2, 48, 64), 1, 8, BAD_ARG, BAD_ARG),
    "wmd_eval_dbe": (lambda l, ws, n: l.wmd_eval_dbe(P, P, None, P, P, 2, 48, 64, 0.15, 0.3, ws, n, None),
                     lambda l: l.wmd_eval_dbe_workspace_bytes(2, 48, 64), 1, 8, BAD_ARG, BAD_ARG),
    "wmd_viz_disparity": (lambda l, ws, n: l.wmd_viz_disparity(P, 2, 6, 20, 11, 37, 95.0, P, P, None, None, ws, n, None),
                          lambda l: l.wmd_viz_workspace_bytes(2, 11, 37), 1, 4, BAD_ARG, BAD_ARG),
    "wmd_viz_normalize": (lambda l, ws, n: l.wmd_viz_normalize(P, P, 2, 35, ws, n, None),
                          lambda l: l.wmd_viz_workspace_bytes(2, 1, 1) - 8, 1, 4, BAD_ARG, BAD_ARG),          # the state alone
    "wmd_viz_colorize": (lambda l, ws, n: l.wmd_viz_colorize(P, 2, 35, 1, 0.0, 0.0, P, P, 1, ws, n, None),
                         lambda l: l.wmd_viz_workspace_bytes(2, 1, 1) - 8, 1, 4, BAD_ARG, BAD_ARG),
    "wmd_lidar_depth_maps": (lambda l, ws, n: l.wmd_lidar_depth_maps(P, P, P, 1000, 2, 6, 8, 0, P, ws, n, None),
                             lambda l: l.wmd_lidar_depth_workspace_bytes(2, 6, 8), 1, 8, WORKSPACE, WORKSPACE),
    "wmd_color_pyramid": (lambda l, ws, n: l.wmd_color_pyramid(P, 4, 375, 1242, 192, 640, 4, P, P, P, P, P, P, P, P, P, ws, n, None),
                          lambda l: l.wmd_color_pyramid_workspace_bytes(4, 375, 1242, 192, 640, 4), 1, 8, WORKSPACE, WORKSPACE),
    "wmd_color_jitter": (lambda l, ws, n: l.wmd_color_jitter(P, P, 3, 12, 20, P, P, P, P, ws, n, None),
                         lambda l: l.wmd_color_jitter_workspace_bytes(3, 12, 20), 1, 8, WORKSPACE, WORKSPACE),
    "wmd_stereo_sgbm": (lambda l, ws, n: l.wmd_stereo_sgbm(P, P, None, P, None, None, 1, 8, 40, 3, 0, 16, 3, 36, 288, 63, 10, 100, 16, 0, 5, ws, n, None),
                        lambda l: l.wmd_stereo_sgbm_workspace_bytes(1, 8, 40, 3, 0, 16, 3), 1, 256, BAD_ARG, WORKSPACE),
    "wmd_stereo_filter_speckles": (lambda l, ws, n: l.wmd_stereo_filter_speckles(P, 2, 5, 7, -16, 10, 16, ws, n, None),
                                   lambda l: l.wmd_stereo_filter_speckles_workspace_bytes(2, 5, 7), 1, 4, BAD_ARG, WORKSPACE),
    "wmd_ssim_bwd": (lambda l, ws, n: l.wmd_ssim_bwd(P, P, P, P, P, 1, 3, 4, 5, 0, 0.85, 0.15, ws, n, None),
                     lambda l: l.wmd_ssim_bwd_workspace_floats(1, 3, 4, 5), 4, 4, WORKSPACE, None),
    "wmd_warp_bwd": (lambda l, ws, n: l.wmd_warp_bwd(C.byref(warp_args(2, 3, 6, 8)), P, P, P, ws, n, None),
                     lambda l: l.wmd_warp_bwd_workspace_floats(C.byref(warp_args(2, 3, 6, 8))), 4, 4, WORKSPACE, None),
    "wmd_smooth_fwd": (lambda l, ws, n: l.wmd_smooth_fwd(P, P, P, 2, 3, 40, 32, 2.0, ws, n, None),
                       lambda l: l.wmd_smooth_workspace_floats(2, 40, 32), 4, 4, WORKSPACE, None),
}


@pytest.mark.parametrize("entry", sorted(REFUSALS))
def test_refusal_matrix(lib, entry):
    call, need, unit, align, null_status, misaligned_status = REFUSALS[entry]
    n = need(lib)
    assert n > 1
    assert call(lib, None, n) == null_status
    assert b"workspace" in lib.wmd_last_error()
    assert call(lib, P, n - 1) == WORKSPACE
    msg = lib.wmd_last_error().decode()
    assert entry in msg and "workspace %d bytes" % ((n - 1) * unit) in msg and "%d needed" % (n * unit) in msg
    if misaligned_status is not None:
        assert call(lib, P + align // 2, n) == misaligned_status
        assert b"workspace" in lib.wmd_last_error() and b"%d-byte aligned" % align in lib.wmd_last_error()
        assert call(lib, P + align // 2, n - 1) == WORKSPACE                   # both at once: the size is tested first


def test_depth_hints_needs_no_workspace_and_refuses_a_claimed_one(lib):
    def fuse(ws, n):
        return lib.wmd_depth_hints_fuse(P, 1, 37.0, P, P, P, P, P, P, P, None, 2, 12, 3, 16, 24, 1e-7, 0.85, 0.15, ws, n, None)
    assert lib.wmd_depth_hints_workspace_floats(2, 12, 16, 24) == 0
    assert fuse(None, 64) == WORKSPACE                   # floats > 0 without a pointer
    assert b"workspace" in lib.wmd_last_error()


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 12, 255, 256, 257])
def test_byte_workspace_is_never_shorter_than_asked(n):
    ws, got = _lib.byte_workspace(n, "cpu")
    assert got == n and ws.dtype == torch.int64 and ws.numel() >= 1
    assert ws.numel() * ws.element_size() >= n
    assert ws.numel() * ws.element_size() < max(n, 8) + 8                   # and no longer than the next word


def test_float_workspace():
    assert _lib.float_workspace(0, "cpu") is None and _lib.ptr(None) is None
    for n in (1, 6, 180):
        ws = _lib.float_workspace(n, "cpu")
        assert ws.dtype == torch.float32 and ws.numel() == n


def test_require_device():
    cpu = torch.zeros(3)
    _lib.require_device("op", x=(None, torch.float32), y=(None, (torch.uint8, torch.bool), "a note"))
    with pytest.raises(_lib.WmdError, match=r"op runs on the GPU only \(x is cpu\)"):
        _lib.require_device("op", skipped=(None, torch.float32), x=(cpu, torch.float32))
    with pytest.raises(_lib.WmdError, match=r"op runs on the GPU only \(pts is ndarray\)"):
        _lib.require_device("op", pts=(np.zeros(3, np.float32), torch.float32))
    # the dtype rule comes after the device rule, so only a device tensor reaches it: a host tensor that says it is one stands in here

    class OnDevice(torch.Tensor):
        is_cuda = True
    dev = cpu.as_subclass(OnDevice)
    _lib.require_device("op", x=(dev, torch.float32))
    _lib.require_device("op", x=(dev, (torch.uint8, torch.float32)))
    _lib.require_device("op", x=(dev, None), y=(dev.to(torch.bool), None, "any dtype"))
    with pytest.raises(_lib.WmdError, match=r"op runs on the GPU only \(mask is cpu\)"):
        _lib.require_device("op", mask=(cpu, None))
    with pytest.raises(_lib.WmdError, match=r"op: x must be torch.float64 \(got torch.float32\)$"):
        _lib.require_device("op", x=(dev, torch.float64))
    with pytest.raises(_lib.WmdError, match=r"op: flip must be torch.uint8 or torch.bool \(got torch.float32\)$"):
        _lib.require_device("op", flip=(dev, (torch.uint8, torch.bool)))
    with pytest.raises(_lib.WmdError, match=r"op: depth_u8 must be torch.uint8 \(got torch.float32\): 16-bit depth maps are not implemented$"):
        _lib.require_device("op", depth_u8=(dev, torch.uint8, "16-bit depth maps are not implemented"))
