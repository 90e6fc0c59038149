"""CPU: the depth-boundary entry points refuse what they must before any HIP call (dummy non-null pointers never reach a
kernel), and the Python functions refuse CPU tensors."""
import pytest
import torch

from wavelet_monodepth_amd import _lib, evaluation as ev


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def dbe(lib, pred=1, gt=1, mask=None, out=1, edges=None, B=2, H=48, W=64, low=0.15, high=0.3, ws=1, n=None):
    n = lib.wmd_eval_dbe_workspace_bytes(B, H, W) if n is None else n
    return lib.wmd_eval_dbe(pred, gt, mask, out, edges, B, H, W, low, high, ws, n, None)


def canny(lib, img=1, edges=1, B=2, H=48, W=64, sigma=1.0, ws=1, n=None):
    n = lib.wmd_eval_dbe_workspace_bytes(B, H, W) if n is None else n
    return lib.wmd_eval_canny(img, edges, B, H, W, sigma, 0.1, 0.2, ws, n, None)


def test_workspace_size(lib):
    # [B,208] uint32 of state, a float64 plane, three bit planes of 2 * ceil(W / 64) words per row
    assert lib.wmd_eval_dbe_workspace_bytes(2, 48, 64) == 2 * 208 * 4 + 2 * 48 * 64 * 8 + 3 * 2 * 48 * 2 * 4
    assert lib.wmd_eval_dbe_workspace_bytes(1, 23, 70) == 208 * 4 + 23 * 70 * 8 + 3 * 23 * 4 * 4
    for shape in ((0, 48, 64), (1, 2, 64), (1, 48, 2), (-1, 5, 5)):
        assert lib.wmd_eval_dbe_workspace_bytes(*shape) == 0


def test_null_pointers(lib):
    for kw in (dict(pred=None), dict(gt=None), dict(out=None), dict(ws=None)):
        assert dbe(lib, **kw) == -1, kw
        assert b"null" in lib.wmd_last_error()
    for kw in (dict(img=None), dict(edges=None), dict(ws=None)):
        assert canny(lib, **kw) == -1, kw


def test_bad_shapes(lib):
    for kw in (dict(B=0), dict(H=2), dict(W=2), dict(H=-4)):
        assert dbe(lib, n=1 << 20, **kw) == -2, kw
        assert canny(lib, n=1 << 20, **kw) == -2, kw


def test_unsupported_before_any_launch(lib):
    # 480 x 640 needs 9600 words per bit plane; the limit is 16384
    assert dbe(lib, B=1, H=480, W=640, n=0) == -5
    assert dbe(lib, B=1, H=512, W=1024, n=0) == -5          # 512 * 32 = 16384: the last size that fits
    assert dbe(lib, B=1, H=513, W=1024, n=1 << 40) == -3
    assert b"LDS" in lib.wmd_last_error()
    assert canny(lib, B=1, H=1024, W=1024, n=1 << 40) == -3
    assert canny(lib, sigma=3.2) == -3                      # radius 13
    assert canny(lib, sigma=3.1, n=0) == -5                 # radius 12: only the workspace is missing
    assert canny(lib, sigma=0.0) == -1
    assert canny(lib, sigma=float("nan")) == -1


def test_short_workspace(lib):
    n = lib.wmd_eval_dbe_workspace_bytes(2, 48, 64)
    assert dbe(lib, n=n - 1) == -5
    assert b"workspace" in lib.wmd_last_error()
    assert canny(lib, n=n - 1) == -5
    assert dbe(lib, ws=12, n=n) == -1                       # enough bytes, not 8-byte aligned


def test_python_functions_refuse_cpu_tensors():
    with pytest.raises(_lib.WmdError):
        ev.canny(torch.zeros(1, 8, 8))
    with pytest.raises(_lib.WmdError):
        ev.compute_depth_boundary_error(torch.zeros(1, 8, 8, dtype=torch.uint8), torch.ones(1, 8, 8))
