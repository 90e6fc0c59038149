"""CPU: wmd_depth_hints_fuse refuses what it must before any HIP call (dummy non-null pointers never reach a kernel), and the
Python functions refuse CPU tensors."""
import pytest
import torch

from wavelet_monodepth_amd import _lib, depth_hints as dh


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def fuse(lib, cand=1, base=1, lookup=1, K=1, inv_K=1, T=1, best_depth=1, best_index=1, losses=None, B=2, M=12, C=3, H=16, W=24,
         ws=None, n=0):
    return lib.wmd_depth_hints_fuse(cand, 1, 37.0, base, lookup, K, inv_K, T, best_depth, best_index, losses, B, M, C, H, W, 1e-7, 0.85,
                                    0.15, ws, n, None)


def test_null_pointers(lib):
    for name in ("cand", "base", "lookup", "K", "inv_K", "T", "best_depth", "best_index"):
        assert fuse(lib, **{name: None}) == -1, name
        assert b"null" in lib.wmd_last_error()


def test_bad_shapes(lib):
    for kw in (dict(M=0), dict(M=-3), dict(H=1), dict(W=1), dict(C=0), dict(B=0)):
        assert fuse(lib, **kw) == -2, kw
    assert b"reflection" in lib.wmd_last_error()


def test_unsupported_before_any_launch(lib):
    assert fuse(lib, C=4) == -3
    assert b"channels" in lib.wmd_last_error()
    assert dh.MAX_CANDIDATES >= 12
    assert fuse(lib, M=dh.MAX_CANDIDATES + 1) == -3
    assert b"candidates" in lib.wmd_last_error()
    assert fuse(lib, B=1, M=12, H=20000, W=20000) == -3          # more than 2^31 candidate values


def test_short_workspace(lib):
    """the size the library asks for is the floor: anything below it, and a size claimed for a NULL pointer, is refused.  The
    kernel stages nothing in device memory, so the query may return 0 (it does today); then no size is below it and the
    refusal that remains is the claimed size without a pointer."""
    for shape in ((2, 12, 16, 24), (1, 12, 320, 1024), (8, 12, 192, 640)):
        n = lib.wmd_depth_hints_workspace_floats(*shape)
        B, M, H, W = shape
        if n > 0:
            assert fuse(lib, B=B, M=M, H=H, W=W, ws=1, n=n - 1) == -5
            assert b"workspace" in lib.wmd_last_error()
            assert fuse(lib, B=B, M=M, H=H, W=W, ws=None, n=0) == -5
        assert fuse(lib, B=B, M=M, H=H, W=W, ws=None, n=n + 64) == -5
        assert b"workspace" in lib.wmd_last_error()


def test_python_functions_refuse_cpu_tensors():
    eye = torch.eye(4)[None]
    with pytest.raises(_lib.WmdError):
        dh.fuse_depth_hints(torch.ones(1, 2, 8, 8), torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8), eye, eye, eye)
    with pytest.raises(_lib.WmdError):
        dh.fuse_depth_hints(torch.ones(2, 8, 8), torch.zeros(3, 8, 8), torch.zeros(3, 8, 8), eye[0], eye[0], eye[0])
    with pytest.raises(_lib.WmdError):
        dh.disparity_to_depth(torch.ones(2, 8, 8), 37.0)
