"""CPU: the host half of the KITTI training inputs.  The new exports load; wmd_lanczos_table equals the oracle's tables
exactly; wmd_color_pyramid and wmd_color_jitter refuse what they must before any HIP call (dummy non-null pointers never
reach a kernel); the workspace queries answer 0 for a shape the call refuses; the Python layer refuses CPU tensors and
parameter sets that are no jitter."""
import numpy as np
import pytest
import torch

import inputs_cases
import inputs_ref as R
from wavelet_monodepth_amd import _lib, kitti_inputs as ki

P = 4096   # a dummy pointer that passes the alignment checks


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def test_exports_load(lib):
    for name in ("wmd_lanczos_ksize", "wmd_lanczos_table", "wmd_color_pyramid_table_ints", "wmd_color_pyramid_tables",
                 "wmd_color_pyramid_workspace_bytes", "wmd_color_pyramid", "wmd_color_jitter_workspace_bytes", "wmd_color_jitter"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES


@pytest.mark.parametrize("n_in,n_out", inputs_cases.table_pairs())
def test_lanczos_table_equals_the_oracle(lib, n_in, n_out):
    assert lib.wmd_lanczos_ksize(n_in, n_out) == R.lanczos_ksize(n_in, n_out)
    bounds, coeffs = ki.lanczos_table(n_in, n_out)
    want_b, want_k = R.lanczos_table(n_in, n_out)
    assert np.array_equal(bounds, want_b) and np.array_equal(coeffs, want_k)


def test_table_pairs_hold_the_training_sizes():
    pairs = inputs_cases.table_pairs()
    for p in [(375, 192), (1242, 640), (375, 320), (1242, 1024), (47, 24), (161, 80), (5, 2), (7, 3), (10, 16), (14, 24), (12, 12)]:
        assert p in pairs


def test_lanczos_table_refusals(lib):
    b, k = np.zeros((3, 2), np.int32), np.zeros((3, 7), np.int32)
    ksize = R.lanczos_ksize(7, 3)
    assert ksize > 7
    assert lib.wmd_lanczos_ksize(0, 3) == 0 and lib.wmd_lanczos_ksize(3, 0) == 0 and lib.wmd_lanczos_ksize(32769, 3) == 0
    assert lib.wmd_lanczos_table(7, 3, None, k.ctypes.data, ksize) == -1
    assert lib.wmd_lanczos_table(7, 3, b.ctypes.data, None, ksize) == -1
    assert lib.wmd_lanczos_table(0, 3, b.ctypes.data, k.ctypes.data, 7) == -2
    assert lib.wmd_lanczos_table(7, 3, b.ctypes.data, k.ctypes.data, 7) == -1       # not the pair's ksize: nothing is written to the short rows
    assert b"ksize" in lib.wmd_last_error() and not k.any()


def test_pyramid_tables_are_the_per_axis_tables_level_after_level(lib):
    H0, W0, h, w, S = 47, 161, 24, 80, 4
    n = lib.wmd_color_pyramid_table_ints(H0, W0, h, w, S)
    buf = np.zeros(n, np.int32)
    assert lib.wmd_color_pyramid_tables(H0, W0, h, w, S, buf.ctypes.data, n) == 0
    want, hi, wi = [], H0, W0
    for s in range(S):
        for a, b in ((wi, w >> s), (hi, h >> s)):
            bounds, coeffs = R.lanczos_table(a, b)
            want += [bounds.ravel(), coeffs.ravel()]
        hi, wi = h >> s, w >> s
    assert np.array_equal(buf, np.concatenate(want))
    assert lib.wmd_color_pyramid_tables(H0, W0, h, w, S, buf.ctypes.data, n - 1) == -1
    assert lib.wmd_color_pyramid_tables(H0, W0, h, w, S, None, n) == -1
    assert lib.wmd_color_pyramid_table_ints(H0, W0, h, w, 6) == 0                   # 24 >> 5 = 0 rows


def pyramid(lib, frames=P, N=5, H0=47, W0=161, h=24, w=80, S=4, flip=P, enable=P, order=P, factors=P, hue=P, tables=P, levels=P,
            color=P, aug=P, ws=P, n=None):
    if n is None:
        n = lib.wmd_color_pyramid_workspace_bytes(N, H0, W0, h, w, S)
    return lib.wmd_color_pyramid(frames, N, H0, W0, h, w, S, flip, enable, order, factors, hue, tables, levels, color, aug, ws, n, None)


def test_pyramid_null_pointers(lib):
    for name in ("frames", "tables", "levels", "color"):
        assert pyramid(lib, **{name: None}) == -1, name
        assert b"null" in lib.wmd_last_error()
    for name in ("order", "factors", "hue", "aug"):                                   # jitter given in part
        assert pyramid(lib, **{name: None}) == -1, name
    # flip is optional, and so is the whole jitter: both pass every check and stop at the workspace
    assert pyramid(lib, flip=None, ws=None) == -5
    assert pyramid(lib, enable=None, order=None, factors=None, hue=None, aug=None, ws=None) == -5


def test_pyramid_bad_shapes(lib):
    for kw in (dict(N=0), dict(H0=0), dict(W0=-1), dict(h=0), dict(w=0), dict(S=0), dict(S=-1), dict(S=9),
               dict(S=6),                  # 24 >> 5: the last level would have no rows
               dict(h=64, w=4, S=4)):      # 4 >> 3: ... no columns
        assert pyramid(lib, n=1 << 20, **kw) == -2, kw
        a = dict(N=5, H0=47, W0=161, h=24, w=80, S=4)
        a.update(kw)
        assert lib.wmd_color_pyramid_workspace_bytes(a["N"], a["H0"], a["W0"], a["h"], a["w"], a["S"]) == 0
    assert b"empty" in lib.wmd_last_error()
    assert pyramid(lib, S=5, ws=None) == -5                                          # 24 >> 4 = 1 row: the deepest level allowed


def test_pyramid_unsupported_before_any_launch(lib):
    assert pyramid(lib, H0=32769, n=1 << 20) == -3
    assert pyramid(lib, N=65536, n=1 << 20) == -3
    assert lib.wmd_color_pyramid_workspace_bytes(1, 32769, 8, 8, 8, 1) == 0
    # 32768 rows -> 1: one output row reads all of them, 32768 x 64 x 3 bytes of LDS
    assert lib.wmd_color_pyramid_workspace_bytes(1, 32768, 8, 1, 8, 1) == 0
    assert pyramid(lib, N=1, H0=32768, W0=8, h=1, w=8, S=1, n=1 << 20) == -3
    assert b"LDS" in lib.wmd_last_error()


def test_pyramid_workspace(lib):
    for N, S in ((1, 1), (5, 4), (36, 4)):
        n = lib.wmd_color_pyramid_workspace_bytes(N, 375, 1242, 192, 640, S)
        assert n == 8 * N * S                                                        # one 64-bit grey sum per (level, image)
        kw = dict(N=N, H0=375, W0=1242, h=192, w=640, S=S)
        assert pyramid(lib, n=n - 1, **kw) == -5
        assert b"workspace" in lib.wmd_last_error()
        assert pyramid(lib, ws=None, **kw) == -5
        assert pyramid(lib, ws=P + 4, **kw) == -5


def jitter(lib, images=P, out=P, N=3, h=12, w=20, enable=P, order=P, factors=P, hue=P, ws=P, n=None):
    if n is None:
        n = lib.wmd_color_jitter_workspace_bytes(N, h, w)
    return lib.wmd_color_jitter(images, out, N, h, w, enable, order, factors, hue, ws, n, None)


def test_jitter_refusals(lib):
    for name in ("images", "out", "enable", "order", "factors", "hue"):
        assert jitter(lib, **{name: None}) == -1, name
        assert b"null" in lib.wmd_last_error()
    for kw in (dict(N=0), dict(h=0), dict(w=-2)):
        assert jitter(lib, n=64, **kw) == -2, kw
    assert jitter(lib, N=1, h=65536, w=32768, n=64) == -3 and lib.wmd_color_jitter_workspace_bytes(1, 65536, 32768) == 0
    assert jitter(lib, N=65536, n=1 << 20) == -3
    assert lib.wmd_color_jitter_workspace_bytes(3, 12, 20) == 24
    assert jitter(lib, n=23) == -5 and jitter(lib, ws=None) == -5 and jitter(lib, ws=P + 4) == -5
    assert lib.wmd_color_jitter_workspace_bytes(1, 4096, 4096) == 8                  # the colour cube passes


def params(n=2, **kw):
    a = dict(enable=np.ones(n, np.uint8), order=np.tile(np.arange(4, dtype=np.uint8), (n, 1)), factors=np.ones((n, 3), np.float32),
             hue_shift=np.zeros(n, np.int32))
    a.update(kw)
    return ki.ColorJitterParams(**a)


def test_jitter_params_are_validated_on_the_host():
    assert len(params(3)) == 3 and params().order.dtype == torch.uint8
    with pytest.raises(_lib.WmdError, match="permutation"):
        params(order=np.array([[0, 1, 2, 3], [0, 1, 1, 3]], np.uint8))
    with pytest.raises(_lib.WmdError, match="permutation"):
        params(order=np.array([[0, 1, 2, 4], [0, 1, 2, 3]], np.uint8))
    with pytest.raises(_lib.WmdError, match="hue_shift"):
        params(hue_shift=np.array([0, 256], np.int32))
    with pytest.raises(_lib.WmdError, match="finite"):
        params(factors=np.array([[1, 1, np.nan], [1, 1, 1]], np.float32))
    with pytest.raises(_lib.WmdError):
        params(order=np.zeros((2, 3), np.uint8))
    with pytest.raises(_lib.WmdError):
        params(factors=torch.ones(2, 3, dtype=torch.float64))
    p = params(3).repeat_interleave(2)
    assert len(p) == 6 and p.order.shape == (6, 4)


def test_cpu_tensors_raise():
    frames = torch.zeros(2, 10, 14, 3, dtype=torch.uint8)
    with pytest.raises(_lib.WmdError):
        ki.color_pyramid(frames, 4, 6, 1)
    with pytest.raises(_lib.WmdError):
        ki.color_pyramid(frames.numpy(), 4, 6, 1)
    with pytest.raises(_lib.WmdError):
        ki.color_jitter(frames, params())
    with pytest.raises(_lib.WmdError):
        ki.preprocess({0: frames, 1: frames}, 4, 6, range(1))
    with pytest.raises(_lib.WmdError):
        ki.preprocess({}, 4, 6)
