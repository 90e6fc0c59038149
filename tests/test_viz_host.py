"""CPU: the colour-image entry points refuse what they must before any HIP call (dummy non-null pointers never reach a
kernel), the Python functions refuse CPU tensors, and nothing in the build lets the compiler reorder float arithmetic."""
import pytest
import torch

from wavelet_monodepth_amd import _lib, build, visualize as viz

STATE = (8 + 3 * 2048) * 4      # bytes of selection state per image


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def disparity(lib, disp=1, B=2, h=6, w=20, H=11, W=37, q=95.0, lut=1, rgb=4, resized=None, rng=None, ws=4, n=None):
    n = lib.wmd_viz_workspace_bytes(B, H, W) if n is None else n
    return lib.wmd_viz_disparity(disp, B, h, w, H, W, q, lut, rgb, resized, rng, ws, n, None)


def colorize(lib, x=1, B=2, n=35, auto=1, lut=1, out=4, ws=4, nbytes=None):
    nbytes = lib.wmd_viz_workspace_bytes(B, 1, 1) if nbytes is None else nbytes
    return lib.wmd_viz_colorize(x, B, n, auto, 0.1, 9.9, lut, out, 1, ws, nbytes, None)


def normalize(lib, x=1, y=4, B=2, n=35, ws=4, nbytes=None):
    nbytes = lib.wmd_viz_workspace_bytes(B, 1, 1) if nbytes is None else nbytes
    return lib.wmd_viz_normalize(x, y, B, n, ws, nbytes, None)


def test_workspace_size(lib):
    assert lib.wmd_viz_workspace_bytes(2, 11, 37) == 2 * STATE + 2 * 11 * 37 * 4
    assert lib.wmd_viz_workspace_bytes(1, 1, 1) == STATE + 4
    for shape in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4)):
        assert lib.wmd_viz_workspace_bytes(*shape) == 0
    sizes = [lib.wmd_viz_workspace_bytes(B, 375, 1242) for B in range(1, 14)]
    assert all(b > a for a, b in zip(sizes, sizes[1:]))                    # monotone in B


def test_null_pointers(lib):
    for kw in (dict(disp=None), dict(lut=None), dict(rgb=None), dict(ws=None)):
        assert disparity(lib, **kw) == -1, kw
        assert b"null" in lib.wmd_last_error()
    for kw in (dict(x=None), dict(lut=None), dict(out=None), dict(ws=None)):
        assert colorize(lib, **kw) == -1, kw
    for kw in (dict(x=None), dict(y=None), dict(ws=None)):
        assert normalize(lib, **kw) == -1, kw


def test_bad_shapes(lib):
    for kw in (dict(B=0), dict(h=0), dict(w=-1), dict(H=0), dict(W=0)):
        assert disparity(lib, n=1 << 30, **kw) == -2, kw
    for kw in (dict(B=0), dict(n=0)):
        assert colorize(lib, nbytes=1 << 30, **kw) == -2, kw
        assert normalize(lib, nbytes=1 << 30, **kw) == -2, kw
    assert disparity(lib, H=65536, W=32768, n=1 << 62) == -3               # 2^31 pixels


def test_percentile_range(lib):
    for q in (-0.001, 100.001, float("nan"), float("inf")):
        assert disparity(lib, q=q) == -1, q
        assert b"percentile" in lib.wmd_last_error()


def test_short_or_misaligned_workspace(lib):
    n = lib.wmd_viz_workspace_bytes(2, 11, 37)
    assert disparity(lib, n=n - 1) == -5
    assert b"workspace" in lib.wmd_last_error()
    assert disparity(lib, ws=6) == -1
    assert colorize(lib, nbytes=2 * STATE - 1) == -5                       # the state is what the automatic range needs
    assert normalize(lib, nbytes=2 * STATE - 1) == -5
    assert colorize(lib, ws=6) == -1
    assert normalize(lib, ws=6) == -1


def test_python_functions_refuse_cpu_tensors_and_bad_arguments():
    with pytest.raises(_lib.WmdError):
        viz.disparity_image(torch.zeros(1, 8, 8))
    with pytest.raises(_lib.WmdError):
        viz.colorize(torch.zeros(1, 8, 8))
    with pytest.raises(_lib.WmdError):
        viz.normalize_image(torch.zeros(1, 8, 8))
    for kw in (dict(vmin=None), dict(vmax=None)):
        with pytest.raises(ValueError):
            viz.colorize(torch.zeros(1, 8, 8), **kw)
    with pytest.raises(ValueError):
        viz.disparity_image(torch.zeros(1, 8, 8), percentile=101)
    with pytest.raises(ValueError):
        viz.colormap("viridis")
    assert viz.colormap("magma").shape == (256, 3)


def test_no_fast_math_reaches_the_kernels():
    """the byte-for-byte results rest on IEEE division and on separately rounded operations"""
    bad = ("-ffast-math", "-Ofast", "-funsafe-math-optimizations", "-freciprocal-math", "-fno-hip-fp32-correctly-rounded-divide-sqrt",
           "-fapprox-func", "-ffinite-math-only", "-fassociative-math")
    assert not [f for f in build.CXXFLAGS if f in bad or f.startswith("-ffp-model")], build.CXXFLAGS
    src = open(build.CSRC + "/wmd_viz.hip").read()
    assert "#pragma clang fp contract(off)" in src
