"""CPU: the numpy oracle of the NYUv2 training inputs (tests/nyu_inputs_ref.py) against the fixture that the reference's own
transforms wrote over Pillow (tests/golden/make_golden_nyu_inputs.py): small cases by value, the 480 x 640 cases by SHA-256 and
a subsample.  The library's host half: the bicubic (and, through the same code, Lanczos) tables against the oracle's,
gamma_lut, the augmentation draw, and every refusal wmd_nyu_inputs makes before any HIP call (dummy non-null pointers never
reach a kernel)."""
import hashlib
import os

import numpy as np
import pytest
import torch

import inputs_cases
import nyu_inputs_cases as cases
import nyu_inputs_ref as R
from wavelet_monodepth_amd import _lib, kitti_inputs as ki, nyu_inputs as ni

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nyu_inputs_reference.npz")
P = 4096   # a dummy pointer that passes the alignment checks


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def test_fixture_names_its_pillow(golden):
    assert str(golden["pillow"]).startswith("12.2")
    assert os.path.getsize(GOLDEN) < 400000


@pytest.mark.parametrize("name", cases.SMALL)
def test_oracle_equals_the_pillow_chain(golden, name):
    c = cases.build(name)
    for i in range(len(c["image"])):
        image, depth = cases.oracle(c, i)
        assert image.dtype == np.uint8 and np.array_equal(image, golden[name + "|image"][i]), i
        assert depth.dtype == np.uint8 and np.array_equal(depth, golden[name + "|depth"][i]), i


@pytest.mark.parametrize("name", cases.REAL)
def test_oracle_equals_the_reference_classes_by_hash(golden, name):
    c = cases.build(name)
    for i in range(len(c["image"])):
        image, depth = cases.oracle(c, i)
        assert np.array_equal(image[::8, ::8], golden["%s|image_sub|%d" % (name, i)]), i
        assert np.array_equal(depth[::8, ::8], golden["%s|depth_sub|%d" % (name, i)]), i
        assert hashlib.sha256(image.tobytes()).hexdigest() == str(golden["%s|image_sha|%d" % (name, i)]), i
        d = R.depth_tensor(depth)
        assert d.dtype == np.float32 and d.shape == (1,) + c["depth_size"]
        assert hashlib.sha256(np.ascontiguousarray(d).tobytes()).hexdigest() == str(golden["%s|depth_sha|%d" % (name, i)]), i


def test_gamma_lut_is_the_table_pillow_applies(golden):
    for g in (0.8, 1.0, 1.25):
        lut = ni.gamma_lut(g)
        assert lut.dtype == np.uint8 and lut.shape == (256,)
        assert np.array_equal(lut, golden["gamma|%s" % g]) and np.array_equal(lut, R.gamma_lut(g)), g
    assert ni.gamma_lut(1.0)[254] == 255                                             # not the identity
    assert (ni.gamma_lut(1.0) != np.arange(256)).sum() > 0 and ni.gamma_lut(0.8)[0] == 0 and ni.gamma_lut(1.25)[255] == 255
    with pytest.raises(_lib.WmdError):
        ni.gamma_lut(0.0)
    assert ni.PERMS == R.PERMS == [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


@pytest.mark.parametrize("n_in,n_out", cases.table_pairs())
def test_bicubic_table_equals_the_oracle(lib, n_in, n_out):
    assert lib.wmd_resample_ksize(ni.FILTER_BICUBIC, n_in, n_out) == R.ksize(n_in, n_out)
    bounds, coeffs = ni.bicubic_table(n_in, n_out)
    want_b, want_k = R.table(n_in, n_out)
    assert np.array_equal(bounds, want_b) and np.array_equal(coeffs, want_k)


def test_table_pairs_hold_the_reference_sizes():
    pairs = cases.table_pairs()
    for p in [(608, 640), (448, 480), (608, 320), (448, 240), (608, 224), (448, 224), (155, 170), (55, 60), (155, 85), (55, 30),
              (7, 3), (5, 2), (64, 100), (48, 72), (64, 32), (48, 24), (48, 60), (32, 32), (48, 48), (32, 20)]:
        assert p in pairs, p


@pytest.mark.parametrize("n_in,n_out", inputs_cases.table_pairs())
def test_generalised_table_with_the_lanczos_filter_equals_wmd_lanczos_table(lib, n_in, n_out):
    assert lib.wmd_resample_ksize(ni.FILTER_LANCZOS, n_in, n_out) == lib.wmd_lanczos_ksize(n_in, n_out)
    bounds, coeffs = ni.resample_table(ni.FILTER_LANCZOS, n_in, n_out)
    want_b, want_k = ki.lanczos_table(n_in, n_out)
    assert np.array_equal(bounds, want_b) and np.array_equal(coeffs, want_k)
    ob, ok = R.table(n_in, n_out, R.LANCZOS)
    assert np.array_equal(bounds, ob) and np.array_equal(coeffs, ok)


def test_resample_table_refusals(lib):
    ksize = R.ksize(7, 3)
    b, k = np.zeros((3, 2), np.int32), np.zeros((3, ksize), np.int32)
    assert lib.wmd_resample_ksize(0, 0, 3) == 0 and lib.wmd_resample_ksize(0, 3, 0) == 0 and lib.wmd_resample_ksize(0, 32769, 3) == 0
    assert lib.wmd_resample_ksize(2, 7, 3) == 0 and lib.wmd_resample_ksize(-1, 7, 3) == 0
    assert lib.wmd_resample_table(0, 7, 3, None, k.ctypes.data, ksize) == -1
    assert lib.wmd_resample_table(0, 7, 3, b.ctypes.data, None, ksize) == -1
    assert lib.wmd_resample_table(2, 7, 3, b.ctypes.data, k.ctypes.data, ksize) == -1
    assert b"filter" in lib.wmd_last_error()
    assert lib.wmd_resample_table(0, 0, 3, b.ctypes.data, k.ctypes.data, ksize) == -2
    assert lib.wmd_resample_table(0, 7, 3, b.ctypes.data, k.ctypes.data, ksize - 2) == -1
    assert b"ksize" in lib.wmd_last_error() and not k.any()
    assert lib.wmd_resample_table(0, 7, 3, b.ctypes.data, k.ctypes.data, ksize) == 0 and k.any()


def test_call_tables_are_the_four_per_axis_tables(lib):
    H0, W0, crop, ih, iw, dh, dw = 61, 161, 3, 60, 170, 30, 85
    n = lib.wmd_nyu_inputs_table_ints(H0, W0, crop, ih, iw, dh, dw)
    buf = np.zeros(n, np.int32)
    assert lib.wmd_nyu_inputs_tables(H0, W0, crop, ih, iw, dh, dw, buf.ctypes.data, n) == 0
    want = []
    for a, b in ((155, iw), (55, ih), (155, dw), (55, dh)):
        bounds, coeffs = R.table(a, b)
        want += [bounds.ravel(), coeffs.ravel()]
    assert np.array_equal(buf, np.concatenate(want))
    assert lib.wmd_nyu_inputs_tables(H0, W0, crop, ih, iw, dh, dw, buf.ctypes.data, n - 1) == -1
    assert lib.wmd_nyu_inputs_tables(H0, W0, crop, ih, iw, dh, dw, None, n) == -1
    assert lib.wmd_nyu_inputs_table_ints(H0, W0, 31, ih, iw, dh, dw) == 0            # 2 crop >= H0


def call(lib, image_u8=P, depth_u8=P, B=7, H0=61, W0=161, crop=3, ih=60, iw=170, dh=30, dw=85, flip=P, perm=P, lut=P, tables=P, n=None,
         image=P, depth=P, disp=P, image_r=P, depth_r=P):
    if n is None:
        n = lib.wmd_nyu_inputs_table_ints(H0, W0, crop, ih, iw, dh, dw)
    return lib.wmd_nyu_inputs(image_u8, depth_u8, B, H0, W0, crop, ih, iw, dh, dw, flip, perm, lut, tables, n, image, depth, disp, image_r,
                              depth_r, None)


def test_entry_point_refusals_without_a_gpu(lib):
    for name in ("image_u8", "depth_u8", "tables", "image", "depth"):
        assert call(lib, **{name: None}) == -1, name
        assert b"null" in lib.wmd_last_error()
    assert call(lib, tables=P + 2) == -1
    for kw in (dict(B=0), dict(H0=0), dict(W0=-1), dict(ih=0), dict(iw=0), dict(dh=0), dict(dw=-3), dict(crop=-1)):
        assert call(lib, n=100, **kw) == -2, kw
    for kw in (dict(crop=31), dict(crop=30, H0=60), dict(crop=81), dict(H0=400, crop=81),dict(crop=1 << 30)):   # 2 crop >= H0 or W0
        assert call(lib, n=100, **kw) == -2, kw
        assert b"crop" in lib.wmd_last_error()
    n = lib.wmd_nyu_inputs_table_ints(61, 161, 3, 60, 170, 30, 85)
    assert n > 0
    for bad in (0, n - 1, n + 1):                                                    # a table of the wrong length
        assert call(lib, n=bad) == -1, bad
        assert b"table_ints" in lib.wmd_last_error()
    assert call(lib, H0=32769, n=100) == -3 and call(lib, B=65536, n=100) == -3 and call(lib, iw=32769, n=100) == -3
    assert lib.wmd_nyu_inputs_table_ints(32769, 161, 3, 60, 170, 30, 85) == 0
    # 32768 rows -> 1: one output row reads all of them, 32768 x 64 x 3 bytes of intermediate
    assert lib.wmd_nyu_inputs_table_ints(32768, 161, 0, 1, 170, 30, 85) == 0
    assert call(lib, B=1, H0=32768, crop=0, ih=1, n=100) == -3
    assert b"LDS" in lib.wmd_last_error()


def test_sample_augmentation_ranges():
    g = torch.Generator().manual_seed(3)
    a = ni.sample_augmentation(512, generator=g)
    assert len(a) == 512 and a.flip.dtype == a.perm.dtype == a.lut.dtype == torch.uint8 and a.lut.shape == (512, 256)
    assert 180 < int(a.flip.sum()) < 332 and int(a.flip.max()) == 1                  # p = 0.5
    swapped = int((a.perm != 0).sum())
    assert 0 < swapped < 110 and int(a.perm.max()) <= 5                              # p = 0.1 x 5/6
    lo, hi = ni.gamma_lut(0.8).astype(int), ni.gamma_lut(1.25).astype(int)
    lut = a.lut.numpy().astype(int)
    assert (lut >= hi - 1).all() and (lut <= lo + 1).all()                           # the tables are monotone in gamma, up to the rounding
    assert len({tuple(r) for r in lut.tolist()}) > 400
    b = ni.sample_augmentation(512, generator=torch.Generator().manual_seed(3))
    assert torch.equal(a.flip, b.flip) and torch.equal(a.perm, b.perm) and torch.equal(a.lut, b.lut)
    every = ni.sample_augmentation(256, swap_p=1.0, gamma=0)
    assert every.lut is None and sorted(set(every.perm.tolist())) == [0, 1, 2, 3, 4, 5]
    assert len(ni.sample_augmentation(0)) == 0


def test_augmentation_is_validated_on_the_host():
    a = ni.Augmentation([0, 1], [5, 0], np.tile(np.arange(256, dtype=np.uint8), (2, 1)))
    assert len(a) == 2 and a.lut.shape == (2, 256)
    assert ni.Augmentation([True, False], [0, 0]).lut is None
    with pytest.raises(_lib.WmdError, match="perm"):
        ni.Augmentation([0, 1], [6, 0])
    with pytest.raises(_lib.WmdError):
        ni.Augmentation([0, 1], [0, 0, 0])
    with pytest.raises(_lib.WmdError):
        ni.Augmentation([0, 1], [0, 0], np.zeros((2, 255), np.uint8))
    with pytest.raises(_lib.WmdError):
        ni.Augmentation(torch.zeros(2), [0, 0])                                      # float flip


def test_cpu_tensors_raise():
    image, depth = torch.zeros(2, 20, 24, 3, dtype=torch.uint8), torch.zeros(2, 20, 24, dtype=torch.uint8)
    with pytest.raises(_lib.WmdError, match="GPU only"):
        ni.train_transform(image, depth, image_size=(8, 8), depth_size=(4, 4), crop=2)
    with pytest.raises(_lib.WmdError):
        ni.train_transform(image.numpy(), depth.numpy())


def test_float_conversions_are_true_divisions():
    u8 = np.arange(256, dtype=np.uint8)
    q = (u8.astype(np.float64) / 255.0).astype(np.float32)                           # one rounding of the exact quotient
    assert np.array_equal(R.image_tensor(u8.reshape(16, 16, 1).repeat(3, axis=2))[0].ravel(), q)
    d = R.depth_tensor(u8.reshape(16, 16)).ravel()
    exact = np.clip((q.astype(np.float64) * 1000.0).astype(np.float32), 10, 1000)    # float32 x float32 is exact in float64
    assert d.dtype == np.float32 and np.array_equal(d, exact)
    assert (d[:3] == 10).all() and d[3] > 10 and d[255] == 1000 and d[254] < 1000
    assert (q != u8.astype(np.float32) * np.float32(1.0 / 255.0)).any()              # a reciprocal multiply is not it


def test_cases_cover_what_they_claim(golden):
    sat = cases.build("saturate_52x68")
    box = sat["image"][:, 2:-2, 2:-2]
    assert set(np.unique(box).tolist()) == {0, 255} and set(np.unique(sat["depth"][:, 2:-2, 2:-2]).tolist()) == {0, 255}
    below = above = 0
    for img in box:                                                                  # the horizontal pass before clip8
        acc = R.accumulators(img, *R.table(64, 100))
        below, above = below + int((acc < 0).sum()), above + int((acc > 255).sum())
    assert below > 100 and above > 100
    mid = np.stack([R._pass(img, *R.table(64, 100)) for img in box])                 # ... and the vertical one
    below = above = 0
    for img in mid:
        acc = R.accumulators(img.transpose(1, 0, 2), *R.table(48, 72))
        below, above = below + int((acc < 0).sum()), above + int((acc > 255).sum())
    assert below > 100 and above > 100
    depth = np.stack([R.depth_tensor(d) for d in golden["saturate_52x68|depth"]])
    assert (depth == 10).any() and (depth == 1000).any()                             # both clamp values
    assert ((golden["saturate_52x68|depth"] <= 2) == (depth[:, 0] == 10)).all()
    clip = cases.build("clip_9x11")
    for a, b in ((7, 3), (5, 2)):
        # the unclipped window, 2 x 2 a / b wide, is wider than the crop box: the box cuts every window on at least one side and
        # at least one window is the whole box.  (With the bicubic support of 2 the outer windows of 7 -> 3 are [0, 6) and [1, 7):
        # cut on one side only; both windows of 5 -> 2 are the whole box.)
        bounds, _ = R.table(a, b)
        lo, hi = bounds[:, 0], bounds[:, 0] + bounds[:, 1]
        assert 2 * 2.0 * a / b > a
        assert ((lo == 0) | (hi == a)).all() and ((lo == 0) & (hi == a)).any() and lo.min() == 0 and hi.max() == a
    b5, _ = R.table(5, 2)
    assert (b5[:, 0] == 0).all() and (b5[:, 1] == 5).all()
    assert clip["crop"] == 2 and clip["image"].shape[1:3] == (9, 11)
    tiles = cases.build("tiles_61x161")
    assert sorted(tiles["perm"].tolist()) == [0, 0, 1, 2, 3, 4, 5] and set(tiles["flip"].tolist()) == {0, 1}
    assert tiles["gamma"][:3] == [0.8, 1.0, 1.25] and tiles["gamma"][6] is None and tiles["perm"][6] == 0
    assert np.array_equal(tiles["lut"][6], np.arange(256)) and not np.array_equal(tiles["lut"][1], np.arange(256))
    assert 161 * 3 % 4 and 161 % 4 and tiles["image_size"][1] > 2 * 64 and tiles["image_size"][0] > 3 * 16   # ragged rows, several tiles
    one = cases.build("one_pass_40x56")
    assert one["image_size"][0] == 40 - 8 and one["image_size"][1] != 56 - 8 and one["depth_size"][1] == 56 - 8 and one["depth_size"][0] != 32
    real = cases.build("real_480x640")
    assert real["flip"].tolist() == [1, 0, 1] and real["perm"].tolist() == [4, 0, 2] and real["gamma"] == [0.8, 1.1, 1.25]
    assert R.ksize(608, 224) == 13 and cases.build("real_224")["is_224"]
