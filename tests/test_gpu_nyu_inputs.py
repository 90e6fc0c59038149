"""GPU: nyu_inputs.train_transform against the fixture that the reference's transforms wrote over Pillow
(tests/golden/nyu_inputs_reference.npz) and against the numpy oracle (tests/nyu_inputs_ref.py).  Exact equality everywhere:
uint8 ==, float32 ==.  The shapes are the smallest at which each failure mode can still occur (tests/nyu_inputs_cases.py);
two cases run at the reference's own sizes and are pinned by SHA-256."""
import hashlib
import os

import numpy as np
import pytest
import torch

import nyu_inputs_cases as cases
import nyu_inputs_ref as R
from wavelet_monodepth_amd import _lib, nyu_inputs as ni, wavelets

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nyu_inputs_reference.npz")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


_ORACLE = {}


def oracle(name):
    """(image u8 [N,ih,iw,3], depth u8 [N,dh,dw]) of a case, computed once, read only"""
    if name not in _ORACLE:
        c = cases.build(name)
        items = [cases.oracle(c, i) for i in range(len(c["image"]))]
        _ORACLE[name] = tuple(np.stack([it[k] for it in items]) for k in range(2))
        for a in _ORACLE[name]:
            a.setflags(write=False)
    return _ORACLE[name]


def aug_of(c, dev):
    return ni.Augmentation(c["flip"], c["perm"], c["lut"]).to(dev)


def run(c, dev, aug="case", **kw):
    a = aug_of(c, dev) if isinstance(aug, str) else aug
    out = ni.train_transform(torch.from_numpy(c["image"]).to(dev), torch.from_numpy(c["depth"]).to(dev), a, is_224=c["is_224"], crop=c["crop"],
                             image_size=c["image_size"], depth_size=c["depth_size"], keep_u8=True, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def describe(got, want):
    bad = np.argwhere(got != want)
    return "%d of %d values differ, first at %s: got %s, want %s" % (len(bad), want.size, bad[:3].tolist(), [got[tuple(i)] for i in bad[:3]],
                                                                      [want[tuple(i)] for i in bad[:3]])


def check(got, image_u8, depth_u8):
    n = len(image_u8)
    assert got["image_u8"].dtype == np.uint8 and got["image_u8"].shape == image_u8.shape
    assert got["depth_u8"].dtype == np.uint8 and got["depth_u8"].shape == depth_u8.shape
    assert np.array_equal(got["image_u8"], image_u8), "uint8 image: " + describe(got["image_u8"], image_u8)
    assert np.array_equal(got["depth_u8"], depth_u8), "uint8 depth: " + describe(got["depth_u8"], depth_u8)
    want_i, want_d = np.stack([R.image_tensor(v) for v in image_u8]), np.stack([R.depth_tensor(v) for v in depth_u8])
    assert got["image"].dtype == np.float32 and got["image"].shape == (n, 3) + image_u8.shape[1:3]
    assert got["depth"].dtype == np.float32 and got["depth"].shape == (n, 1) + depth_u8.shape[1:3]
    assert np.array_equal(got["image"], want_i), "image: " + describe(got["image"], want_i)
    assert np.array_equal(got["depth"], want_d), "depth: " + describe(got["depth"], want_d)


@pytest.mark.parametrize("name", cases.SMALL)
def test_small_cases_equal_the_fixture_and_the_oracle(dev, gold, name):
    """tiles_61x161: several tiles on both axes, 483- and 161-byte rows, up- and downscale, mixed flips, all six permutations,
    an item without table; clip_9x11: windows wider than the crop box; saturate_52x68: clip8 on both sides and both depth clamps;
    one_pass_40x56: one pass skipped per plane"""
    c = cases.build(name)
    got = run(c, dev, disparity=True)
    check(got, gold[name + "|image"], gold[name + "|depth"])
    check(got, *oracle(name))
    assert np.array_equal(got["disp_gt"], np.float32(10) / got["depth"]) and got["disp_gt"].dtype == np.float32


@pytest.mark.parametrize("name", cases.REAL)
def test_reference_sizes_equal_the_reference_classes(dev, gold, name):
    """448 x 608 -> 480 x 640 and 240 x 320 (N = 3), and -> 224 x 224 with 13-tap rows: the hashes of what the reference's own
    classes gave, and the oracle"""
    c = cases.build(name)
    got = run(c, dev)
    for i in range(len(c["image"])):
        assert np.array_equal(got["image_u8"][i][::8, ::8], gold["%s|image_sub|%d" % (name, i)]), i
        assert np.array_equal(got["depth_u8"][i][::8, ::8], gold["%s|depth_sub|%d" % (name, i)]), i
        assert hashlib.sha256(np.ascontiguousarray(got["image_u8"][i]).tobytes()).hexdigest() == str(gold["%s|image_sha|%d" % (name, i)]), i
        assert hashlib.sha256(np.ascontiguousarray(got["depth"][i]).tobytes()).hexdigest() == str(gold["%s|depth_sha|%d" % (name, i)]), i
    check(got, *oracle(name))


def test_defaults_are_the_reference_sizes(dev):
    image, depth = torch.zeros(1, 480, 640, 3, dtype=torch.uint8, device=dev), torch.full((1, 480, 640), 128, dtype=torch.uint8, device=dev)
    out = ni.train_transform(image, depth)
    assert sorted(out) == ["depth", "image"] and out["image"].shape == (1, 3, 480, 640) and out["depth"].shape == (1, 1, 240, 320)
    assert float(out["depth"].min()) == float(out["depth"].max()) == float(R.depth_tensor(np.full((1, 1), 128, np.uint8))[0, 0, 0])
    out = ni.train_transform(image, depth, is_224=True, disparity=True)
    assert sorted(out) == ["depth", "disp_gt", "image"] and out["image"].shape == (1, 3, 224, 224) and out["disp_gt"].shape == (1, 1, 224, 224)


def test_no_augmentation_is_no_flip_no_swap_and_no_table(dev):
    c = cases.build("tiles_61x161")
    n = len(c["image"])
    plain = run(c, dev, aug=None)
    same = run(c, dev, aug=ni.Augmentation(np.zeros(n, np.uint8), np.zeros(n, np.uint8)).to(dev))
    ident = run(c, dev, aug=ni.Augmentation(np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.tile(np.arange(256, dtype=np.uint8), (n, 1))).to(dev))
    gamma1 = run(c, dev, aug=ni.Augmentation(np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.tile(ni.gamma_lut(1.0), (n, 1))).to(dev))
    for k in plain:
        assert np.array_equal(plain[k], same[k]) and np.array_equal(plain[k], ident[k]), k
    assert not np.array_equal(plain["image_u8"], gamma1["image_u8"]) and np.array_equal(plain["depth"], gamma1["depth"])
    want = [R.item(c["image"][i], c["depth"][i], c["crop"], c["image_size"], c["depth_size"]) for i in range(n)]
    check(plain, np.stack([w[0] for w in want]), np.stack([w[1] for w in want]))


def test_the_cropped_away_border_is_never_read(dev):
    """clip_9x11 with another border around the same box: every window is cut by the box, and the result does not move"""
    c = cases.build("clip_9x11")
    other = dict(c, image=255 - c["image"], depth=255 - c["depth"])
    other["image"][:, 2:-2, 2:-2], other["depth"][:, 2:-2, 2:-2] = c["image"][:, 2:-2, 2:-2], c["depth"][:, 2:-2, 2:-2]
    a, b = run(c, dev), run(other, dev)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_all_256_depth_codes_through_the_epilogue(dev):
    """depth size == box size: both passes are skipped and every code reaches the conversion; against a correctly rounded
    (u8 / 255) * 1000 with the clamp (the float32 product of two float32 is exact in float64)"""
    codes = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    depth = np.zeros((1, 20, 20), np.uint8)
    depth[:, 2:-2, 2:-2] = codes
    image = np.repeat(depth[..., None], 3, axis=3)
    out = ni.train_transform(torch.from_numpy(image).to(dev), torch.from_numpy(depth).to(dev), crop=2, image_size=(16, 16), depth_size=(16, 16),
                             disparity=True, keep_u8=True)
    assert np.array_equal(out["depth_u8"].cpu().numpy(), codes)
    q = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    want = np.clip((q.astype(np.float64) * 1000.0).astype(np.float32), np.float32(10), np.float32(1000))
    got = out["depth"].cpu().numpy().ravel()
    assert np.array_equal(got, want), describe(got, want)
    assert np.array_equal(out["image"].cpu().numpy()[0, 1].ravel(), q)
    disp = (np.float64(10.0) / want.astype(np.float64)).astype(np.float32)           # a correctly rounded division
    assert np.array_equal(out["disp_gt"].cpu().numpy().ravel(), disp)


def raw_call(c, dev):
    """the C entry point on outputs prefilled with -1 (float32) / 77 (uint8)"""
    l = _lib.lib()
    image, depth = torch.from_numpy(c["image"]).to(dev), torch.from_numpy(c["depth"]).to(dev)
    B, H0, W0 = depth.shape
    (ih, iw), (dh, dw) = c["image_size"], c["depth_size"]
    a = aug_of(c, dev)
    tables = ni.resample.device_tables("nyu_inputs", (H0, W0, c["crop"], ih, iw, dh, dw), dev)
    assert tables.numel() == l.wmd_nyu_inputs_table_ints(H0, W0, c["crop"], ih, iw, dh, dw)
    out_i, out_d = torch.full((B, 3, ih, iw), -1.0, device=dev), torch.full((B, 1, dh, dw), -1.0, device=dev)
    disp = torch.full((B, 1, dh, dw), -1.0, device=dev)
    u8_i, u8_d = torch.full((B, ih, iw, 3), 77, dtype=torch.uint8, device=dev), torch.full((B, dh, dw), 77, dtype=torch.uint8, device=dev)
    _lib.check(l.wmd_nyu_inputs(_lib.ptr(image), _lib.ptr(depth), B, H0, W0, c["crop"], ih, iw, dh, dw, _lib.ptr(a.flip), _lib.ptr(a.perm),
                                _lib.ptr(a.lut), _lib.ptr(tables), tables.numel(), _lib.ptr(out_i), _lib.ptr(out_d), _lib.ptr(disp),
                                _lib.ptr(u8_i), _lib.ptr(u8_d), _lib.current_stream()), "wmd_nyu_inputs")
    return dict(image=out_i.cpu().numpy(), depth=out_d.cpu().numpy(), disp_gt=disp.cpu().numpy(), image_u8=u8_i.cpu().numpy(),
                depth_u8=u8_d.cpu().numpy())


def test_raw_call_writes_every_output_and_repeats_bit_for_bit(dev):
    c = cases.build("tiles_61x161")
    a, b = raw_call(c, dev), raw_call(c, dev)
    for k in ("image", "depth", "disp_gt"):
        assert not (a[k] == -1).any(), k                                             # every valid value is >= 0
    check(a, *oracle("tiles_61x161"))
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    n_tables = len(ni.resample.DEVICE_TABLES)
    got = run(c, dev, disparity=True)
    assert len(ni.resample.DEVICE_TABLES) == n_tables                                               # the uploaded tables are memoised per shape
    for k in a:
        assert np.array_equal(a[k], got[k]), k


def test_depth_feeds_the_dwt_without_conversion(dev):
    c = cases.build("tiles_61x161")
    out = ni.train_transform(torch.from_numpy(c["image"]).to(dev), torch.from_numpy(c["depth"]).to(dev), aug_of(c, dev), crop=c["crop"],
                             image_size=(64, 96), depth_size=(32, 48), disparity=True)
    assert out["disp_gt"].shape == (7, 1, 32, 48) and out["disp_gt"].is_contiguous() and out["disp_gt"].dtype == torch.float32
    yl, yh = wavelets.DWT(J=4).to(dev)(out["disp_gt"])
    assert yl.shape == (7, 1, 2, 3) and len(yh) == 4 and bool(torch.isfinite(yl).all())
    # the Haar low-pass of four levels is 16 x the mean of each 16 x 16 block
    want = out["disp_gt"].double().reshape(7, 1, 2, 16, 3, 16).mean(dim=(3, 5)) * 16
    assert torch.allclose(yl.double(), want, rtol=1e-5, atol=0)


def test_device_side_refusals(dev):
    image, depth = torch.zeros(2, 20, 24, 3, dtype=torch.uint8, device=dev), torch.zeros(2, 20, 24, dtype=torch.uint8, device=dev)
    kw = dict(crop=2, image_size=(8, 8), depth_size=(4, 4))
    assert ni.train_transform(image, depth, **kw)["image"].shape == (2, 3, 8, 8)
    with pytest.raises(_lib.WmdError, match="GPU only"):
        ni.train_transform(image.cpu(), depth, **kw)
    with pytest.raises(_lib.WmdError, match="GPU only"):
        ni.train_transform(image, depth.cpu(), **kw)
    with pytest.raises(_lib.WmdError, match="uint8"):
        ni.train_transform(image.float(), depth, **kw)
    with pytest.raises(_lib.WmdError, match="16-bit"):
        ni.train_transform(image, depth.to(torch.int16), **kw)                       # the test PNGs of is_test=True
    with pytest.raises(_lib.WmdError, match="crop"):
        ni.train_transform(image, depth, crop=10, image_size=(8, 8), depth_size=(4, 4))
    with pytest.raises(_lib.WmdError):
        ni.train_transform(image, depth[:, :19], **kw)
    with pytest.raises(_lib.WmdError):
        ni.train_transform(image, depth[:1], **kw)
    with pytest.raises(_lib.WmdError, match="items"):
        ni.train_transform(image, depth, ni.Augmentation([0, 1, 0], [0, 0, 0]).to(dev), **kw)
    with pytest.raises(_lib.WmdError):
        ni.train_transform(image, depth, ni.Augmentation([0, 1], [0, 0]), **kw)      # on the host
    with pytest.raises(_lib.WmdError):
        ni.train_transform(image, depth, image_size=(0, 8), depth_size=(4, 4), crop=2)
