"""GPU: kitti_inputs.color_pyramid / color_jitter / preprocess against the fixture that the reference's MonoDataset.preprocess
wrote over Pillow (tests/golden/inputs_reference.npz) and against the numpy oracle (tests/inputs_ref.py).  Exact equality
everywhere: uint8 ==, float32 == against u8 / 255.  The shapes are the smallest at which each failure mode can still occur
(tests/inputs_cases.py); one chain runs at the KITTI training size and one image holds all 2^24 colours."""
import hashlib
import os

import numpy as np
import pytest
import torch

import inputs_cases
import inputs_ref as R
from wavelet_monodepth_amd import _lib, kitti_inputs as ki, photometric as ph

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputs_reference.npz")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def params(j, dev):
    return None if j is None else ki.ColorJitterParams(j["enable"], j["order"], j["factors"], j["hue_shift"]).to(dev)


def run_case(case, dev):
    out = ki.color_pyramid(torch.from_numpy(case["frames"]).to(dev), case["height"], case["width"], case["num_scales"],
                           torch.from_numpy(case["flip"]).to(dev), params(case["jitter"], dev))
    return [tuple(t.cpu().numpy() for t in level) for level in out]


def tensor_of(u8):
    """[N,h,w,3] uint8 -> float32 [N,3,h,w], the oracle's ToTensor"""
    return np.stack([R.to_tensor(img) for img in u8])


def describe(got, want):
    bad = np.argwhere(got != want)
    return "%d of %d values differ, first at %s: got %s, want %s" % (len(bad), want.size, bad[:3].tolist(), [got[tuple(i)] for i in bad[:3]],
                                                                      [want[tuple(i)] for i in bad[:3]])


def check_levels(levels, want_color, want_aug):
    """levels: [(u8, color, aug)] from the device; want_*: per scale uint8 [N,h,w,3]"""
    assert len(levels) == len(want_color)
    for s, (u8, color, aug) in enumerate(levels):
        assert u8.dtype == np.uint8 and color.dtype == np.float32 and aug.dtype == np.float32
        assert u8.shape == want_color[s].shape and color.shape == (u8.shape[0], 3) + u8.shape[1:3] == aug.shape
        assert np.array_equal(u8, want_color[s]), "scale %d, uint8 level: %s" % (s, describe(u8, want_color[s]))
        assert np.array_equal(color, tensor_of(want_color[s])), "scale %d, color" % s
        want = tensor_of(want_aug[s])
        assert np.array_equal(aug, want), "scale %d, color_aug: %s" % (s, describe(aug, want))


@pytest.mark.parametrize("name", inputs_cases.CASES)
def test_cases_equal_the_reference_chain(dev, gold, name):
    """ratio_47x161: non-integer ratios, 483-byte rows, five images with mixed flips, four levels; clip_5x7: both borders clipped
    at once; upscale_10x14; saturate_48x64: clip8 on both sides; same_12x20: the identity; orders_*: every jitter order at
    random and at edge parameters, a disabled item between enabled ones, the k + 0.5 grey mean."""
    case = inputs_cases.build(name)
    S = case["num_scales"]
    check_levels(run_case(case, dev), [gold["%s|color|%d" % (name, s)] for s in range(S)], [gold["%s|aug|%d" % (name, s)] for s in range(S)])


def test_same_size_is_the_identity_and_no_jitter_aliases_color(dev):
    case = inputs_cases.build("same_12x20")
    frames = torch.from_numpy(case["frames"]).to(dev)
    (u8, color, aug), = ki.color_pyramid(frames, 12, 20, 1)
    assert torch.equal(u8, frames) and aug is color
    (flipped, _, _), = ki.color_pyramid(frames, 12, 20, 1, flip=torch.tensor([True, False], device=dev))
    assert torch.equal(flipped[0], frames[0].flip(1)) and torch.equal(flipped[1], frames[1])


@pytest.mark.parametrize("name", ["orders_random", "orders_edges"])
def test_color_jitter_alone(dev, gold, name):
    case = inputs_cases.build(name)
    got = ki.color_jitter(torch.from_numpy(case["frames"]).to(dev), params(case["jitter"], dev)).cpu().numpy()
    want = gold[name + "|aug|0"]
    for i in np.flatnonzero(np.any(got != want, axis=(1, 2, 3))):
        print("item", i, case["jitter"]["order"][i], case["jitter"]["factors"][i], case["jitter"]["hue_shift"][i])
    assert got.dtype == np.uint8 and np.array_equal(got, want), describe(got, want)


def test_to_tensor_all_256_values(dev):
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, axis=3)
    (_, color, _), = ki.color_pyramid(torch.from_numpy(u8).to(dev), 16, 16, 1)
    exact = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)           # a correctly rounded division
    assert np.array_equal(color.cpu().numpy()[0, 1].ravel(), exact)


@pytest.mark.parametrize("shift", [0, 37])
def test_full_colour_cube_hue_only(dev, gold, shift):
    """all 2^24 colours through the hue op (the other factors are 1.0 and change nothing): a fused multiply-add in the HSV
    round trip or a float32 hue sum moves thousands of colours"""
    cube = R.colour_cube()
    j = dict(enable=np.ones(1, np.uint8), order=np.array([[0, 1, 2, 3]], np.uint8), factors=np.ones((1, 3), np.float32),
             hue_shift=np.array([shift], np.int32))
    got = ki.color_jitter(torch.from_numpy(cube[None]).to(dev), params(j, dev))[0].cpu().numpy()
    want = R.hue(cube, shift)
    differ = int((got != want).any(-1).sum())
    print("shift %d: %d of 2^24 colours differ from the oracle" % (shift, differ))
    assert differ == 0, describe(got, want)
    assert hashlib.sha256(got.tobytes()).hexdigest() == str(gold["cube|%d" % shift])     # Pillow's own result


@pytest.fixture(scope="module")
def real_size():
    """N = 3 native KITTI frames -> the oracle's four levels and jittered levels; computed once, read only"""
    n = 3
    frames = inputs_cases.image("real", (n, 375, 1242, 3), 7)
    ramp = (np.add.outer(np.arange(375), np.arange(1242)) // 7 % 256).astype(np.uint8)
    frames[2] = np.stack([ramp, ramp[::-1], ramp[:, ::-1]], axis=-1)                  # one smooth frame beside two of noise
    flip = np.array([1, 0, 1], np.uint8)
    j = inputs_cases.random_jitter("real", n, 5, perms=[PERM([2, 3, 1, 0]), PERM([1, 0, 3, 2]), PERM([3, 0, 2, 1])])
    color = [R.pyramid(frames[i], 192, 640, 4, bool(flip[i])) for i in range(n)]
    aug = [[R.jitter(l, j["order"][i], j["factors"][i], j["hue_shift"][i]) for l in color[i]] for i in range(n)]
    return dict(frames=frames, height=192, width=640, num_scales=4, flip=flip, jitter=j,
                color=[np.stack([color[i][s] for i in range(n)]) for s in range(4)], aug=[np.stack([aug[i][s] for i in range(n)]) for s in range(4)])


def PERM(order):
    return inputs_cases.PERMS.index(order)


def test_real_size_chain(dev, real_size):
    """375 x 1242 -> 192 x 640, 96 x 320, 48 x 160, 24 x 80: 3726-byte rows, many tiles per image, flip and jitter on, contrast
    after saturation and hue (the grey sum runs over the partially jittered level)"""
    levels = run_case(real_size, dev)
    assert [l[0].shape for l in levels] == [(3, 192, 640, 3), (3, 96, 320, 3), (3, 48, 160, 3), (3, 24, 80, 3)]
    check_levels(levels, real_size["color"], real_size["aug"])


def test_preprocess_keys_shapes_and_shared_parameters(dev, gold):
    """B = 2 samples x 3 frames of 47 x 161: the reference's keys and shapes, every frame of a sample under that sample's flip and
    jitter (checked against single-frame color_pyramid calls), and the dictionary feeds the photometric loss as it is"""
    B, H0, W0, h, w = 2, 47, 161, 32, 64
    ids = [0, -1, 1]
    frames = {f: torch.from_numpy(inputs_cases.image("pre%s" % f, (B, H0, W0, 3), 11)).to(dev) for f in ids}
    do_flip = torch.tensor([1, 0], dtype=torch.uint8, device=dev)
    j = inputs_cases.random_jitter("pre", B, 12, enable=[1, 1])
    jit = params(j, dev)
    inputs = ki.preprocess(frames, h, w, range(4), do_flip, jit)
    assert sorted(inputs, key=str) == sorted([(n, f, s) for n in ("color", "color_aug") for f in ids for s in range(4)], key=str)
    for f in ids:
        single = ki.color_pyramid(frames[f], h, w, 4, do_flip, jit)
        for s in range(4):
            for n, k in (("color", 1), ("color_aug", 2)):
                t = inputs[(n, f, s)]
                assert t.shape == (B, 3, h >> s, w >> s) and t.dtype == torch.float32 and t.is_contiguous() and t.device == dev
                assert torch.equal(t, single[s][k]), (n, f, s)
        want = R.jitter(R.pyramid(frames[f][0].cpu().numpy(), h, w, 1, True)[0], j["order"][0], j["factors"][0], j["hue_shift"][0])
        assert np.array_equal(inputs[("color_aug", f, 0)][0].cpu().numpy(), R.to_tensor(want))
    plain = ki.preprocess(frames, h, w, [0, 2])
    assert sorted(plain, key=str) == sorted([(n, f, s) for n in ("color", "color_aug") for f in ids for s in (0, 2)], key=str)
    assert plain[("color_aug", 1, 2)] is plain[("color", 1, 2)]
    # ... and on into generate_images_pred / compute_losses without conversion
    K = np.array([[0.58, 0, 0.5, 0], [0, 1.92, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
    for key, v in ki.scaled_intrinsics(K, h, w, range(4)).items():
        inputs[key] = v.to(dev)[None].repeat(B, 1, 1)
    from util import loss_case
    _, out = loss_case(B=B, H=h, W=w)
    outputs = {k: torch.from_numpy(v).to(dev) for k, v in out.items()}
    opt = ph.LossOptions(height=h, width=w, frame_ids=ids)
    ph.generate_images_pred(inputs, outputs, opt)
    losses = ph.compute_losses(inputs, outputs, opt, tie_break_noise=0.0)
    assert np.isfinite(float(losses["loss"])) and float(losses["loss"]) > 0


def raw_call(case, dev, poison):
    """the C entry point with a workspace of our own, filled with `poison` first"""
    l = _lib.lib()
    frames = torch.from_numpy(case["frames"]).to(dev)
    N, H0, W0 = frames.shape[:3]
    h, w, S = case["height"], case["width"], case["num_scales"]
    n_ws = l.wmd_color_pyramid_workspace_bytes(N, H0, W0, h, w, S)
    assert n_ws == 8 * N * S
    ws = torch.full((n_ws,), poison, dtype=torch.uint8, device=dev)
    pixels = sum(N * (h >> s) * (w >> s) for s in range(S))
    levels = torch.full((pixels * 3,), 77, dtype=torch.uint8, device=dev)
    color, aug = torch.full((pixels * 3,), -1.0, device=dev), torch.full((pixels * 3,), -1.0, device=dev)
    flip, jit = torch.from_numpy(case["flip"]).to(dev), params(case["jitter"], dev)
    tables = ki.resample.device_tables("color_pyramid", (H0, W0, h, w, S), dev)
    _lib.check(l.wmd_color_pyramid(_lib.ptr(frames), N, H0, W0, h, w, S, _lib.ptr(flip), _lib.ptr(jit.enable), _lib.ptr(jit.order),
                                   _lib.ptr(jit.factors), _lib.ptr(jit.hue_shift), _lib.ptr(tables), _lib.ptr(levels), _lib.ptr(color),
                                   _lib.ptr(aug), _lib.ptr(ws), n_ws, _lib.current_stream()), "wmd_color_pyramid")
    return levels.cpu().numpy(), color.cpu().numpy(), aug.cpu().numpy()


def test_bit_stable_on_a_poisoned_workspace(dev):
    """the grey sums are integer atomics and the call clears its own counters: two runs on workspaces full of 0xFF and of 0x5A
    give the bits of the wrapper's run"""
    case = inputs_cases.build("ratio_47x161")
    a, b = raw_call(case, dev, 0xFF), raw_call(case, dev, 0x5A)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    levels = run_case(case, dev)
    assert np.array_equal(a[0], np.concatenate([l[0].ravel() for l in levels]))
    assert np.array_equal(a[2], np.concatenate([l[2].ravel() for l in levels]))
    n_tables = len(ki.resample.DEVICE_TABLES)
    run_case(case, dev)
    assert len(ki.resample.DEVICE_TABLES) == n_tables                          # the uploaded tables are memoised per shape


def test_device_side_refusals(dev):
    frames = torch.zeros(2, 10, 14, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.WmdError, match="empty"):
        ki.color_pyramid(frames, 4, 6, 4)                                            # 4 >> 3 = 0 rows
    with pytest.raises(_lib.WmdError):
        ki.color_pyramid(frames.float(), 4, 6, 1)
    with pytest.raises(_lib.WmdError):
        ki.color_pyramid(frames, 4, 6, 1, flip=torch.zeros(3, dtype=torch.uint8, device=dev))
    j = inputs_cases.random_jitter("refuse", 3, 1)
    with pytest.raises(_lib.WmdError):
        ki.color_pyramid(frames, 4, 6, 1, jitter=params(j, dev))                     # three items for two frames
    with pytest.raises(_lib.WmdError):
        ki.color_jitter(frames, ki.ColorJitterParams(j["enable"][:2], j["order"][:2], j["factors"][:2], j["hue_shift"][:2]))   # on the host
