"""GPU: the semi-global matcher (csrc/wmd_stereo.hip through wavelet_monodepth_amd.stereo) against the numpy oracle
(tests/stereo_ref.py).  Everything is integer arithmetic, so every comparison is equality of bits: the int16 maps, and the
uint16 cost volume and summed path costs where a case asks for them.  The oracle runs once per case and is shared."""
import numpy as np
import pytest
import torch

import stereo_cases
import stereo_ref as R
from wavelet_monodepth_amd import _lib, depth_hints as dh, stereo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def gpu_settings(s):
    return stereo.SGBMSettings(**s._asdict())


_ORACLE = {}


def oracle(name, seed=0, reverse=False):
    key = (name, seed, reverse)
    if key not in _ORACLE:
        left, right = stereo_cases.sgbm_inputs(name, seed)
        _ORACLE[key] = (left, right, R.sgbm(left, right, stereo_cases.settings(name), reverse=reverse))
    return _ORACLE[key]


def dev_pair(left, right, dev):
    return torch.from_numpy(left[None].copy()).to(dev), torch.from_numpy(right[None].copy()).to(dev)


@pytest.mark.parametrize("name", list(stereo_cases.SGBM_CASES))
def test_map_and_volumes_equal_the_oracle(dev, name):
    left, right, want = oracle(name)
    s = stereo_cases.settings(name)
    l, r = dev_pair(left, right, dev)
    disp, cost, S = stereo.sgbm(l, r, gpu_settings(s), return_volumes=True)
    assert disp.dtype == torch.int16 and tuple(disp.shape) == (1,) + left.shape[:2]
    cost, S, disp = cost[0].cpu().numpy(), S[0].cpu().numpy(), disp[0].cpu().numpy()
    valid = want["disp"] != (s.minDisparity - 1) * 16
    print(name, "valid %.1f %% of the map, %d of them removed as speckles, max S %d of %d" % (
        100 * valid.mean(), int((want["raw"] != want["disp"]).sum()), int(want["S"].max()), R.s_bound(s, left.shape[2])))
    assert np.array_equal(cost, want["cost"]), "cost volume: %d of %d differ" % ((cost != want["cost"]).sum(), cost.size)
    assert np.array_equal(S, want["S"]), "S: %d of %d differ" % ((S != want["S"]).sum(), S.size)
    assert np.array_equal(disp, want["disp"]), "map: %d of %d differ" % ((disp != want["disp"]).sum(), disp.size)
    # the map before the speckle stage (small maps lose everything to a 100-pixel window), without the volumes: the
    # workspace's own, at another stride
    raw = stereo.sgbm(l, r, gpu_settings(s._replace(speckleWindowSize=0)))[0].cpu().numpy()
    assert np.array_equal(raw, want["raw"]), "map before speckles: %d of %d differ" % ((raw != want["raw"]).sum(), raw.size)


def test_batch_with_reverse_flags(dev):
    """B = 3, reverse = [0, 1, 0]: every image equals its own oracle call; the middle pair is a right-view base"""
    name = "base_20x72_d16_b3_5"
    s = stereo_cases.settings(name)
    pairs, wants = [], []
    for b, rev in enumerate((False, True, False)):
        left, right = stereo_cases.sgbm_inputs(name, seed=b)
        if rev:
            left, right = right, left
        pairs.append((left, right))
        wants.append(R.sgbm(left, right, s, reverse=rev)["disp"])
    l = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev)
    r = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
    got = stereo.sgbm(l, r, gpu_settings(s), reverse=[0, 1, 0]).cpu().numpy()
    for b in range(3):
        assert np.array_equal(got[b], wants[b]), "image %d: %d pixels differ" % (b, (got[b] != wants[b]).sum())
    assert (got[1][:, -16:] == -16).all() and (got[0][:, :16] == -16).all()
    assert (got[1][:, :-16] != -16).mean() > 0.9
    flags = torch.tensor([0, 1, 0], dtype=torch.uint8, device=dev)
    assert torch.equal(stereo.sgbm(l, r, gpu_settings(s), reverse=flags).cpu(), torch.from_numpy(np.stack(wants)))


def test_single_channel_3d_input(dev):
    left, right, want = oracle("eight_columns_7x40_c1_d32")
    s = stereo_cases.settings("eight_columns_7x40_c1_d32")
    l, r = dev_pair(left[:, :, 0], right[:, :, 0], dev)
    assert np.array_equal(stereo.sgbm(l, r, gpu_settings(s))[0].cpu().numpy(), want["disp"])


@pytest.mark.parametrize("name", ["ragged_9x200_d160", "base_20x72_d16_b1_8"])
def test_poisoned_workspace_gives_the_same_bytes(dev, name):
    """the entry itself, with a workspace the test owns: filled with 0xA5, then with 0x5A, the map is the oracle's both times"""
    left, right, want = oracle(name)
    s = stereo_cases.settings(name)
    l, r = dev_pair(left, right, dev)
    H, W, C = left.shape
    lib = _lib.lib()
    n = lib.wmd_stereo_sgbm_workspace_bytes(1, H, W, C, s.minDisparity, s.numDisparities, s.blockSize)
    assert n > 0
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0
    for fill in (0xA5, 0x5A):
        ws.fill_(fill)
        disp = torch.full((1, H, W), 0x7A7A, dtype=torch.int16, device=dev)
        _lib.check(lib.wmd_stereo_sgbm(_lib.ptr(l), _lib.ptr(r), None, _lib.ptr(disp), None, None, 1, H, W, C, s.minDisparity, s.numDisparities,
                                       s.blockSize, s.P1, s.P2, s.preFilterCap, s.uniquenessRatio, s.speckleWindowSize, s.speckleRange,
                                       s.disp12MaxDiff, s.directions, _lib.ptr(ws), n, _lib.current_stream()), "wmd_stereo_sgbm")
        assert np.array_equal(disp[0].cpu().numpy(), want["disp"]), "fill %#x" % fill


@pytest.mark.parametrize("name", stereo_cases.SPECKLE_CASES)
def test_filter_speckles_equals_the_oracle(dev, name):
    case = stereo_cases.speckle_case(name)
    want = R.filter_speckles(case["disp"].astype(np.int64), case["invalid"], case["max_size"], case["max_diff"]).astype(np.int16)
    src = torch.from_numpy(case["disp"]).to(dev)
    got = stereo.filter_speckles(src, case["invalid"], case["max_size"], case["max_diff"])
    assert torch.equal(src.cpu(), torch.from_numpy(case["disp"]))          # a copy: the input is untouched
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(got.cpu().numpy() != case["invalid"], case["kept"])


def test_filter_speckles_batch_keeps_images_apart(dev):
    """two maps whose blobs would join across the image border if the batch were one tall map"""
    disp = np.full((2, 6, 9), -16, dtype=np.int16)
    disp[0, 4:6, 2:5] = 64       # 6 pixels at the bottom of image 0
    disp[1, 0:2, 2:5] = 64       # 6 pixels at the top of image 1
    got = stereo.filter_speckles(torch.from_numpy(disp).to(dev), -16, 6, 16).cpu().numpy()
    assert (got == -16).all()
    got = stereo.filter_speckles(torch.from_numpy(disp).to(dev), -16, 5, 16).cpu().numpy()
    assert np.array_equal(got, disp)


def hint_settings():
    return [stereo.SGBMSettings(**R.reference_like(16, b, directions=d)._asdict()) for b, d in ((1, 5), (2, 5), (3, 5), (3, 8))]


@pytest.mark.parametrize("base_is_right", [False, True])
def test_precompute_depth_hints_end_to_end(dev, base_is_right):
    """candidates from the matcher, then fusion: equal to fuse_depth_hints fed the oracle's candidates, in index and depth, bit
    for bit; no hint on the band that has no disparity"""
    left, right, _ = R.synthetic_pair()
    base, lookup = (right, left) if base_is_right else (left, right)
    H, W, _ = base.shape
    ss = hint_settings()
    want = np.stack([R.sgbm(base, lookup, s, reverse=base_is_right)["disp"] for s in ss]).astype(np.float32) / 16
    b, l = dev_pair(base, lookup, dev)
    cand = stereo.depth_hint_candidates(b, l, base_is_right, ss)
    assert cand.dtype == torch.float32 and tuple(cand.shape) == (1, 4, H, W)
    assert np.array_equal(cand[0].cpu().numpy(), want)
    assert torch.equal(cand[0, 1], cand[0, 2])                  # blockSize 2 and 3: the same window
    K = np.array([[0.58 * W, 0, 0.5 * W, 0], [0, 1.92 * H, 0.5 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
    Kt = torch.from_numpy(K)[None].to(dev)
    iKt = torch.from_numpy(np.linalg.pinv(K).astype(np.float32))[None].to(dev)
    T = torch.eye(4)[None].clone()
    T[0, 0, 3] = 0.1 if base_is_right else -0.1
    fbl = float(np.float32(K[0, 0]) * np.float32(0.1))
    img = lambda a: (torch.from_numpy(a.copy()).permute(2, 0, 1).float() / 255)[None].contiguous().to(dev)
    depth, index = dh.fuse_depth_hints(torch.from_numpy(want)[None].to(dev), img(base), img(lookup), Kt, iKt, T.to(dev), disparities=True,
                                       focal_times_baseline=fbl)
    out = stereo.precompute_depth_hints(b, l, base_is_right, Kt, iKt, settings=ss)
    assert set(out) == {"depth_hint", "depth_hint_mask"}
    assert torch.equal(out["depth_hint"].view(torch.int32), depth.view(torch.int32))
    _, index2 = dh.fuse_depth_hints(cand, img(base), img(lookup), Kt, iKt, T.to(dev), disparities=True, focal_times_baseline=fbl)
    assert torch.equal(index2, index)
    band = out["depth_hint_mask"][..., -16:] if base_is_right else out["depth_hint_mask"][..., :16]
    assert not band.any() and out["depth_hint_mask"].mean() > 0.6      # the valid rectangle is 56 / 72 of the map
