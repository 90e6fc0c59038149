"""GPU: the LiDAR depth maps (csrc/wmd_lidar.hip through kitti_utils.project_lidar) against the float64 numpy oracle
(tests/lidar_ref.py, rounded to float32 once) and the reference's own generate_depth_map (tests/golden/lidar_reference.npz).

Against the oracle every comparison is exact (== on float32, so -0.0 equals 0.0): the kernel evaluates the same seven
float64 operations per row without contraction, the same IEEE division and rint, and resolves the ordering rules with integer
atomics.  Against the reference it is exact wherever the arithmetic is (the exact, special and degenerate cases, and
vel_depth=True everywhere); with a general calibration the reference's BLAS sums the projection in another order, a
difference in the last float64 bits that the rounding to float32 turns into at most one float32 ulp, on the same support.
Reads the fixture only; every case runs the kernel once per mode and the checks share the result."""
import numpy as np
import pytest
import torch

import lidar_cases
import lidar_ref
from util import load_golden
from wavelet_monodepth_amd import _lib, evaluation, kitti_utils as ku

pytestmark = pytest.mark.gpu
MODES = (("cam", False), ("vel", True))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return load_golden("lidar_reference.npz")


def on(case, dev):
    return torch.from_numpy(case["points"]).to(dev), torch.from_numpy(case["P"]).to(dev)


@pytest.fixture(scope="module")
def results(dev):
    """name -> (case, {mode: kernel map as numpy}); computed once, read only"""
    memo = {}

    def get(name):
        if name not in memo:
            case = lidar_cases.build(name)
            pts, P = on(case, dev)
            memo[name] = (case, {mode: ku.project_lidar(pts, P, case["shape"], vel_depth=vel).cpu().numpy() for mode, vel in MODES})
        return memo[name]
    return get


def reference(gold, name, mode, shape):
    if name != lidar_cases.FULL:
        return gold["%s|%s" % (name, mode)].astype(np.float32)
    flat = np.zeros(shape[0] * shape[1], np.float32)
    flat[gold["%s|%s|index" % (name, mode)]] = gold["%s|%s|value" % (name, mode)]
    return flat.reshape(shape)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def packed(names, dev):
    cases = [lidar_cases.build(n) for n in names]
    offsets = np.concatenate(([0], np.cumsum([len(c["points"]) for c in cases]))).astype(np.int64)
    return (cases, torch.from_numpy(np.concatenate([c["points"] for c in cases])).to(dev), torch.from_numpy(np.stack([c["P"] for c in cases])).to(dev),
            torch.from_numpy(offsets).to(dev))


@pytest.mark.parametrize("name", lidar_cases.CASES)
def test_kernel_equals_the_float64_oracle(results, name):
    case, out = results(name)
    for mode, vel in MODES:
        want = lidar_ref.depth_map(case["points"], case["P"], case["shape"], vel).astype(np.float32)
        assert out[mode].shape == case["shape"] and out[mode].dtype == np.float32
        wrong = int((out[mode] != want).sum())
        print(name, mode, "pixels that differ from the oracle:", wrong, "of", want.size, "non-zero", int((want != 0).sum()))
        assert wrong == 0


@pytest.mark.parametrize("name", lidar_cases.CASES)
def test_kernel_against_the_reference(results, gold, name):
    case, out = results(name)
    ref = {mode: reference(gold, name, mode, case["shape"]) for mode, _ in MODES}
    assert np.array_equal(out["vel"], ref["vel"])
    assert np.array_equal(out["cam"] != 0, ref["cam"] != 0)
    if name in lidar_cases.EXACT_CLASS:
        assert np.array_equal(out["cam"], ref["cam"])
    else:   # positive finite float32 numbers: their bit patterns are one apart per ulp
        ulp = np.abs(bits(out["cam"]).astype(np.int64) - bits(ref["cam"]).astype(np.int64))[ref["cam"] != 0]
        print(name, "camera depth: %d of %d values one float32 ulp from the reference" % (int((ulp != 0).sum()), ulp.size))
        assert ulp.size == 0 or ulp.max() <= 1


def test_batched_call_equals_the_per_scan_calls(results, dev):
    """five scans with N = 0, 1, 255, 256, 1025 and five matrices in one call; then scans of two other cases that share a size"""
    for names in (lidar_cases.RAGGED, (lidar_cases.SPECIAL, "n1", "n0", lidar_cases.SPECIAL)):
        cases, pts, P, offsets = packed(names, dev)
        for mode, vel in MODES:
            batch = ku.project_lidar(pts, P, cases[0]["shape"], vel_depth=vel, offsets=offsets).cpu().numpy()
            assert batch.shape == (len(names),) + cases[0]["shape"]
            for b, n in enumerate(names):
                assert np.array_equal(bits(batch[b]), bits(results(n)[1][mode])), (n, mode)


@pytest.mark.parametrize("name", ["exact_9x16", lidar_cases.GENERAL, lidar_cases.FULL])
def test_two_runs_give_the_same_bits(results, dev, name):
    case, out = results(name)
    pts, P = on(case, dev)
    for mode, vel in MODES:
        again = ku.project_lidar(pts, P, case["shape"], vel_depth=vel).cpu().numpy()
        assert np.array_equal(bits(again), bits(out[mode]))


def raw_call(pts, P, offsets, shape, vel, ws, depth):
    l = _lib.lib()
    B, (H, W) = offsets.numel() - 1, shape
    _lib.check(l.wmd_lidar_depth_maps(_lib.ptr(pts), _lib.ptr(offsets), _lib.ptr(P), pts.shape[0], B, H, W, int(vel), _lib.ptr(depth), _lib.ptr(ws),
                                      ws.numel() * 8, _lib.current_stream()), "wmd_lidar_depth_maps")


def test_poisoned_workspace_and_output_change_nothing(results, dev):
    """the call initialises what it reads: a workspace and an output pre-filled with 0xFF bytes (and with 0x00, and with the
    words a previous call left) give the bits of a fresh call"""
    l = _lib.lib()
    cases, pts, P, offsets = packed(lidar_cases.RAGGED, dev)
    H, W = cases[0]["shape"]
    n = l.wmd_lidar_depth_workspace_bytes(len(cases), H, W)
    assert n > 0 and n % 8 == 0
    ws = torch.empty(n // 8, device=dev, dtype=torch.int64)
    depth = torch.empty((len(cases), H, W), device=dev, dtype=torch.float32)
    for fill in (-1, 0, None, -1):          # None: what the previous call left
        for mode, vel in MODES:
            if fill is not None:
                ws.fill_(fill)
                depth.view(torch.int32).fill_(-1)
            raw_call(pts, P, offsets, (H, W), vel, ws, depth)
            got = depth.cpu().numpy()
            for b, name in enumerate(lidar_cases.RAGGED):
                assert np.array_equal(bits(got[b]), bits(results(name)[1][mode])), (fill, name, mode)


def test_non_default_stream(results, dev):
    case, out = results(lidar_cases.GENERAL)
    pts, P = on(case, dev)
    stream = torch.cuda.Stream(device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got = ku.project_lidar(pts, P, case["shape"], vel_depth=False)
    stream.synchronize()
    assert np.array_equal(bits(got.cpu().numpy()), bits(out["cam"]))


@pytest.mark.parametrize("name", ["exact_6x4", lidar_cases.SPECIAL, lidar_cases.GENERAL])
def test_generate_depth_map_from_files(tmp_path, gold, dev, name):
    case = lidar_cases.build(name)
    lidar_cases.write_calib(case, str(tmp_path))
    scan = str(tmp_path / "0000000000.bin")
    lidar_cases.write_scan(case, scan)
    vel = ku.generate_depth_map(str(tmp_path), scan, 2, True)
    assert vel.is_cuda and vel.dtype == torch.float32 and tuple(vel.shape) == case["shape"]
    assert np.array_equal(vel.cpu().numpy(), reference(gold, name, "vel", case["shape"]))
    both = ku.generate_depth_maps(str(tmp_path), [scan, scan], cam=2, vel_depth=False)
    assert tuple(both.shape) == (2,) + case["shape"] and torch.equal(both[0], both[1])
    cam, ref = both[0].cpu().numpy(), reference(gold, name, "cam", case["shape"])
    assert np.array_equal(cam != 0, ref != 0)
    if name in lidar_cases.EXACT_CLASS:
        assert np.array_equal(cam, ref)
    else:
        assert np.abs(bits(cam).astype(np.int64) - bits(ref).astype(np.int64))[ref != 0].max() <= 1


def test_kitti_metrics_take_the_kernel_map(results, gold, dev):
    """export_gt_depth.py stores the vel_depth=True maps and evaluate_depth.py reads them: the metrics of a synthetic
    prediction against the kernel's map are those against the reference's map, bit for bit"""
    case, out = results(lidar_cases.FULL)
    H, W = case["shape"]
    ref = reference(gold, lidar_cases.FULL, "vel", case["shape"])
    yy, xx = np.mgrid[0:96, 0:320].astype(np.float32)
    disp = torch.from_numpy((0.05 + 0.4 * yy / 96 + 0.02 * np.sin(xx / 17))[None]).to(dev)
    pts, P = on(case, dev)
    got = evaluation.kitti_metrics(disp, ku.project_lidar(pts, P[None], (H, W), True, torch.tensor([0, len(pts)], device=dev)))
    want = evaluation.kitti_metrics(disp, torch.from_numpy(ref)[None].to(dev))
    assert int(got[2][0]) == int(want[2][0]) > 1000                  # valid ground-truth pixels inside the Eigen crop
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.isfinite(got[0]).all()
