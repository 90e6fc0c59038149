"""CPU: wmd_lidar_depth_maps refuses what it must before any HIP call (dummy non-null pointers never reach a kernel),
the workspace query answers 0 for a shape the call refuses, project_lidar refuses CPU tensors, and the host half of
kitti_utils -- read_calib_file, load_velodyne_points, velo_to_image_matrix -- reads written files back bit for bit."""
import numpy as np
import pytest
import torch

import lidar_cases
from wavelet_monodepth_amd import _lib, kitti_utils as ku

ALIGNED = 4096   # a dummy pointer that passes the alignment checks


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def call(lib, points=ALIGNED, offsets=ALIGNED, P=ALIGNED, total=1000, B=2, H=6, W=8, vel=0, depth=ALIGNED, ws=ALIGNED, n=None):
    if n is None:
        n = lib.wmd_lidar_depth_workspace_bytes(B, H, W)
    return lib.wmd_lidar_depth_maps(points, offsets, P, total, B, H, W, vel, depth, ws, n, None)


def test_null_pointers(lib):
    for name in ("points", "offsets", "P", "depth"):
        assert call(lib, **{name: None}) == -1, name
        assert b"null" in lib.wmd_last_error()
    assert call(lib, points=ALIGNED + 4) == -1                       # float4 rows
    assert b"aligned" in lib.wmd_last_error()


def test_bad_shapes(lib):
    for kw in (dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(H=-5), dict(W=-1)):
        assert call(lib, n=1 << 20, **kw) == -2, kw
        assert lib.wmd_lidar_depth_workspace_bytes(kw.get("B", 2), kw.get("H", 6), kw.get("W", 8)) == 0


def test_unsupported_before_any_launch(lib):
    assert lib.wmd_lidar_depth_workspace_bytes(1, 65536, 32768) == 0                 # H W = 2^31
    assert call(lib, B=1, H=65536, W=32768, n=1 << 40) == -3
    assert b"2^31" in lib.wmd_last_error()
    assert lib.wmd_lidar_depth_workspace_bytes(1, 65536, 32767) > 0                  # ... and just below it
    assert call(lib, total=2 ** 31) == -3                                            # bounds every scan's N
    assert call(lib, total=2 ** 31 - 1, ws=None) == -5                               # passes that check, stops at the next


def test_workspace(lib):
    """8 bytes per pixel word, 8 + 4 + 4 per bucket of sub2ind (H (W - 1) + 1 of them), each array padded to 8 bytes"""
    for B, H, W in ((1, 6, 8), (5, 8, 12), (2, 5, 1), (3, 4, 2), (64, 375, 1242)):
        n = lib.wmd_lidar_depth_workspace_bytes(B, H, W)
        nk = B * (H * (W - 1) + 1)
        assert n == 8 * B * H * W + 8 * nk + 2 * 8 * ((nk + 1) // 2)
        assert call(lib, B=B, H=H, W=W, n=n - 1) == -5
        assert b"workspace" in lib.wmd_last_error()
        assert call(lib, B=B, H=H, W=W, ws=None) == -5
        assert call(lib, B=B, H=H, W=W, ws=ALIGNED + 4) == -5


def test_project_lidar_refuses_cpu_tensors_and_bad_layouts():
    pts, P = torch.zeros(10, 4), torch.zeros(3, 4, dtype=torch.float64)
    with pytest.raises(_lib.WmdError):
        ku.project_lidar(pts, P, (6, 8))
    with pytest.raises(_lib.WmdError):
        ku.project_lidar(pts, P[None], (6, 8), offsets=torch.tensor([0, 10]))
    with pytest.raises(_lib.WmdError):
        ku.project_lidar(pts.numpy(), P, (6, 8))


@pytest.mark.parametrize("name", ["exact_6x4", "general_37x124", "ragged_3"])
def test_host_readers_against_the_numpy_chain(tmp_path, name):
    case = lidar_cases.build(name)
    lidar_cases.write_calib(case, str(tmp_path))
    scan = str(tmp_path / "scan.bin")
    lidar_cases.write_scan(case, scan)
    cam2cam = ku.read_calib_file(str(tmp_path / "calib_cam_to_cam.txt"))
    velo2cam = ku.read_calib_file(str(tmp_path / "calib_velo_to_cam.txt"))
    assert cam2cam["calib_time"] == "09-Jan-2012 13:57:47"                           # not a number: stays text
    assert cam2cam["corner_dist"].dtype == np.float64 and cam2cam["corner_dist"].tolist() == [0.0995]
    for key, want in case["cam2cam"].items():
        assert np.array_equal(cam2cam[key], want), key
    for key, want in case["velo2cam"].items():
        assert np.array_equal(velo2cam[key], want), key
    P, shape = ku.velo_to_image_matrix(cam2cam, velo2cam, cam=2)
    assert shape == case["shape"] and P.dtype == np.float64 and P.shape == (3, 4)
    assert np.array_equal(P, lidar_cases.chain(case["cam2cam"], case["velo2cam"]))
    pts = ku.load_velodyne_points(scan)
    assert pts.dtype == np.float32 and pts.shape == case["points"].shape
    assert np.array_equal(pts[:, :3].view(np.uint32), case["points"][:, :3].view(np.uint32)) and (pts[:, 3] == 1).all()


def test_read_calib_file_edge_lines(tmp_path):
    path = tmp_path / "calib.txt"
    path.write_text("A: 1 2  3\nB: 1e-3 -2.5e+00\nC: abc: def\nD: 1-2\n")
    data = ku.read_calib_file(str(path))
    assert data["A"] == "1 2  3"                    # a double blank is no number: the value stays text, as in the reference
    assert data["B"].tolist() == [1e-3, -2.5]
    assert data["C"] == "abc: def" and data["D"] == "1-2"
