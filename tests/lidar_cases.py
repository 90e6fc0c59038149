"""Named, seeded velodyne cases for the LiDAR depth-map tests.  numpy only; shared by tests/golden/make_golden_lidar.py (which
runs the reference on them) and the tests (which regenerate them).

    build(name) -> {"name", "shape": (H, W), "points": [N,4] float32 as in the .bin (4th column: a reflectance),
                    "cam2cam": {"S_rect_02", "R_rect_00", "P_rect_02"}, "velo2cam": {"R", "T"}, "P": P_velo2im float64 [3,4]}
    write_calib(case, directory), write_scan(case, path): the files the reference reads.

EXACT cases: focal 4, identity R_rect, the axis-swap velodyne rotation (camera x = -y, y = -z, z = x), T = (0, 0, -0.25), a
principal point at half-integers (an integer cx for a single column), y and z on a 1/16 grid and x from {0, 1/8, 1/4, 1/2, 1, 2, 4, 8, -1}: every product and sum
of the projection is exact in float64, so the order of a BLAS summation cannot matter.  p_2 = x - 1/4 is -1/4 and -1/8 (in
bounds with a negative depth), 0 (inf or NaN), 1/4 or larger; with |p_2| <= 1/4 both quotients land on .5 exactly (rounding
ties).  y and z are drawn so that the projection covers the image and a margin of 0.75 pixels around it whatever p_2 is.
"""
import os

import numpy as np

EXACT = {"exact_6x4": (6, 4, 400, 11), "exact_9x16": (9, 16, 2000, 12), "exact_5x1": (5, 1, 200, 13), "exact_4x2": (4, 2, 200, 14),
         "exact_5x3": (5, 3, 200, 15)}
SPECIAL = "special_6x8"
DEGENERATE = ("n0", "n1")
GENERAL = "general_37x124"
FULL = "full_375x1242"
RAGGED = tuple("ragged_%d" % i for i in range(5))            # one batch: N = 0, 1, 255, 256, 1025 at 8 x 12, five matrices
RAGGED_N = (0, 1, 255, 256, 1025)
EXACT_CLASS = tuple(EXACT) + (SPECIAL,) + DEGENERATE         # the oracle equals the reference in float64
GENERAL_CLASS = (GENERAL,) + RAGGED                          # ... up to the BLAS order in camera mode
CASES = EXACT_CLASS + GENERAL_CLASS + (FULL,)

XS = np.array([0, 0.125, 0.25, 0.5, 1, 2, 4, 8, -1], np.float32)
AXIS_SWAP = np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]])


def chain(cam2cam, velo2cam, cam=2):
    """kitti_utils.py:56-68 in numpy"""
    rigid = np.vstack((np.hstack((velo2cam["R"].reshape(3, 3), velo2cam["T"][..., np.newaxis])), np.array([0, 0, 0, 1.0])))
    R4 = np.eye(4)
    R4[:3, :3] = cam2cam["R_rect_00"].reshape(3, 3)
    return np.dot(np.dot(cam2cam["P_rect_0%d" % cam].reshape(3, 4), R4), rigid)


def _case(name, H, W, points, P_rect, R_rect, R, T):
    cam2cam = {"S_rect_02": np.array([float(W), float(H)]), "R_rect_00": np.asarray(R_rect, np.float64).reshape(9),
               "P_rect_02": np.asarray(P_rect, np.float64).reshape(12)}
    velo2cam = {"R": np.asarray(R, np.float64).reshape(9), "T": np.asarray(T, np.float64).reshape(3)}
    return {"name": name, "shape": (H, W), "points": np.ascontiguousarray(points, np.float32), "cam2cam": cam2cam,
            "velo2cam": velo2cam, "P": chain(cam2cam, velo2cam)}


def _exact_points(H, W, n, rng):
    cx, cy = (W // 2 + 0.5 if W > 1 else 1.0), H // 2 + 0.5   # W = 1: 0.5 rounds to 0 and 1.5 to 2, a tie in u never lands
    x = XS[rng.integers(0, len(XS), n)]
    p2 = x.astype(np.float64) - 0.25
    free = (p2 == 0) | (x < 0)                                # no projection to aim: any y, z
    qu, qv = rng.uniform(-0.25, W + 1.25, n), rng.uniform(-0.25, H + 1.25, n)   # p_0 / p_2, p_1 / p_2: in bounds from 0.5 to W + 0.5
    y = np.where(free, rng.uniform(-1, 1, n), (cx - qu) * p2 / 4)
    z = np.where(free, rng.uniform(-1, 1, n), (cy - qv) * p2 / 4)
    pts = np.stack([x, np.round(y * 16) / 16, np.round(z * 16) / 16, rng.uniform(0, 1, n)], 1).astype(np.float32)
    return pts, [[4.0, 0, cx, 0], [0, 4.0, cy, 0], [0, 0, 1, 0]]


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ \
        np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])


def _kitti_like(H, W, rng, jitter=1.0):
    """a calibration of the KITTI kind scaled to H x W: focal 0.58 W, a stereo offset in P_rect, small rotations"""
    f = 0.581 * W * (1 + 0.01 * jitter * rng.standard_normal())
    P_rect = [[f, 0, 0.4908 * W + jitter * rng.standard_normal(), 0.0361 * W], [0, f, 0.4609 * H + jitter * rng.standard_normal(), 0.2161],
              [0, 0, 1, 0.002746]]
    R_rect = _rot(*(0.01 * rng.standard_normal(3)))
    R = _rot(*(0.015 * rng.standard_normal(3))) @ AXIS_SWAP
    T = np.array([-0.004, -0.0763, -0.2718]) + 0.01 * jitter * rng.standard_normal(3)
    return P_rect, R_rect, R, T


def _cloud(n, rng):
    """points in front of and beside the car: range 2 .. 80 m, +-70 degrees of azimuth, -25 .. +4 degrees of elevation;
    a twentieth of them behind it"""
    r, az, el = rng.uniform(2, 80, n) ** rng.uniform(0.5, 1, n), np.radians(rng.uniform(-70, 70, n)), np.radians(rng.uniform(-25, 4, n))
    x = r * np.cos(el) * np.cos(az) * np.where(rng.uniform(0, 1, n) < 0.05, -1, 1)
    return np.stack([x, r * np.cos(el) * np.sin(az), r * np.sin(el), rng.uniform(0, 1, n)], 1).astype(np.float32)


def _rings(rng):
    """64 rings x 1875 azimuth steps = 120 000 returns of a flat road 1.73 m below the sensor between two walls, a range
    noise of 2 cm; rows ordered by azimuth step, then ring, as a spinning sensor writes them"""
    az = np.repeat(np.radians(np.arange(1875) * (360.0 / 1875)), 64)
    el = np.tile(np.radians(np.linspace(2.0, -24.8, 64)), 1875)
    dx, dy, dz = np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)
    with np.errstate(divide="ignore", invalid="ignore"):
        ground = np.where(dz < 0, -1.73 / dz, np.inf)
        walls = np.where(dy > 0, 7.0 / dy, np.where(dy < 0, -9.0 / dy, np.inf))
        front = np.where(np.abs(dx) > 1e-9, 45.0 / np.abs(dx), np.inf)
    r = np.minimum(np.minimum(ground, walls), np.minimum(front, 120.0)) + 0.02 * rng.standard_normal(az.size)
    return np.stack([r * dx, r * dy, r * dz, rng.uniform(0, 1, az.size)], 1).astype(np.float32)


def build(name):
    if name in EXACT:
        H, W, n, seed = EXACT[name]
        pts, P_rect = _exact_points(H, W, n, np.random.default_rng(seed))
        return _case(name, H, W, pts, P_rect, np.eye(3), AXIS_SWAP, [0, 0, -0.25])
    if name == SPECIAL:
        rng = np.random.default_rng(21)
        pts, P_rect = _exact_points(6, 8, 300, rng)
        planted = [np.nan, np.inf, -np.inf, -0.0]
        for k, i in enumerate(rng.permutation(300)[:36]):       # every value in every coordinate, three times
            pts[i, k % 3] = planted[(k // 3) % 4]
        return _case(name, 6, 8, pts, P_rect, np.eye(3), AXIS_SWAP, [0, 0, -0.25])
    if name in DEGENERATE:
        pts = np.zeros((0, 4), np.float32) if name == "n0" else np.array([[1.0, -0.1875, 0.0625, 0.5]], np.float32)
        return _case(name, 6, 8, pts, [[4.0, 0, 4.5, 0], [0, 4.0, 3.5, 0], [0, 0, 1, 0]], np.eye(3), AXIS_SWAP, [0, 0, -0.25])
    if name == GENERAL:
        rng = np.random.default_rng(31)
        return _case(name, 37, 124, _cloud(20000, rng), *_kitti_like(37, 124, rng))
    if name == FULL:
        rng = np.random.default_rng(41)
        return _case(name, 375, 1242, _rings(rng), *_kitti_like(375, 1242, rng))
    if name in RAGGED:
        i = RAGGED.index(name)
        rng = np.random.default_rng(50 + i)
        return _case(name, 8, 12, _cloud(RAGGED_N[i], rng), *_kitti_like(8, 12, rng, jitter=0.3))
    raise KeyError(name)


def _numbers(a):
    return " ".join("%.17e" % v for v in np.asarray(a, np.float64).ravel())   # 18 digits: float() returns the same bits


def write_calib(case, directory):
    """calib_cam_to_cam.txt and calib_velo_to_cam.txt with the keys the reference reads, and a date line that stays text"""
    with open(os.path.join(directory, "calib_cam_to_cam.txt"), "w") as f:
        f.write("calib_time: 09-Jan-2012 13:57:47\ncorner_dist: 9.950000e-02\n")
        for key in ("S_rect_02", "R_rect_00", "P_rect_02"):
            f.write("%s: %s\n" % (key, _numbers(case["cam2cam"][key])))
    with open(os.path.join(directory, "calib_velo_to_cam.txt"), "w") as f:
        f.write("calib_time: 15-Mar-2012 11:37:16\n")
        for key in ("R", "T"):
            f.write("%s: %s\n" % (key, _numbers(case["velo2cam"][key])))
        f.write("delta_f: 0.000000e+00 0.000000e+00\n")


def write_scan(case, path):
    case["points"].tofile(path)
