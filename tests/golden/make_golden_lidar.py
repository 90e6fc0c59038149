"""Golden vectors for the LiDAR depth maps, produced by the REFERENCE's own generate_depth_map (KITTI/kitti_utils.py).

Every case of tests/lidar_cases.py is written as calib_cam_to_cam.txt, calib_velo_to_cam.txt and a velodyne .bin into a
temporary directory, and the reference reads those files in both modes.  kitti_utils.py still says `np.int`, which numpy
dropped in 1.24: the alias is restored in this process only.  Run in the build container only:

    python tests/golden/make_golden_lidar.py        # writes tests/golden/lidar_reference.npz

Stored per case (no inputs: the tests regenerate them from lidar_cases):
    exact, special, degenerate, general and ragged cases:  "<name>|cam", "<name>|vel"  the reference's float64 maps
    the 375 x 1242 case:  "<name>|cam|index", "|cam|value", "|vel|index", "|vel|value"  the non-zero pixels (flat int32
                          index, float32 value; the vel values are float32 numbers to begin with, the camera depths are
                          rounded once, which the tests that read them allow for)
Asserted here, so that a fixture that contradicts tests/lidar_ref.py cannot be written: oracle == reference in float64 on
every exact, special and degenerate case in both modes; on the other cases an identical vel_depth=True map and an identical
non-zero support in camera mode (there the reference's BLAS sums the projection in another order: last bits).
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference/KITTI")
import lidar_cases  # noqa: E402
import lidar_ref  # noqa: E402

np.int = int  # noqa: NPY001  (kitti_utils.py:92)
import kitti_utils as RK  # noqa: E402  (the reference's)


def reference_maps(case):
    with tempfile.TemporaryDirectory() as d:
        lidar_cases.write_calib(case, d)
        scan = os.path.join(d, "0000000000.bin")
        lidar_cases.write_scan(case, scan)
        with np.errstate(all="ignore"):
            return {mode: RK.generate_depth_map(d, scan, 2, mode == "vel") for mode in ("cam", "vel")}


def main():
    out = {}
    for name in lidar_cases.CASES:
        case = lidar_cases.build(name)
        ref = reference_maps(case)
        ours = {mode: lidar_ref.depth_map(case["points"], case["P"], case["shape"], mode == "vel") for mode in ("cam", "vel")}
        for mode in ("cam", "vel"):
            assert ref[mode].shape == case["shape"] and ref[mode].dtype == np.float64
        assert np.array_equal(ours["vel"], ref["vel"]), name
        assert np.array_equal(ours["cam"] != 0, ref["cam"] != 0), name
        differ = int((ours["cam"] != ref["cam"]).sum())
        if name in lidar_cases.EXACT_CLASS:
            assert differ == 0, (name, differ)
        ulp32 = np.abs(ours["cam"].astype(np.float32).view(np.int32).astype(np.int64) - ref["cam"].astype(np.float32).view(np.int32).astype(np.int64))
        print("%-16s N %6d  non-zero %5d / %5d  camera-mode values that differ from the oracle in float64: %d (after float32 rounding: "
              "%d, at most %d ulp)" % (name, len(case["points"]), (ref["cam"] != 0).sum(), (ref["vel"] != 0).sum(), differ,
                                       (ulp32 != 0).sum(), ulp32.max() if ulp32.size else 0))
        if name == lidar_cases.FULL:
            for mode in ("cam", "vel"):
                flat = ref[mode].ravel()
                index = np.flatnonzero(flat)
                out["%s|%s|index" % (name, mode)] = index.astype(np.int32)
                out["%s|%s|value" % (name, mode)] = flat[index].astype(np.float32)
            assert np.array_equal(out[name + "|vel|value"].astype(np.float64), ref["vel"].ravel()[out[name + "|vel|index"]])
        else:
            out[name + "|cam"], out[name + "|vel"] = ref["cam"], ref["vel"]
    path = os.path.join(ROOT, "tests", "golden", "lidar_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
