"""KITTI ground-truth depth maps from velodyne scans on the GPU (csrc/wmd_lidar.hip): KITTI/kitti_utils.py.

    read_calib_file(path)                                    kitti_utils.py:23   host
    load_velodyne_points(filename)                           :14                 host
    velo_to_image_matrix(cam2cam, velo2cam, cam=2)           :56-68              host -> (P_velo2im float64 [3,4], (H, W))
    project_lidar(points, P, im_shape, vel_depth, offsets)   :73-104             device tensors, one scan or a packed batch
    generate_depth_map(calib_dir, velo_filename, cam, vel_depth)    :52          -> float32 device tensor [H,W]
    generate_depth_maps(calib_dir, velo_filenames, cam, vel_depth)  -> [B,H,W] in one call, ready for evaluation.kitti_metrics

export_gt_depth.py calls generate_depth_map(calib_dir, velo_filename, 2, True) per test frame of the Eigen split,
KITTIRAWDataset.get_depth calls it per training sample; the resize and flip of get_depth stay with the caller.  The files
are read on the host; projection, scatter and the duplicate rule run in three HIP launches, bit for bit reproducible.
No autograd, no CPU fallback: CPU tensors raise.
"""
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, current_stream, ptr

_FLOAT_CHARS = frozenset("0123456789.e+- ")


def read_calib_file(path):
    """A KITTI calibration file -> {key: text}; a value that is made of number characters only and parses as numbers
    separated by single blanks becomes a float64 array."""
    data = {}
    with open(path, "r") as f:
        for line in f:
            key, colon, value = line.partition(":")
            if not colon:
                raise ValueError("%s: no 'key:' in line %r" % (path, line))
            value = value.strip()
            data[key] = value
            if _FLOAT_CHARS.issuperset(value):
                try:
                    data[key] = np.array([float(tok) for tok in value.split(" ")])
                except ValueError:
                    pass
    return data


def load_velodyne_points(filename):
    """A KITTI velodyne .bin -> [N,4] float32 rows (forward, left, up, 1): the reflectance column is replaced by 1."""
    points = np.fromfile(filename, dtype=np.float32).reshape(-1, 4)
    points[:, 3] = 1.0
    return points


def velo_to_image_matrix(cam2cam, velo2cam, cam=2):
    """The dictionaries of calib_cam_to_cam.txt and calib_velo_to_cam.txt -> (P_velo2im float64 [3,4], (H, W)).
    P_velo2im = (P_rect_0<cam> . R_cam2rect) . velo2cam, the products in that order; the image size is S_rect_02 for
    every camera, as in the reference."""
    rigid = np.vstack((np.hstack((velo2cam["R"].reshape(3, 3), velo2cam["T"][..., np.newaxis])), np.array([0, 0, 0, 1.0])))
    H, W = (int(v) for v in cam2cam["S_rect_02"][::-1].astype(np.int32))
    R_cam2rect = np.eye(4)
    R_cam2rect[:3, :3] = cam2cam["R_rect_00"].reshape(3, 3)
    P_rect = cam2cam["P_rect_0" + str(cam)].reshape(3, 4)
    return np.dot(np.dot(P_rect, R_cam2rect), rigid), (H, W)


def project_lidar(points, P, im_shape, vel_depth=False, offsets=None):
    """points [N,4] float32 (the 4th column is ignored), P [3,4] float64 -> depth [H,W] float32; or the packed batch:
    points [total,4], offsets [B+1] int64 on the device (scan b is rows offsets[b] .. offsets[b+1]-1), P [B,3,4] ->
    [B,H,W].  Per pixel the value of the last point that lands there -- the forward coordinate x with vel_depth, else
    the camera depth -- then the reference's duplicate rule over sub2ind buckets; 0 where nothing lands."""
    single = offsets is None
    _lib.require_device("project_lidar", points=(points, torch.float32), P=(P, torch.float64))
    if points.dim() != 2 or points.shape[1] != 4:
        raise _lib.WmdError("points must be [N,4] (got %s)" % (tuple(points.shape),))
    total = points.shape[0]
    if single:
        if tuple(P.shape) != (3, 4):
            raise _lib.WmdError("P must be [3,4] for a single scan (got %s)" % (tuple(P.shape),))
        P = P.unsqueeze(0)
        offsets = torch.tensor([0, total], dtype=torch.int64, device=points.device)
    _lib.require_device("project_lidar", offsets=(offsets, torch.int64))
    if offsets.dim() != 1 or offsets.numel() < 2 or tuple(P.shape) != (offsets.numel() - 1, 3, 4):
        raise _lib.WmdError("offsets must be [B+1] and P [B,3,4] (got %s, %s)" % (tuple(offsets.shape), tuple(P.shape)))
    B = offsets.numel() - 1
    H, W = int(im_shape[0]), int(im_shape[1])
    if H < 1 or W < 1:
        raise _lib.WmdError("im_shape must be positive (got %d x %d)" % (H, W))
    points, P, offsets = points.detach().contiguous(), P.detach().contiguous(), offsets.contiguous()
    l = _lib.lib()
    ws, n = _lib.byte_workspace(l.wmd_lidar_depth_workspace_bytes(B, H, W), points.device)
    depth = torch.empty((B, H, W), device=points.device, dtype=torch.float32)
    check(l.wmd_lidar_depth_maps(ptr(points) if total else None, ptr(offsets), ptr(P), total, B, H, W, 1 if vel_depth else 0,
                                 ptr(depth), ptr(ws), n, current_stream()), "wmd_lidar_depth_maps")
    return depth[0] if single else depth


def generate_depth_maps(calib_dir, velo_filenames, cam=2, vel_depth=False, device="cuda"):
    """The scans of one calibration directory -> [B,H,W] float32 on the device in one call: the reference's
    generate_depth_map(calib_dir, f, cam, vel_depth) for every f."""
    cam2cam = read_calib_file(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
    velo2cam = read_calib_file(os.path.join(calib_dir, "calib_velo_to_cam.txt"))
    P, im_shape = velo_to_image_matrix(cam2cam, velo2cam, cam)
    scans = [load_velodyne_points(f) for f in velo_filenames]
    if not scans:
        raise _lib.WmdError("generate_depth_maps needs at least one scan")
    offsets = np.concatenate(([0], np.cumsum([len(s) for s in scans]))).astype(np.int64)
    dev = torch.device(device)
    return project_lidar(torch.from_numpy(np.concatenate(scans, axis=0)).to(dev), torch.from_numpy(P)[None].repeat(len(scans), 1, 1).to(dev),
                         im_shape, vel_depth, torch.from_numpy(offsets).to(dev))


def generate_depth_map(calib_dir, velo_filename, cam=2, vel_depth=False, device="cuda"):
    """The reference's generate_depth_map: one scan -> [H,W] float32 on the device."""
    return generate_depth_maps(calib_dir, [velo_filename], cam, vel_depth, device)[0]
