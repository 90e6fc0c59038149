"""Colour images of the predictions on the GPU (csrc/wmd_viz.hip): the three places the reference makes them on the host, for
whole batches resident in HBM, with the bytes numpy and matplotlib give there.

    disparity_image(disp, size)      KITTI/test_simple.py:144-175: bilinear resize, min .. 95th percentile, magma, uint8
    colorize(value, vmin, vmax)      NYUv2/utils.py:63-82: fixed (0.1 .. 10 m) or automatic range, plasma, uint8
    normalize_image(x)               KITTI/utils.py:22-28: (x - min) / (max - min) for the event file

The colormap tables ship as data (data/colormaps.json, hex text: uint8 [256,3] = (cmap(arange(256))[:, :3] * 255)
.astype(uint8) of matplotlib 3.10.8, whose colormap data is CC0) and are uploaded once per device; matplotlib is not
imported.  No CPU fallback: CPU tensors raise.  Inputs of disparity_image, of colorize's automatic range and of normalize_image must be finite.
"""
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, current_stream, ptr

_TABLES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "colormaps.json")
_host_tables = None
_device_tables = {}


def colormap(name, device=None):
    """uint8 [256,3] table `name` ("magma", "plasma"): the numpy array, or with `device` the copy resident there"""
    global _host_tables
    if _host_tables is None:
        import json

        with open(_TABLES) as f:
            _host_tables = {k: np.frombuffer(bytes.fromhex(v), np.uint8).reshape(256, 3).copy() for k, v in json.load(f).items() if k != "source"}
    if name not in _host_tables:
        raise ValueError("unknown colormap %r (shipped: %s)" % (name, ", ".join(sorted(_host_tables))))
    if device is None:
        return _host_tables[name]
    key = (name, torch.device(device))
    if key not in _device_tables:
        _device_tables[key] = torch.from_numpy(_host_tables[name]).to(device).contiguous()
    return _device_tables[key]


def _maps(t, what):
    """a float32 device tensor [H,W], [B,H,W] or [B,1,H,W] -> [B,H,W]"""
    _lib.require_device(what, input=(t, torch.float32))
    if t.dim() == 2:
        return t[None]
    if t.dim() == 4 and t.shape[1] == 1:
        return t[:, 0]
    if t.dim() != 3:
        raise _lib.WmdError("%s expects [H,W], [B,H,W] or [B,1,H,W], got %s" % (what, tuple(t.shape)))
    return t


def disparity_image(disp, size=None, percentile=95, cmap="magma", return_range=False, return_resized=False, workspace=None):
    """disp [B,h,w] (or [B,1,h,w], [h,w]) float32 at decoder resolution -> uint8 [B,H,W,3] on the device: what test_simple
    saves as <name>_disp.jpeg, for every image of the batch in five launches.  size = (H, W) of the pictures (None: h, w).
    vmin = the map's min, vmax = np.percentile(map, percentile) exactly (a radix select, no sort), per image.
    return_range: also [B,2] float32 (vmin, vmax); return_resized: also the resized maps [B,H,W], bit-equal to
    ops.upsample_bilinear(disp, size).  workspace: a device tensor of any dtype to reuse between calls (its contents do not matter)."""
    if not 0 <= float(percentile) <= 100:
        raise ValueError("Percentiles must be in the range [0, 100]")
    d = _maps(disp, "disparity_image").contiguous()
    B, h, w = d.shape
    H, W = (h, w) if size is None else (int(size[0]), int(size[1]))
    dev = d.device
    rgb = torch.empty((B, H, W, 3), device=dev, dtype=torch.uint8)
    rng = torch.empty((B, 2), device=dev, dtype=torch.float32) if return_range else None
    res = torch.empty((B, H, W), device=dev, dtype=torch.float32) if return_resized else None
    l = _lib.lib()
    if workspace is None:
        workspace, n = _lib.byte_workspace(l.wmd_viz_workspace_bytes(B, H, W), dev)
    else:
        n = workspace.numel() * workspace.element_size()
    check(l.wmd_viz_disparity(ptr(d), B, h, w, H, W, float(percentile), ptr(colormap(cmap, dev)), ptr(rgb), ptr(res), ptr(rng),
                              ptr(workspace), n, current_stream()), "wmd_viz_disparity")
    out = (rgb,) + ((rng,) if return_range else ()) + ((res,) if return_resized else ())
    return out[0] if len(out) == 1 else out


def colorize(value, vmin=0.1, vmax=10, cmap="plasma", channels_first=True):
    """value [B,H,W] (or [B,1,H,W], [H,W]) float32 -> uint8 [B,3,H,W] (channels_first, what the reference returns per image)
    or [B,H,W,3].  vmin and vmax both numbers: t = (value - vmin) / (vmax - vmin) in float32, below the range -> the first
    colour, above -> the last, NaN -> black.  Both None: every map's own min and max.  One of the two None: ValueError."""
    if (vmin is None) != (vmax is None):
        raise ValueError("colorize: give both vmin and vmax, or neither")
    v = _maps(value, "colorize").contiguous()
    B, H, W = v.shape
    dev = v.device
    out = torch.empty((B, 3, H, W) if channels_first else (B, H, W, 3), device=dev, dtype=torch.uint8)
    auto = vmin is None
    ws, n = _lib.byte_workspace(_lib.lib().wmd_viz_workspace_bytes(B, 1, 1), dev) if auto else (None, 0)
    # as numpy does with a float32 array and Python scalars: the difference in double, each scalar rounded to float32
    lo, den = (0.0, 0.0) if auto else (float(np.float32(vmin)), float(np.float32(vmax - vmin)))
    check(_lib.lib().wmd_viz_colorize(ptr(v), B, H * W, int(auto), lo, den, ptr(colormap(cmap, dev)), ptr(out), int(bool(channels_first)),
                                      ptr(ws), n, current_stream()), "wmd_viz_colorize")
    return out[0] if value.dim() == 2 else out


def normalize_image(x, per_image=False):
    """(x - min) / (max - min) in float32, 1e5 in place of a zero range; the range over the whole tensor (the reference's
    form) or, per_image, over every x[b] on its own.  Same shape as x."""
    _lib.require_device("normalize_image", x=(x, torch.float32))
    v = x.contiguous()
    if v.numel() == 0:
        return v.clone()
    B = v.shape[0] if per_image and v.dim() > 1 else 1
    y = torch.empty_like(v)
    ws, n = _lib.byte_workspace(_lib.lib().wmd_viz_workspace_bytes(B, 1, 1), v.device)
    check(_lib.lib().wmd_viz_normalize(ptr(v), ptr(y), B, v.numel() // B, ptr(ws), n, current_stream()), "wmd_viz_normalize")
    return y
