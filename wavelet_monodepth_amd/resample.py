"""Pillow's 8-bit resample tables (csrc/wmd_resample.h), built by the library on the host, for kitti_inputs and nyu_inputs:
one (bounds, coeffs) pair per axis, and the memo of the packed tables a call uploads once per shape."""
import numpy as np
import torch

from . import _lib
from ._lib import check

FILTER_BICUBIC, FILTER_LANCZOS = 0, 1

DEVICE_TABLES = {}   # (entry point, its shape arguments, device) -> int32 device tensor


def table(name, *args):
    """(bounds int32 [out,2] = (xmin, n), coeffs int32 [out,ksize]) by wmd_<name>_ksize / wmd_<name>_table: "resample" with
    (filter, n_in, n_out), or "lanczos", its alias in the C ABI, with (n_in, n_out)"""
    l = _lib.lib()
    args = [int(a) for a in args]
    ksize = getattr(l, "wmd_%s_ksize" % name)(*args)
    if ksize == 0:
        raise _lib.WmdError("%s_table%s: filter or sizes out of range" % (name, tuple(args)))
    bounds, coeffs = np.zeros((args[-1], 2), np.int32), np.zeros((args[-1], ksize), np.int32)
    check(getattr(l, "wmd_%s_table" % name)(*args, bounds.ctypes.data, coeffs.ctypes.data, ksize), "wmd_%s_table" % name)
    return bounds, coeffs


def resample_table(filter, n_in, n_out):
    """Pillow's 8-bit resize with FILTER_BICUBIC or FILTER_LANCZOS"""
    return table("resample", filter, n_in, n_out)


def device_tables(name, args, device):
    """the packed tables of wmd_<name>(*args, ...) on `device`: wmd_<name>_table_ints ints by wmd_<name>_tables, uploaded once"""
    key = (name, tuple(args), str(device))
    if key not in DEVICE_TABLES:
        l = _lib.lib()
        n = getattr(l, "wmd_%s_table_ints" % name)(*args)
        host = np.zeros(max(n, 1), np.int32)
        check(getattr(l, "wmd_%s_tables" % name)(*args, host.ctypes.data, n), "wmd_%s_tables" % name)
        DEVICE_TABLES[key] = torch.from_numpy(host).to(device)
    return DEVICE_TABLES[key]
