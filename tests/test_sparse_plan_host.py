"""CPU: what wmd_sparse_conv would launch (wmd_sparse_conv_plan, wmd_sparse_conv_config_name) held against the independent statement
of the host's rules in sparse_conv_ref.select -- the instantiation and grid.x for every row of the GPU module's case table, under the
default switches and, in child processes (the library reads them once), under WMD_SPARSE_MR / _ROWS / _GRID -- and the refusals:
the query and the launch entry answer a bad problem with the same text, before any HIP call (the dummy pointers reach no kernel)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import sparse_conv_ref as SR
from wavelet_monodepth_amd import _lib, sparse_ops

BAD_ARG, BAD_SHAPE, UNSUPPORTED = -1, -2, -3


def _atoi(name, default):
    if name not in os.environ:
        return default
    m = re.match(r"\s*[-+]?\d+", os.environ[name])
    return int(m.group()) if m else 0


def switches():
    """the library's switches as this process's environment sets them, in the mirror's words"""
    return dict(grid_target=_atoi("WMD_SPARSE_GRID", 2048), rows_on=_atoi("WMD_SPARSE_ROWS", 1) != 0, mr_force=_atoi("WMD_SPARSE_MR", 0))


def plan(c, max_out):
    return sparse_ops.sparse_conv_plan(c["H"], c["W"], c["C1"], c["Cout"], c["ksize"], max_out, B=c["B"], up1=c["up1"], C2=c["C2"], C1tot=c["C1tot"],
                                       c1_off=c["c1_off"], dual=c["dual"], c1_off2=c["c1_off2"], pad=c["pads"][0], act=c["act"],
                                       split_waves=c["split_waves"])


def check_table():
    """every table row at four capacities: the plan's name and grid.x are the mirror's under this process's switches"""
    sw = switches()
    for c in SR.TABLE:
        for max_out in (1, 16, 17, c["H"] * c["W"]):
            want = SR.case_select(c, max_out, **sw)
            assert plan(c, max_out) == (want["name"], want["grid_x"]), (c["key"], max_out, sw, plan(c, max_out), want)
    print("PLAN OK", sw)


def test_table_is_the_twelve_instantiations():
    lib = _lib.lib()
    n = lib.wmd_sparse_conv_num_configs()
    assert n == 12
    assert sorted(lib.wmd_sparse_conv_config_name(i).decode() for i in range(n)) == SR.ALL_INSTANTIATIONS
    assert lib.wmd_sparse_conv_config_name(-1) is None and lib.wmd_sparse_conv_config_name(n) is None


def test_every_row_names_the_instantiation_it_exists_for():
    assert switches() == dict(grid_target=2048, rows_on=True, mr_force=0), "the suite runs under the default switches"
    for c in SR.TABLE:
        assert plan(c, c["H"] * c["W"])[0] == SR.want_name(c), c["key"]


def test_plan_follows_the_mirror():
    check_table()


SETTINGS = [("WMD_SPARSE_MR", "1"), ("WMD_SPARSE_MR", "2"), ("WMD_SPARSE_MR", "4"), ("WMD_SPARSE_ROWS", "0"), ("WMD_SPARSE_GRID", "64")]


def test_plan_follows_the_mirror_under_every_switch():
    """one fresh process per setting (started together); the mirror is given the same setting"""
    here = os.path.dirname(os.path.abspath(__file__))
    children = []
    for switch, value in SETTINGS:
        env = {k: v for k, v in os.environ.items() if not k.startswith("WMD_SPARSE_")}
        env[switch] = value
        env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(here), here, env.get("PYTHONPATH", "")])
        children.append((switch, value, subprocess.Popen([sys.executable, "-c", "import test_sparse_plan_host as T; T.check_table()"], env=env,
                                                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    for switch, value, p in children:
        out, err = p.communicate(timeout=120)
        assert p.returncode == 0 and "PLAN OK" in out, "%s=%s: exit status %d\n%s\n%s" % (switch, value, p.returncode, out[-2000:], err[-4000:])
    # the settings were live: each one moves some row of the table off the default plan
    default = {(c["key"], m): SR.case_select(c, m) for c in SR.TABLE for m in (1, 16, 17, c["H"] * c["W"])}
    for sw in (dict(mr_force=1), dict(mr_force=2), dict(mr_force=4), dict(rows_on=False), dict(grid_target=64)):
        assert any(SR.case_select(SR.CASES[k], m, **sw) != v for (k, m), v in default.items()), sw


BASE = dict(H=8, W=10, C1=5, up1=1, C1tot=5, c1_off=0, C2=0, Cout=4, ksize=3, pad_mode=1, act=1, max_out=80, c1_off2=0, split_waves=0, B=1)
REFUSALS = [
    ("ksize", dict(ksize=5), UNSUPPORTED, "wmd_sparse_conv: ksize=5"),
    ("max_out", dict(max_out=-1), BAD_SHAPE, "wmd_sparse_conv: max_out=-1"),
    ("split_waves", dict(split_waves=-1), BAD_ARG, "wmd_sparse_conv: split_waves=-1"),
    ("slice", dict(c1_off=3, C1tot=7), BAD_ARG, "wmd_sparse_conv: channel slice"),
    ("dual_cout", dict(wp2=1, bias2=1, Cout=17, C1tot=10, c1_off2=5), BAD_ARG, "wmd_sparse_conv: dual-head mode needs Cout <= 16, C2 == 0 and a valid slice"),
]


@pytest.mark.parametrize("key,change,status,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_of_the_plan_are_the_launch_entrys(key, change, status, text):
    lib = _lib.lib()
    p = dict(BASE, **change)
    gx = C.c_int(7)
    assert lib.wmd_sparse_conv_plan(C.byref(_lib.SparseConvArgs(**p)), C.byref(gx)) == -1 and gx.value == 0
    assert lib.wmd_last_error().decode() == text
    assert lib.wmd_sparse_conv_plan(C.byref(_lib.SparseConvArgs(**p)), None) == -1
    ptrs = dict(x1=1, out_coords=1, out_nnz=1, wp=1, bias=1, y=1)
    assert lib.wmd_sparse_conv(C.byref(_lib.SparseConvArgs(**p, **ptrs)), None) == status
    assert lib.wmd_last_error().decode() == text


def test_an_empty_launch_has_no_plan_and_no_error():
    lib = _lib.lib()
    gx = C.c_int(7)
    assert lib.wmd_sparse_conv_plan(C.byref(_lib.SparseConvArgs(**dict(BASE, ksize=5))), None) == -1
    before = lib.wmd_last_error()
    assert lib.wmd_sparse_conv_plan(C.byref(_lib.SparseConvArgs(**dict(BASE, max_out=0))), C.byref(gx)) == -1 and gx.value == 0
    assert lib.wmd_sparse_conv_plan(C.byref(_lib.SparseConvArgs(**dict(BASE, max_out=0, split_waves=-1, B=70000))), None) == -1   # as the launch: nothing to refuse
    assert lib.wmd_last_error() == before == b"wmd_sparse_conv: ksize=5", "the empty launch's answer sets no error"
    assert sparse_ops.sparse_conv_plan(8, 10, 5, 4, 3, 0) == (None, 0)
    # the accepted problem beside it, for contrast: no pointer is needed, wp2 is only "dual"
    assert lib.wmd_sparse_conv_plan(C.byref(_lib.SparseConvArgs(**BASE)), C.byref(gx)) >= 0 and gx.value == 5
