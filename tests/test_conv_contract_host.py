"""CPU: the fused convolution's problem contract (include/wmd.h, at wmd_conv_args) as every entry that takes the problem
answers it -- one violated rule at a time, then pairs for the order.  Every refusal precedes any HIP call: the dummy non-null
pointers never reach a kernel, and no launch entry is ever called with a problem it would accept."""
import ctypes as C

import pytest

from wavelet_monodepth_amd import _lib

BASE = dict(B=2, H=12, W=40, C1=32, up1=2, C2=16, Cout=32, ksize=3, pad_mode=1)
AMPLE = 1 << 40   # workspace floats: no entry gets as far as asking for more


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def conv_args(p, null=()):
    ptr = {k: None if k in null else 1 for k in ("x1", "x2", "wp", "y")}
    return _lib.ConvArgs(act=p.get("act", 1), slope=0.0, bias=None, workspace=1, workspace_floats=AMPLE, tune_cfg=0, tune_ksplit=0,
                         **ptr, **{k: p[k] for k in BASE})


def problem_of(cls, p, **kw):
    return cls(**{k: p[k] for k in BASE if k in dict(cls._fields_)}, **kw)


def fwd(lib, p, null=()):
    return lib.wmd_conv_fwd(C.byref(conv_args(p, null)), None)


def bf16(lib, p, null=()):
    return lib.wmd_conv_bf16_fwd(C.byref(conv_args(p, null)), 3, None)


def wino44(lib, p, null=()):
    return lib.wmd_conv_wino44_fwd(C.byref(conv_args(p, null)), None)


def dgrad(lib, p, null=()):
    a = problem_of(_lib.ConvDgradArgs, p, dz=1, wp_dgrad=1, dx1=1, dx2=1, workspace=1, workspace_floats=AMPLE)
    return lib.wmd_conv_dgrad(C.byref(a), None)


def wgrad(lib, p, null=()):
    a = problem_of(_lib.ConvWgradArgs, p, x1=None if "x1" in null else 1, x2=None if "x2" in null else 1, dz=1, dw=1, dbias=1,
                   workspace=1, workspace_floats=AMPLE)
    return lib.wmd_conv_wgrad(C.byref(a), None)


def dw_args(p, null):
    return problem_of(_lib.DwConvArgs, p, x1=None if "x1" in null else 1, x2=None if "x2" in null else 1, w=1)


def dw_fwd(lib, p, null=()):
    return lib.wmd_dwconv3x3_fwd(C.byref(dw_args(p, null)), 1, None)


def dw_bwd(lib, p, null=()):
    return lib.wmd_dwconv3x3_bwd(C.byref(dw_args(p, null)), 1, 1, 1, 1, 1, 1, AMPLE, None)


def sparse(lib, p, null=()):
    a = problem_of(_lib.SparseConvArgs, p, C1tot=BASE["C1"], c1_off=0, act=p.get("act", 1), slope=0.0, x1=None if "x1" in null else 1,
                   x2=None if "x2" in null else 1, out_coords=1, out_nnz=1, max_out=16, wp=1, y=1, out_scale=1.0, nnz_stride=1)
    return lib.wmd_sparse_conv(C.byref(a), None)


# entry -> (call, the rows that have no meaning for it)
ENTRIES = {
    "wmd_conv_fwd": (fwd, ()),
    "wmd_conv_bf16_fwd": (bf16, ()),
    "wmd_conv_wino44_fwd": (wino44, ()),
    "wmd_conv_dgrad": (dgrad, ("act", "x1")),
    "wmd_conv_wgrad": (wgrad, ("act",)),
    "wmd_dwconv3x3_fwd": (dw_fwd, ("act", "ksize", "Cout")),
    "wmd_dwconv3x3_bwd": (dw_bwd, ("act", "ksize", "Cout")),
    "wmd_sparse_conv": (sparse, ("B",)),   # its frame count is max(B, 1)
}

# (what the row is about, the change, status, a word of the message) in the documented order of the rules
ROWS = [
    ("B", dict(B=0), -2, b"B="),
    ("H", dict(H=0), -2, b"B="),
    ("C1", dict(C1=0), -2, b"B="),
    ("C2", dict(C2=-1), -2, b"B="),
    ("Cout", dict(Cout=0), -2, b"B="),
    ("ksize", dict(ksize=5), -3, b"ksize"),
    ("up1", dict(up1=3), -1, b"up1"),
    ("even", dict(H=13), -2, b"even"),
    ("pad_mode", dict(pad_mode=3), -1, b"pad_mode"),
    ("act", dict(act=4), -1, b"act"),
    ("reflect", dict(H=1, W=1, up1=1), -2, b"reflect"),
]
CASES = [(e, r) for e in ENTRIES for r in ROWS if r[0] not in ENTRIES[e][1]]


@pytest.mark.parametrize("entry,row", CASES, ids=["%s-%s" % (e, r[0]) for e, r in CASES])
def test_one_violated_rule(lib, entry, row):
    what, change, status, word = row
    if entry == "wmd_conv_dgrad" and what == "C2":
        status, word = -1, b"dx2 given"   # its own rule, in front of the shared ones
    assert ENTRIES[entry][0](lib, dict(BASE, **change)) == status
    assert word in lib.wmd_last_error(), lib.wmd_last_error()


@pytest.mark.parametrize("entry", [e for e in ENTRIES if "x1" not in ENTRIES[e][1]])
def test_a_launch_needs_its_tensors(lib, entry):
    call = ENTRIES[entry][0]
    assert call(lib, BASE, null=("x1",)) == -1 and b"null" in lib.wmd_last_error()
    assert call(lib, BASE, null=("x2",)) == -1 and b"x2" in lib.wmd_last_error()


def queries(lib, p, null):
    a = conv_args(p, null)
    return (lib.wmd_conv_bf16_supported(C.byref(a), 3), lib.wmd_conv_bf16_workspace_floats(C.byref(a), 3),
            lib.wmd_conv_wino44_supported(C.byref(a)), lib.wmd_conv_wino44_workspace_floats(C.byref(a)),
            lib.wmd_conv_fwd_workspace_floats(C.byref(a)))


def test_shape_queries_read_no_tensor_pointer(lib):
    nulls = ("x1", "x2", "wp", "y")
    got = queries(lib, BASE, nulls)
    assert got == queries(lib, BASE, ()) and got[0] == 1 and got[2] == 1 and got[3] > 0
    assert lib.wmd_conv_fwd_plan(C.byref(conv_args(BASE, nulls)), None) == lib.wmd_conv_fwd_plan(C.byref(conv_args(BASE)), None) >= 0
    for what, change, _, _ in ROWS:
        p = dict(BASE, **change)
        assert queries(lib, p, nulls)[:4] == (0, 0, 0, 0), what
        assert queries(lib, p, nulls) == queries(lib, p, ()), what


@pytest.mark.parametrize("entry", ["wmd_conv_fwd", "wmd_conv_bf16_fwd", "wmd_conv_wino44_fwd", "wmd_sparse_conv"])
@pytest.mark.parametrize("change,status,word", [
    (dict(B=0, H=0, up1=3), -2, b"B="),             # sizes before up1
    (dict(H=0, ksize=5), -2, b"B="),                # sizes before ksize
    (dict(ksize=5, up1=3), -3, b"ksize"),           # ksize before up1
    (dict(H=13, pad_mode=3), -2, b"even"),          # evenness before pad_mode
    (dict(act=4, H=1, W=1, up1=1), -1, b"act"),     # act before the reflect minimum
])
def test_simultaneous_violations_report_in_the_documented_order(lib, entry, change, status, word):
    assert ENTRIES[entry][0](lib, dict(BASE, **change)) == status
    assert word in lib.wmd_last_error(), lib.wmd_last_error()
