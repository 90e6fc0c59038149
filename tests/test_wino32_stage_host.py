"""The gather-offset arithmetic of the 32x32x2 Winograd kernels' staging front end (csrc/wmd_conv_wino32_stage.h), checked on the CPU.

tests/wino32_stage_host.cpp includes the header's host-callable part and walks, for every patch position of every 2x2 Winograd tile
with an output pixel inside the image, the table route (w32_full_rc / w32_low_rc + channel * plane + row + column) against the
per-position rule of conv_wino32_kernel's GENERIC staging: both read zero or both give the same byte offset, the low-resolution
cell of an upsampled operand is the one the UP transform reads, and the 16-byte pieces -- exactly where the whole patch row lies
inside the source row -- start at the dword offsets of their columns.  All three pad modes, same-size / upsampled / data-gradient
sources, maps a few pixels either side of one and two tiles (6x20, 7x18, 9x22, 12x40, 14x18, 5x7 among them).  Compiled for the
host only; no HIP call, no GPU.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wino32_stage") / "wino32_stage_host")
    src = os.path.join(ROOT, "tests", "wino32_stage_host.cpp")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--offload-host-only", "-O2", "-std=c++17", "-Wall", "-Werror",
                           "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    return exe


@pytest.mark.parametrize("tile,x4", [("8x16", True), ("4x32", True), ("6x20", False), ("6x40", False)])
def test_table_route_equals_the_per_position_rule(walker, tile, x4):
    r = subprocess.run([walker, tile], capture_output=True, text=True)
    m = re.search(r"checked (\d+) failed (\d+) x4_tiles (\d+) low_cells (\d+)", r.stdout)
    assert m, r.stdout + r.stderr
    checked, failed, x4_tiles, low_cells = map(int, m.groups())
    assert r.returncode == 0 and failed == 0, r.stdout[-4000:]
    assert checked > 100000 and low_cells > 10000
    assert (x4_tiles > 0) == x4     # interior tiles of the 16- and 32-wide shapes took the 16-byte comparison; 20 / 40 wide have none
