"""The workspace layouts of the data, loss and evaluation operators (csrc/wmd_ws_layouts.h on WsLayout of csrc/wmd_internal.h), checked on
the CPU.

tests/ws_layout_host.cpp includes the header and walks every layout function over the shapes of test_workspace_host.QUERIES and of the
existing host tests: sizing on a null workspace equals carving a real buffer, the regions are pairwise disjoint, aligned and inside the
answered bytes, and they start where include/wmd.h says they do.  The two float workspaces that hold fp64 partials are carved at bases
that are 0, 4, 8 and 12 mod 16.  Compiled for the host only, once plain and once with the address and undefined-behaviour sanitizers:
a stand-alone program, no HIP call, no GPU.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_every_layout_sizes_as_it_carves(tmp_path, sanitize):
    exe = str(tmp_path / "ws_layout_host")
    src = os.path.join(ROOT, "tests", "ws_layout_host.cpp")
    extra = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--offload-host-only", "-O1", "-std=c++17", "-Wall", "-Werror",
                           "-Wno-unused-function", "-I" + os.path.join(ROOT, "include")] + extra + [src, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    m = re.search(r"(\d+) checks, (\d+) failed", r.stdout)
    assert m, r.stdout + r.stderr
    assert r.returncode == 0 and int(m.group(2)) == 0 and not r.stderr.strip(), r.stdout[-4000:] + r.stderr[-4000:]
    assert int(m.group(1)) > 1000
