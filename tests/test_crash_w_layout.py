"""Layout of W~ in the crash cache of the fused symmetric n = m = 32 kernel (csrc/qpn_internal.h, crash_w_index): the index
function is compiled for the host and checked on all 1024 entries.  A reuse sweep's read-back fetches only the columns of W~
whose multiplier is not zero, which saves memory traffic only if a column owns its cache lines; and a lane moves the four tile
registers g of one (row half Ib, lane group lq) as one 32-byte piece."""
import os
import shutil
import subprocess

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quadraticprogramnetworks.jl_amd", "csrc")
LINE = 128 // 8           # doubles per 128-byte cache line


@pytest.fixture(scope="module")
def index(tmp_path_factory):
    """idx[row, col] and the cache's constants, from the compiled header."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc) and not shutil.which("hipcc"):
        pytest.fail("hipcc not found: the package cannot be built here either")
    tmp = tmp_path_factory.mktemp("crash_w")
    src = tmp / "layout.hip"
    src.write_text('#include "qpn_internal.h"\n#include <cstdio>\n'
                   "int main() {\n"
                   '    printf("%d %d %d %d\\n", kCrashU, kCrashW, kCrashS, kCrashDoubles);\n'
                   '    for (int r = 0; r < 32; ++r) for (int c = 0; c < 32; ++c) printf("%d\\n", crash_w_index(r, c));\n'
                   "    return 0;\n}\n")
    exe = tmp / "layout"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    consts = dict(zip(("U", "W", "S", "doubles"), map(int, out[0].split())))
    idx = np.array([int(x) for x in out[1:1025]], dtype=np.int64).reshape(32, 32)
    return idx, consts


def test_the_map_is_a_bijection_onto_the_block(index):
    idx, consts = index
    assert sorted(idx.ravel().tolist()) == list(range(1024))
    # the W~ block is exactly the space between U' and S
    assert consts["W"] - consts["U"] == 1024 and consts["S"] - consts["W"] == 1024


def test_the_block_starts_on_a_cache_line_in_every_node(index):
    _, consts = index
    # (the allocation itself comes from hipMalloc, aligned to 256 bytes or more)
    assert consts["W"] % LINE == 0 and consts["doubles"] % LINE == 0


def test_a_column_owns_exactly_two_lines(index):
    idx, _ = index
    lines = idx // LINE
    owner = {}
    for c in range(32):
        own = set(lines[:, c].tolist())
        assert len(own) == 2, (c, own)
        # one line per row half
        assert len(set(lines[:16, c].tolist())) == 1 and len(set(lines[16:, c].tolist())) == 1
        for ln in own:
            assert owner.setdefault(ln, c) == c, f"line {ln} is shared by columns {owner[ln]} and {c}"
    assert len(owner) == 64


def test_a_lanes_four_registers_are_one_aligned_piece(index):
    idx, _ = index
    for ib in range(2):
        for lq in range(4):
            for c in range(32):
                at = [idx[16 * ib + 4 * g + lq, c] for g in range(4)]
                assert at == list(range(at[0], at[0] + 4)) and at[0] % 4 == 0, (ib, lq, c, at)
