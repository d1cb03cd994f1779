"""Mixed reuse sweeps of the fused symmetric n = m = 32 kernel: which launch positions compute Stage A.  The rule is restated in
crash_mix_rule.py; here it is compared with the constants in the C++ sources and with the C++ function itself (compiled for
the host), and its evenness is checked: consecutive workgroup ids go round-robin over the 8 XCDs, so the share must be even
over every XCD's own dispatch sequence and over the launch, whatever the share -- an even period on blockIdx.x would put all
computing wavefronts on half of the dies.

Bounds (reasoned, not measured): within one XCD the rule is an error-diffusion sequence, so any run of L of its positions holds
floor or ceil of L * share / 256 computing ones up to one more rounding -- within 1.  Over the launch, the 8 phases are the 8
multiples of 32, so by Hermite's identity the rows k0 .. k0 + L - 1 hold floor((k0 + L) share / 32) - floor(k0 share / 32)
computing positions -- within 1 of 8 L share / 256."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import crash_mix_rule as rule

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quadraticprogramnetworks.jl_amd", "csrc")
SHARES = sorted({32, 64, 96, 128, 160, 192, 37, 255, 256} | ({rule.SHARE} if rule.SHARE else set()))


def _define(text, name):
    m = re.search(r"#ifndef %s\s*\n#define %s\s+(\d+)\s*\n#endif" % (name, name), text)
    assert m, name
    return int(m.group(1))


def test_constants_match_the_sources():
    capi = open(os.path.join(CSRC, "qpn_capi_nodes.hip")).read()
    internal = open(os.path.join(CSRC, "qpn_internal.h")).read()
    assert _define(capi, "QPN_CRASH_MIX_SHARE") == rule.SHARE
    assert _define(capi, "QPN_CRASH_MIX_TAIL") == rule.TAIL
    m = re.search(r"constexpr int kResidentMI355X = (\d+) \* (\d+);", internal)
    assert m and int(m.group(1)) * int(m.group(2)) == rule.RESIDENT
    assert 0 <= rule.SHARE <= 256 and rule.TAIL >= 0


def test_restatement_equals_the_compiled_rule(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc) and not shutil.which("hipcc"):
        pytest.fail("hipcc not found: the package cannot be built here either")
    src = tmp_path / "rule.hip"
    src.write_text('#include "qpn_internal.h"\n#include <cstdio>\n#include <cstdlib>\n'
                   "int main(int argc, char **argv) {\n"
                   "    const int share = atoi(argv[1]), from = atoi(argv[2]), count = atoi(argv[3]);\n"
                   "    for (int p = 0; p < count; ++p) putchar(crash_mix_recomputes(p, share, from) ? '1' : '0');\n"
                   "    return 0;\n}\n")
    exe = tmp_path / "rule"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])
    for share, batch in [(128, 10000), (96, 40000), (37, 12289), (256, 4500), (rule.SHARE, 10000)]:
        from_ = rule.reuse_from(batch)
        got = subprocess.run([str(exe), str(share), str(from_), str(batch)], capture_output=True, text=True, check=True).stdout
        want = "".join("1" if rule.recomputes(p, share, from_) else "0" for p in range(batch))
        assert got == want, (share, batch)


@pytest.mark.parametrize("batch", [10000, 40000])
@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("tail", sorted({0, 128, rule.TAIL}))
def test_share_is_even_per_xcd_and_per_window(batch, share, tail):
    from_ = rule.reuse_from(batch, tail)
    assert 0 < from_ <= batch and from_ % rule.XCDS == 0
    sel = np.array([rule.recomputes(p, share, from_) for p in range(batch)], dtype=np.int64)
    # every position from reuse_from on reuses
    assert not sel[from_:].any()
    c = share / 256.0
    W = 512
    # per XCD: every window of 512 consecutive positions (any start) below reuse_from holds 64 positions of each XCD
    for x in range(rule.XCDS):
        own = np.zeros(batch, dtype=np.int64)
        own[x::rule.XCDS] = sel[x::rule.XCDS]
        cs = np.concatenate([[0], np.cumsum(own)])
        cnt = cs[W:from_ + 1] - cs[:from_ + 1 - W]
        assert cnt.size > 0 and np.all(np.abs(cnt - c * (W // rule.XCDS)) <= 1.0 + 1e-9), (x, cnt.min(), cnt.max())
        # ... and the XCD's whole mixed sequence holds its share
        assert abs(own.sum() - c * (from_ // rule.XCDS)) <= 1.0 + 1e-9
    # the launch: windows of 512 consecutive positions made of whole rows of 8 (one position per XCD)
    cs = np.concatenate([[0], np.cumsum(sel)])
    starts = np.arange(0, from_ - W + 1, rule.XCDS)
    cnt = cs[starts + W] - cs[starts]
    assert np.all(np.abs(cnt - c * W) <= 1.0 + 1e-9), (cnt.min(), cnt.max())
    # a window that starts inside a row adds two partial rows: at most one more on either side
    cnt = cs[W:from_ + 1] - cs[:from_ + 1 - W]
    assert np.all(np.abs(cnt - c * W) <= 3.0 + 1e-9), (cnt.min(), cnt.max())


def test_small_launches_and_share_zero_are_plain_reuse_sweeps():
    assert not rule.mixed(4096, 128) and not rule.mixed(2500, 128) and not rule.mixed(1250, 128)
    assert not rule.mixed(10000, 0)
    assert rule.mixed(4500, 128) == (rule.reuse_from(4500) > 0)
    assert rule.reuse_from(10000, 0) == 8192 and rule.reuse_from(40000, 0) == 36864 and rule.reuse_from(12289, 0) == 12288
    assert rule.reuse_from(10000, 128) == 6144
