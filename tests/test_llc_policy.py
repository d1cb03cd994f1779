"""Which sweeps stream the crash cache past the last-level cache (llc_streams_crash, csrc/qpn_internal.h): R = what a sweep touches of
the node records and the outputs, C = the crash cache; stream iff R <= budget < R + C.  Below that window everything fits and
default loads keep all of it resident; above it nothing can be kept and the launch takes the instantiation it always took.
The rule is restated here in Python and compared with the C++ function itself, compiled for the host, over a grid of
(batch, n, m, p, budget); then the cases that matter: the benchmark's 10 000 nodes stream at the default budget, 40 000 nodes
(beyond the cache) and 4 096 (everything fits) do not, budget 0 never streams, budget -1 always does, and the decision is
monotone in the budget on both edges of the window."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quadraticprogramnetworks.jl_amd", "csrc")
CRASH_DOUBLES = 2816

BATCHES = (1, 96, 4096, 4500, 6000, 7000, 8000, 10000, 12000, 14000, 20000, 40000, 1 << 20)
SHAPES = ((32, 32, 8), (32, 32, 0), (32, 32, 64), (16, 16, 8), (5, 3, 2))
BUDGETS = (-1, 0, 1, 64, 128, 200, 255, 256, 257, 300, 320, 400, 512, 1024, 1 << 20)


def record_bytes(n, m, p):
    return 8 * (n * n + n * p + n + m * n + m * p + 2 * m)          # Qd, R, qd, Ad, B, l, u


def output_bytes(n, m):
    return 8 * (n + m) + (n + m) + 4 + 8 + 4 + 8 * n                 # z, active, status, resid, pivots, x


def streams(batch, n, m, p, budget_mb):
    if budget_mb < 0:
        return True
    if budget_mb == 0:
        return False
    R = batch * (record_bytes(n, m, p) + output_bytes(n, m))
    C = batch * CRASH_DOUBLES * 8
    return R <= (budget_mb << 20) < R + C


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc) and not shutil.which("hipcc"):
        pytest.fail("hipcc not found: the package cannot be built here either")
    tmp = tmp_path_factory.mktemp("llc")
    src = tmp / "llc.hip"
    src.write_text('#include "qpn_internal.h"\n#include <cstdio>\n'
                   "int main() {\n"
                   '    printf("%d %d\\n", kLlcBudgetMB, kCrashDoubles);\n'
                   "    long long b, n, m, p, g;\n"
                   '    while (scanf("%lld %lld %lld %lld %lld", &b, &n, &m, &p, &g) == 5) putchar(llc_streams_crash(b, n, m, p, g) ? \'1\' : \'0\');\n'
                   "    return 0;\n}\n")
    exe = tmp / "llc"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])

    def run(cases):
        text = "".join("%d %d %d %d %d\n" % c for c in cases)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout
        head, _, bits = out.partition("\n")
        default, doubles = (int(v) for v in head.split())
        return default, doubles, [c == "1" for c in bits]

    return run


def test_constants_match_the_sources(compiled):
    internal = open(os.path.join(CSRC, "qpn_internal.h")).read()
    m = re.search(r"#ifndef QPN_LLC_BUDGET_MB\s*\n#define QPN_LLC_BUDGET_MB\s+(\d+)\s*\n#endif", internal)
    assert m
    default, doubles, _ = compiled([])
    assert default == int(m.group(1)) and default > 0
    assert doubles == CRASH_DOUBLES
    # the benchmark's shape: 20.75 KB of records per node
    assert record_bytes(32, 32, 8) == 21248


def test_restatement_equals_the_compiled_rule(compiled):
    cases = [(b, n, m, p, g) for b, (n, m, p), g in itertools.product(BATCHES, SHAPES, BUDGETS)]
    _, _, got = compiled(cases)
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        assert g == streams(*c), c


def test_the_cases_that_matter(compiled):
    default, _, _ = compiled([])
    cases = [(10000, 32, 32, 8, default), (40000, 32, 32, 8, default), (4096, 32, 32, 8, default)]
    _, _, got = compiled(cases)
    assert got == [True, False, False]
    assert streams(10000, 32, 32, 8, default) and not streams(40000, 32, 32, 8, default) and not streams(4096, 32, 32, 8, default)
    sweep = [(b, n, m, p, g) for b, (n, m, p) in itertools.product(BATCHES, SHAPES) for g in (0, -1)]
    _, _, got = compiled(sweep)
    for c, g in zip(sweep, got):
        assert g == (c[4] == -1), c


@pytest.mark.parametrize("batch", [4096, 7000, 10000, 14000, 40000])
def test_monotone_in_the_budget_on_both_edges(compiled, batch):
    """Over growing positive budgets the decision is no, ..., no, yes, ..., yes, no, ..., no: it switches on once (the budget
    reaches R) and off once (the budget reaches R + C), and the two edges are where the restatement puts them."""
    budgets = list(range(1, 2049))
    _, _, got = compiled([(batch, 32, 32, 8, g) for g in budgets])
    on = [g for g, s in zip(budgets, got) if s]
    assert on and on == list(range(on[0], on[-1] + 1))
    R = batch * (record_bytes(32, 32, 8) + output_bytes(32, 32))
    C = batch * CRASH_DOUBLES * 8
    assert on[0] == -(-R // (1 << 20)) and on[-1] == (R + C - 1) >> 20
