"""The row post-check of every node solve (QPN_ROW_POSTCHECK and its three parts, csrc/qpn_internal.h): the violation count of
check_avi_solution, the natural-map residual with a NaN turned into +inf, and the comp_indices mask, shifted by 4 for a GAVI row.
The macros are wrapped in a host program and run over the full grid of
    p, d     in {-inf, -1, -comp_tol, -check_tol/2, -0.0, 0, check_tol/2, comp_tol, 1, 1 + comp_tol/2, 1 + 2 comp_tol, inf, nan},
    (l, u)   in {(-inf, inf), (0, inf), (-inf, 1), (0, 1), (1, 1), (1, 1 + comp_tol/2), (inf, inf)},
    both kinds, and (check_tol, comp_tol) in {(1e-6, 1e-2), (0, 0), (1e-6, 1e300)}
-- 13 * 13 * 7 * 2 * 3 = 7098 rows -- and every row is compared, with equality, against
  * level_batch.node_postcheck, the Python twin: violation flag, residual bit for bit, mask;
  * the oracle's qpo_check_avi_solution and qpo_comp_indices: count and mask.  The oracle spells isapprox with the finiteness
    tests; the kernels' one spelling, (x == y) | (|x - y| <= ct), leaves them out: this is the check that the two agree.
The oracle takes a row as a one-row item and forms r = M z + q itself.  With M = 0 and q = r that reproduces (p, d) while the z
member is finite (or r is NaN anyway); an infinite z times the zero entry is NaN.  Such rows go in with the kinds' roles swapped
(the count does not look at the kind once p and d are told apart) or, when both members are infinite, with M = +-1 so that
M z + q is the wanted infinity; the r the oracle returns is compared with the wanted one on every row, so no row is checked on
other numbers than its own."""
import itertools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import qpn_amd  # noqa: F401
from qpn_amd import level_batch
from oracle import binding as oracle

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quadraticprogramnetworks.jl_amd", "csrc")
INF, NAN = float("inf"), float("nan")
TOLS = ((1e-6, 1e-2), (0.0, 0.0), (1e-6, 1e300))


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def grid():
    rows = []
    for check_tol, ct in TOLS:
        vals = (-INF, -1.0, -ct, -check_tol / 2, -0.0, 0.0, check_tol / 2, ct, 1.0, 1.0 + ct / 2, 1.0 + 2 * ct, INF, NAN)
        bounds = ((-INF, INF), (0.0, INF), (-INF, 1.0), (0.0, 1.0), (1.0, 1.0), (1.0, 1.0 + ct / 2), (INF, INF))
        for p, d, (l, u), kind in itertools.product(vals, vals, bounds, (0, 1)):
            rows.append((p, d, l, u, kind, check_tol, ct))
    return rows


ROWS = grid()


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """(count, residual bits, mask) of every row of ROWS from the C++ text, one run."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc) and not shutil.which("hipcc"):
        pytest.fail("hipcc not found: the package cannot be built here either")
    tmp = tmp_path_factory.mktemp("postcheck")
    src = tmp / "postcheck.hip"
    src.write_text('#include "qpn_internal.h"\n#include <cmath>\n#include <cstdio>\n#include <cstring>\n'
                   "using std::isnan;      // (host code: the unqualified name the macros use is a device function otherwise)\n"
                   "static double dbl(unsigned long long b) { double x; memcpy(&x, &b, 8); return x; }\n"
                   "int main() {\n"
                   "    unsigned long long v[4], t[2]; int kind;\n"
                   '    while (scanf("%llx %llx %llx %llx %d %llx %llx", &v[0], &v[1], &v[2], &v[3], &kind, &t[0], &t[1]) == 7) {\n'
                   "        const double p = dbl(v[0]), d = dbl(v[1]), l = dbl(v[2]), u = dbl(v[3]), tol = dbl(t[0]), ct = dbl(t[1]);\n"
                   "        int bad = 0; double e; unsigned mask;\n"
                   "        QPN_ROW_POSTCHECK(bad, e, mask, p, d, l, u, kind, tol, ct);\n"
                   "        // the parts, as check_avi_kernel and comp_indices_kernel use them, are the same text\n"
                   "        int bad2 = 0; unsigned m2;\n"
                   "        QPN_ROW_VIOLATIONS(bad2, p, d, l, u, tol);\n"
                   "        QPN_ROW_MASK(m2, p, d, l, u, ct);\n"
                   "        if (bad != bad2 || mask != m2 << (kind ? 4 : 0)) return 3;\n"
                   "        unsigned long long eb; memcpy(&eb, &e, 8);\n"
                   '        printf("%d %llx %u\\n", bad, eb, mask);\n'
                   "    }\n"
                   "    return 0;\n}\n")
    exe = tmp / "postcheck"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)])
    text = "".join("%x %x %x %x %d %x %x\n" % (bits(p), bits(d), bits(l), bits(u), kind, bits(tol), bits(ct))
                   for p, d, l, u, kind, tol, ct in ROWS)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    got = [(int(a), int(b, 16), int(c)) for a, b, c in (line.split() for line in out if line)]
    assert len(got) == len(ROWS)
    return got


def test_the_grid_is_the_full_grid():
    assert len(ROWS) == 13 * 13 * 7 * 2 * 3 == 7098
    assert all(np.isfinite(ct) for _, _, _, _, _, _, ct in ROWS)            # the precondition of qpn_approx


def test_equals_the_python_twin(compiled):
    """node_postcheck on a one-row node.  It takes a node's rows as [free STD x n | GAVI x m]: a GAVI row is the node n = 0, m = 1
    with z = d, r = p; an STD row with other bounds than (-inf, inf) does not exist in a node, so an STD row goes in as the GAVI
    row of the same (p, d, l, u) -- the arithmetic does not look at the kind -- and its mask comes back shifted: >> 4.  The free
    STD rows also go in as they are (n = 1, m = 0)."""
    free = 0
    for (p, d, l, u, kind, tol, ct), (bad, eb, mask) in zip(ROWS, compiled):
        row = (p, d, l, u, kind, tol, ct)
        rbad, rres, rmask = level_batch.node_postcheck(np.array([d]), np.array([p]), np.array([l]), np.array([u]), 0, tol, ct)
        assert (bad > 0) == rbad, row
        assert eb == bits(rres), row
        assert mask == (int(rmask[0]) if kind else int(rmask[0]) >> 4), row
        if kind == 0 and l == -INF and u == INF:
            fbad, fres, fmask = level_batch.node_postcheck(np.array([p]), np.array([d]), np.zeros(0), np.zeros(0), 1, tol, ct)
            assert ((bad > 0), eb, mask) == (fbad, bits(fres), int(fmask[0])), row
            free += 1
    assert free == 13 * 13 * 3


def oracle_item(p, d, kind):
    """(kind, M, q, z) of the one-row item on which the oracle sees exactly (p, d): z is the member its kind reads from z, M z + q
    the other one."""
    for k in (kind, 1 - kind):
        a, c = (d, p) if k else (p, d)              # a: read from z;  c: formed as M a + q
        if np.isfinite(a) or np.isnan(c):
            return k, 0.0, c, a                      # fma(0, a, c) = c (NaN if a is not finite: wanted then)
        if np.isinf(a) and np.isinf(c):
            return k, (1.0 if (a > 0) == (c > 0) else -1.0), c, a
    raise AssertionError((p, d))


def test_equals_the_oracle(compiled):
    # (equal as numbers: fma(0, a, -0.0) is +0.0 for a > 0, and no comparison of the post-check tells the two zeros apart)
    same = lambda x, y: x == y or (np.isnan(x) and np.isnan(y))
    for (p, d, l, u, kind, tol, ct), (bad, _, mask) in zip(ROWS, compiled):
        row = (p, d, l, u, kind, tol, ct)
        k, M, q, z = oracle_item(p, d, kind)
        _, deg, r = oracle.check_avi_solution(np.array([[M]]), [q], [l], [u], [z], kind=[k], tol=tol)
        op, od = (r[0], z) if k else (z, r[0])
        assert same(op, p) and same(od, d), row         # the oracle counted on this row's own numbers
        assert deg == bad, row
        omask = oracle.comp_indices([p], [d], [l], [u], tol=ct, shift=4 if kind else 0)
        assert int(omask[0]) == mask, row
