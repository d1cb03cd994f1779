"""Planted nodes for the warm start of the mid-size classes (qpn_nodes_set_warm, csrc/qpn_warm_mid.hip): shared by
tests/test_warm_mid_host.py (the numpy twin with fits=) and tests/test_gpu_warm_mid.py (the kernel).

The shapes are the class corners of solve_cases.CELLS -- their nodes are solve_cases.cell_cases', built once per process and shared
with the tests of the cold routes -- plus (97, 64), the shape solve() sends for the leaders of the pair nets, and, for the host
test alone, (128, 128).  All ten families of solve_cases.FAMILIES, three nodes each, weak left out where min(n, m) < 3 (it needs
two inactive rows independent of the active ones).  The hints are warm_cases' makers, which ask nothing of the shape.
"""
from __future__ import annotations

import numpy as np

import solve_cases as SC

LEADERS = (97, 64)
CLASSES = ("s48", "wg", "wg2")
# the schedule thresholds of sweep_mid (csrc/qpn_capi_nodes.hip): a handle keeps a longest-first order beyond these many nodes
TILED = {"s48": (33, 33, 2050), "wg": (49, 49, 1030), "wg2": (65, 65, 260)}

_CACHE = {}


def extra_nodes(n, m, p=3, per=3, seed=31):
    """A shape that solve_cases.CELLS does not have: every family `per` times, one w for all (built once, left unchanged)."""
    if (n, m, p, per, seed) not in _CACHE:
        rng = np.random.default_rng([seed, n, m])
        w = rng.standard_normal(p)
        fams = tuple(f for f in SC.FAMILIES if not (f == "weak" and min(n, m) < 3))
        _CACHE[n, m, p, per, seed] = [SC.make_node(rng, n, m, f, p, w) for f in fams for _ in range(per)]
    return _CACHE[n, m, p, per, seed]


def shapes():
    """[(class, n, m, p, nodes)]: the corners of the three classes, and the leaders' shape in wg2."""
    out = []
    for cls in CLASSES:
        for n, m, p, nodes in SC.cell_cases(cls):
            out.append((cls, n, m, p, nodes))
            if (n, m) == (65, 65):
                out.append((cls, *LEADERS, 3, extra_nodes(*LEADERS)))
    return out


def shape(n, m):
    return next(s for s in shapes() if s[1:3] == (n, m))


def hinted_rows(z, n):
    """k of a hint: the multipliers that are not zero (a NaN counts: the kernel declines before it counts)."""
    return int(np.count_nonzero(np.asarray(z)[n:]))
