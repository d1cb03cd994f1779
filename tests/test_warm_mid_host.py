"""The host side of the warm start of the mid-size classes: the LDS rule, the numpy twin with fits=, and the switch of solve_level.

warm_mid_fits (level_batch's restatement of csrc/qpn_internal.h) meets the floors the interface promises -- every k <= min(n, 64)
for n <= 100, every k <= 32 up to n = 128 --, never admits k > n, and is monotone in k.  level_batch.warm_nodes_host with
fits=warm_mid_fits, on the planted nodes of tests/warm_mid_cases.py with their true hints, accepts the nodes inside the rule and no
others (without fits= it accepts them all: the rule is the only reason).  Through a spy engine, solve_level calls Nodes.set_warm
once per handle, and only when WARM_DUALS_ROUTE and WARM_DUALS_MID are both on.
"""
import re
import os

import numpy as np
import pytest

import solve_cases as SC
import warm_cases as WC
import warm_mid_cases as MC

import qpn_amd  # noqa: F401
from qpn_amd import level_batch
from qpn_amd.engine import colmajor
from oracle_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _abi(nodes):
    Q, R, qd, A, B, l, u = SC.stack(nodes)
    return [colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u]


def test_the_rule_meets_its_floors_and_is_monotone():
    fits = level_batch.warm_mid_fits
    for n in range(1, 129):
        admitted = [fits(n, k) for k in range(0, 130)]
        assert admitted[0]
        assert not any(admitted[n + 1:]), n                                    # k <= n
        assert all(a or not b for a, b in zip(admitted, admitted[1:])), n      # monotone: once out, out
        assert all(admitted[:min(n, 32) + 1]), n
        if n <= 100:
            assert all(admitted[:min(n, 64) + 1]), n
    assert not fits(128, 128) and not fits(5, -1)


def test_the_rule_restates_the_kernel_header():
    with open(os.path.join(ROOT, "quadraticprogramnetworks.jl_amd", "csrc", "qpn_internal.h")) as f:
        src = f.read()
    lds, fixed = re.search(r"kWarmMidLds = (\d+) \* 1024, kWarmMidFixed = (\d+);", src).groups()
    assert (int(lds) * 1024, int(fixed)) == (level_batch.WARM_MID_LDS, level_batch.WARM_MID_FIXED)
    assert "k >= 0 && k <= n && 8 * (k * (n | 1) + n * ((k + 1) | 1)) + kWarmMidFixed <= kWarmMidLds" in src


@pytest.mark.parametrize("n,m", [(48, 40), MC.LEADERS, (128, 100), (128, 128)])
def test_the_twin_accepts_what_the_rule_admits_and_nothing_else(n, m):
    nodes = MC.extra_nodes(n, m, per=2) if (n, m) == (128, 128) else MC.shape(n, m)[4]
    rng = np.random.default_rng([1, n, m])
    hints = np.stack([WC.true_hint(c, rng) for c in nodes])
    free = level_batch.warm_nodes_host(_abi(nodes), nodes[0]["w"], hints)
    assert free["accepted"].all(), [c["family"] for c, a in zip(nodes, free["accepted"]) if not a]
    res = level_batch.warm_nodes_host(_abi(nodes), nodes[0]["w"], hints, fits=level_batch.warm_mid_fits)
    inside = np.array([level_batch.warm_mid_fits(n, int(np.count_nonzero(c["side"]))) for c in nodes])
    assert np.array_equal(res["accepted"], inside), [(c["family"], int(np.count_nonzero(c["side"]))) for c in nodes]
    assert inside.all() == (n < 128), (n, m)                                  # kfull at n = 128 is beyond the rule
    for k in ("z", "status", "resid", "pivots", "active"):
        assert np.array_equal(res[k][inside], free[k][inside])
    assert np.array_equal(res["z"][~inside], hints[~inside]) and np.all(res["pivots"][~inside] == -1)


class _SpyHandle:
    """A resident handle served by the oracle (cold) and the twin (warm): Nodes.solve's interface, and a log of set_warm."""

    def __init__(self, eng, records):
        self.eng, self.records = eng, [np.array(a) for a in records]
        self.batch, self.n = self.records[2].shape
        self.m = self.records[5].shape[1]

    def set_warm(self, on=True):
        self.eng.set_warm_calls.append((self.n, self.m, self.batch, on))

    def solve(self, w, opts=None, want=("z", "resid", "pivots", "active"), out=None, x_out=None, warm=None):
        self.eng.hinted.append(warm is not None)
        cold = OracleEngine.solve_nodes(self.eng, *self.records, w)
        res = {k: np.array(cold[k]) for k in ("z", "status", "resid", "pivots")}
        if warm is not None:
            got = level_batch.warm_nodes_host(self.records, w, warm, fits=level_batch.warm_mid_fits)
            for k in res:
                res[k][got["accepted"]] = got[k][got["accepted"]]
        out = {} if out is None else out
        out.update(res)
        return out


class _SpyEngine(OracleEngine):
    def __init__(self):
        super().__init__()
        self.set_warm_calls, self.hinted, self.uploads = [], [], 0

    def upload_nodes(self, *records):
        self.uploads += 1
        return _SpyHandle(self, records)


@pytest.mark.parametrize("route,mid", [(False, False), (True, False), (False, True), (True, True)])
def test_solve_level_opts_in_only_under_both_switches(route, mid):
    import parent_cases as PC
    assert level_batch.WARM_DUALS_MID is False and level_batch.WARM_DUALS_ROUTE is False
    net, x, S = PC.kinked_pairs()
    followers = sorted(net.network_depth_map[2])
    level_batch.WARM_DUALS_ROUTE, level_batch.WARM_DUALS_MID = route, mid
    try:
        e = _SpyEngine()
        for _ in range(3):
            x = level_batch.solve_level(net, followers, x, engine=e)
    finally:
        level_batch.WARM_DUALS_ROUTE = level_batch.WARM_DUALS_MID = False
    if route and mid:
        assert len(e.set_warm_calls) == e.uploads > 0 and all(c[3] == 1 for c in e.set_warm_calls)     # once per handle
    else:
        assert e.set_warm_calls == []
    # the hint itself is WARM_DUALS_ROUTE's alone: passed from a handle's second sweep on, whatever WARM_DUALS_MID says
    assert any(e.hinted) == route and not any(e.hinted[:e.uploads])
