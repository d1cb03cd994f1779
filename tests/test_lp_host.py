"""polyhedra.solve_lps_host -- the numpy twin of qpn_solve_lps and the normative statement of its method -- against an independent
LP solver (scipy HiGHS) on a seeded family, with every certificate (multipliers, Farkas vector, ray) checked in plain numpy on the
unscaled data, and on hand cases.  tests/lp_cases.py holds the family and the checks (the GPU suite shares them)."""
import importlib.util
import os

import numpy as np
import pytest
from scipy.optimize import linprog

import qpn_amd  # noqa: F401
from qpn_amd import polyhedra
from qpn_amd.engine import colmajor

import goldenio
import lp_cases
from lp_cases import FAILURE, INFEASIBLE, ITER_LIMIT, OPTIMAL, UNBOUNDED

INF = np.inf


def _highs(c, A, l, u):
    """-> (status of the ABI, objective) by HiGHS.  Its presolve may answer "infeasible or unbounded": a zero-objective solve of
    the same rows tells the two apart."""
    rows, rhs = [], []
    for i in range(A.shape[0]):
        if np.isfinite(u[i]): rows.append(A[i]); rhs.append(u[i])
        if np.isfinite(l[i]): rows.append(-A[i]); rhs.append(-l[i])
    kw = dict(A_ub=np.array(rows), b_ub=np.array(rhs)) if rows else {}
    free = [(None, None)] * A.shape[1]
    res = linprog(c, bounds=free, method="highs", **kw)
    if res.status == 0:
        return OPTIMAL, float(res.fun)
    feas = linprog(np.zeros(A.shape[1]), bounds=free, method="highs", **kw)
    assert feas.status in (0, 2), feas.message
    if feas.status == 2:
        return INFEASIBLE, None
    assert res.status in (2, 3), res.message             # (a feasible LP that HiGHS does not solve: unbounded)
    return UNBOUNDED, None


@pytest.mark.parametrize("block", range(6))
def test_twin_agrees_with_highs_on_the_seeded_family(block):
    counts = {OPTIMAL: 0, INFEASIBLE: 0, UNBOUNDED: 0}
    for seed in range(100 * block, 100 * block + 100):
        A, l, u, c, row = lp_cases.family_case(seed)
        kw = dict(cost=c[None]) if row is None else dict(obj_row=[row[0]], obj_sign=[row[1]])
        got = polyhedra.solve_lps_host(colmajor(A[None]), l[None], u[None], [0], **kw)
        want, fun = _highs(c, A, l, u)
        st = int(got["status"][0])
        assert st == want, (seed, st, want)
        if want == OPTIMAL:
            assert abs(got["obj"][0] - fun) <= 1e-8 * max(1.0, abs(fun)), (seed, got["obj"][0], fun)
        lp_cases.check_certificates(A, l, u, c, {k: v[0] for k, v in got.items()})
        assert got["iters"][0] < 50 * sum(A.shape) + 100
        counts[st] += 1
    assert all(v >= 5 for v in counts.values()), counts     # every outcome occurs in every block of seeds


def test_row_objective_equals_the_cost_it_names():
    A, l, u, c, row = lp_cases.family_case(2)                # (seed % 3 == 2: a row objective)
    assert row is not None
    a = polyhedra.solve_lps_host(colmajor(A[None]), l[None], u[None], [0], obj_row=[row[0]], obj_sign=[row[1]])
    b = polyhedra.solve_lps_host(colmajor(A[None]), l[None], u[None], [0], cost=c[None])
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _solve(A, l, u, c, **opts):
    A = np.atleast_2d(np.asarray(A, dtype=np.float64)); l = np.asarray(l, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    got = polyhedra.solve_lps_host(colmajor(A[None]), l[None], u[None], [0], cost=c[None], opts=opts or None)
    got = {k: v[0] for k, v in got.items()}
    lp_cases.check_certificates(A, l, u, c, got)
    return got


def test_hand_cases():
    # r < d: one row in two variables; bounded along the row, unbounded across it
    g = _solve([[1.0, 1.0]], [1.0], [3.0], [1.0, 1.0])
    assert g["status"] == OPTIMAL and g["obj"] == 1.0
    assert _solve([[1.0, 1.0]], [1.0], [3.0], [1.0, -1.0])["status"] == UNBOUNDED
    # r = d: a box corner
    g = _solve(np.eye(2), [-1.0, -2.0], [1.0, 2.0], [1.0, -1.0])
    assert g["status"] == OPTIMAL and np.array_equal(g["x"], [-1.0, 2.0]) and g["obj"] == -3.0
    # duplicate rows: the tighter copy decides; contradictory copies are infeasible
    g = _solve([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0]], [0.0, 0.5, 0.0], [2.0, 2.0, 1.0], [1.0, 1.0])
    assert g["status"] == OPTIMAL and abs(g["obj"] - 0.5) <= 1e-12
    assert _solve([[1.0, 0.0], [1.0, 0.0]], [1.0, -INF], [INF, 0.0], [0.0, 0.0])["status"] == INFEASIBLE
    # a zero row inside its bounds is inert; outside them it settles the job, with the unit Farkas vector
    g = _solve([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]], [-1.0, 0.0, 0.0], [1.0, 1.0, 1.0], [1.0, 1.0])
    assert g["status"] == OPTIMAL and g["obj"] == 0.0
    g = _solve([[0.0, 0.0], [1.0, 0.0]], [1.0, 0.0], [2.0, 1.0], [1.0, 0.0])
    assert g["status"] == INFEASIBLE and np.array_equal(g["lam"], [-1.0, 0.0]) and g["iters"] == 0
    g = _solve([[0.0, 0.0], [1.0, 0.0]], [-2.0, 0.0], [-1.0, 1.0], [1.0, 0.0])
    assert g["status"] == INFEASIBLE and np.array_equal(g["lam"], [1.0, 0.0])
    # a free row changes nothing
    g = _solve([[1.0, 2.0], [1.0, 0.0], [0.0, 1.0]], [-INF, 0.0, 0.0], [INF, 1.0, 1.0], [-1.0, -1.0])
    assert g["status"] == OPTIMAL and g["obj"] == -2.0 and g["lam"][0] == 0.0
    # equality rows: a point, and a line the objective runs along
    g = _solve([[1.0, 1.0], [1.0, -1.0]], [2.0, 0.0], [2.0, 0.0], [3.0, 1.0])
    assert g["status"] == OPTIMAL and np.allclose(g["x"], [1.0, 1.0], atol=1e-12)
    assert _solve([[1.0, 1.0]], [2.0], [2.0], [1.0, -1.0])["status"] == UNBOUNDED
    assert _solve([[1.0, 1.0], [2.0, 2.0]], [2.0, 5.0], [2.0, 5.0], [1.0, 0.0])["status"] == INFEASIBLE
    # the iteration limit: the answer is the point reached, nothing is claimed
    A, l, u, c, _ = lp_cases.family_case(18)
    full = _solve(A, l, u, c)
    cut = _solve(A, l, u, c, max_iters=3)
    assert full["iters"] > 3 and cut["status"] == ITER_LIMIT and cut["iters"] == 3 and not cut["lam"].any()


def test_pinned_polyhedron_row_extremes():
    """x1 >= 1, x1 + x2 <= 1, x2 >= 0 pins x = (1, 0): every row's minimum and maximum coincide (tests/test_polyhedra.py's case)."""
    A = np.array([[1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]); l = np.array([1.0, -INF, 0.0]); u = np.array([INF, 1.0, INF])
    rows = np.repeat(np.arange(3), 2); sign = np.tile([1, -1], 3)
    got = polyhedra.solve_lps_host(colmajor(A[None]), l[None], u[None], np.zeros(6, np.int64), obj_row=rows, obj_sign=sign)
    assert np.all(got["status"] == OPTIMAL)
    assert np.allclose(got["obj"] * sign, [1.0, 1.0, 1.0, 1.0, 0.0, 0.0], atol=1e-12)
    assert np.allclose(got["x"], np.tile([1.0, 0.0], (6, 1)), atol=1e-12)
    for t in range(6):
        lp_cases.check_certificates(A, l, u, sign[t] * A[rows[t]], {k: v[t] for k, v in got.items()})


def test_indices_out_of_range_answer_failure_and_zeros():
    A = np.eye(2)[None]; l = np.zeros((1, 2)); u = np.ones((1, 2))
    got = polyhedra.solve_lps_host(colmajor(A), l, u, [0, 1, -1, 0], obj_row=[0, 0, 0, 2], obj_sign=[1, 1, 1, 1])
    assert list(got["status"]) == [OPTIMAL, FAILURE, FAILURE, FAILURE]
    assert not got["x"][1:].any() and not got["lam"][1:].any() and not got["iters"][1:].any()


def test_the_twins_answer_what_the_recorded_commit_answered():
    """tests/golden/lp_twin_record.json holds the digests of every output of solve_lps_host, issubset_pairs_host and
    implicit_bounds_host on the families of the GPU suites, written by tests/golden/make_lp_twin_record.py from the commit before
    the twins were last edited: the kernels are held bit-equal to the twins, this holds the twins bit-equal to themselves."""
    spec = importlib.util.spec_from_file_location("make_lp_twin_record", os.path.join(goldenio.GOLD, "make_lp_twin_record.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    want = goldenio.load("lp_twin_record.json")["cases"]
    got = maker.record(polyhedra)
    assert sorted(got) == sorted(want) and len(want) == 40
    for name in sorted(want):
        assert got[name]["histograms"] == want[name]["histograms"], name
        assert got[name]["outputs"] == want[name]["outputs"], name


# ---- the host functions on the LP route (an oracle engine that also has the twin as solve_lps) against the node-AVI route --------
def _twin_engine():
    from oracle_engine import OracleEngine

    class TwinEngine(OracleEngine):
        lp_calls = 0                                             # (the base class counts attribute reads, `hasattr` probes included)

        def solve_lps(self, Ac, l, u, poly_of, cost=None, obj_row=None, obj_sign=None, opts=None):
            type(self).lp_calls += 1
            return polyhedra.solve_lps_host(Ac, l, u, poly_of, cost=cost, obj_row=obj_row, obj_sign=obj_sign, opts=opts)

    return TwinEngine(), OracleEngine()


def _random_polys(seed, count, dmax=5, mmax=8):
    """(tests/test_polyhedra.py's generator, stated again)"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(count):
        d = int(rng.integers(1, dmax + 1)); m = int(rng.integers(1, mmax + 1))
        A = rng.standard_normal((m, d))
        x0 = rng.standard_normal(d)
        c = A @ x0
        l = c - np.abs(rng.standard_normal(m)) - 0.05; u = c + np.abs(rng.standard_normal(m)) + 0.05
        l = np.where(rng.random(m) < 0.3, -np.inf, l); u = np.where(rng.random(m) < 0.3, np.inf, u)
        if t % 3 == 1 and m >= 2:
            A[1] = A[0]; l[0], u[0] = -np.inf, c[0] - 1.0; l[1], u[1] = c[0] + 1.0, np.inf
        if t % 3 == 2 and m >= 2:
            u[0] = l[0] = c[0]
        out.append((A, l, u))
    return out


def test_implicit_bounds_and_exemplar_slack_take_the_lp_route():
    twin, plain = _twin_engine()
    polys = _random_polys(11, 40)
    empty, example, eps = polyhedra.exemplar_slack_batch(polys, twin, tol=1e-4)
    empty0, _, eps0 = polyhedra.exemplar_slack_batch(polys, plain, tol=1e-4)
    assert twin.lp_calls > 0 and twin.calls["solve_nodes"] == 0
    assert np.array_equal(empty, empty0) and empty.any() and not empty.all() and np.all(np.abs(eps - eps0) <= 1e-8)
    for (A, l, u), e, x in zip(polys, empty, example):
        assert (x is None) == bool(e)
        if not e:
            assert np.all(A @ x >= l - 2e-4) and np.all(A @ x <= u + 2e-4)
    keep = [p for p, e in zip(polys, empty) if not e]
    pinned = (np.array([[1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]), np.array([1.0, -INF, 0.0]), np.array([INF, 1.0, INF]))
    n0, s0, p0 = twin.lp_calls, twin.calls["solve_nodes"], plain.calls["solve_nodes"]
    got = polyhedra.implicit_bounds_batch(keep + [pinned], twin)
    want = polyhedra.implicit_bounds_batch(keep + [pinned], plain)
    shapes = {A.shape for A, l, u in keep + [pinned] if not np.all(np.isclose(l, u, rtol=0, atol=1e-4) | (l == u))}
    assert twin.lp_calls - n0 == len(shapes)          # one call per shape ...
    # ... and the emptiness projection alone on the node solver (the oracle engine counts reads of the attribute: the probe too)
    assert twin.calls["solve_nodes"] - s0 == 2 < plain.calls["solve_nodes"] - p0
    for (eq, vals), (eq0, vals0) in zip(got, want):
        assert np.array_equal(eq, eq0) and np.all(np.abs(vals[eq] - vals0[eq]) <= 1e-7)
    assert list(got[-1][0]) == [True, True, True] and np.allclose(got[-1][1], [1.0, 1.0, 0.0], atol=1e-9)
