"""polyhedra.implicit_bounds_host, the numpy twin and normative statement of qpn_implicit_bounds (one job per polyhedron), without a
GPU: the seeded family of tests/implicit_cases.py against HiGHS, hand cases, implicit_bounds_batch(route="polyhedron") and
check_convexity_items on an engine that has `implicit_bounds` (a spy built from the twin over the oracle engine) against the route
of the jobs, and the new symbol with its ctypes signature."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
from scipy.optimize import linprog

import implicit_cases
import lp_cases
from implicit_cases import BY_EXTREMES, BY_POINTS, EMPTY, EXPLICIT, FAILURE, IMPLICIT, ITER_LIMIT, OK, PINNED, UNBOUNDED, UNDECIDED

from qpn_amd import polyhedra, polyhedra_host
from qpn_amd.engine import colmajor

INF = np.inf
TOL = 1e-4
SHAPES = [(3, 2), (8, 4), (16, 8), (24, 12)]
SEEDS = list(range(60))


def _twin(A, l, u, **kw):
    return polyhedra.implicit_bounds_host(colmajor(A), l, u, **kw)


def _one(A, l, u, **kw):
    A = np.atleast_2d(np.asarray(A, dtype=np.float64)); l = np.asarray(l, dtype=np.float64); u = np.asarray(u, dtype=np.float64)
    return {k: v[0] for k, v in _twin(A[None], l[None], u[None], **kw).items()}


def _explicit(l, u, tol=TOL):
    with np.errstate(invalid="ignore"):
        return (np.abs(l - u) <= tol) | (l == u)


def _highs(A, l, u):
    """One polyhedron by HiGHS, by the recipe of tests/test_lp_host.py for its "infeasible or unbounded" answer (a zero-objective
    solve of the same rows tells the two apart).  -> None when it is infeasible, else (lo [r], hi [r]) over the rows that are no
    explicit equalities: the extremes of a_i'x, -+inf where unbounded, NaN where HiGHS gives no answer (and on explicit rows)."""
    r, d = A.shape
    rows, rhs = [], []
    for i in range(r):
        if np.isfinite(u[i]): rows.append(A[i]); rhs.append(u[i])
        if np.isfinite(l[i]): rows.append(-A[i]); rhs.append(-l[i])
    kw = dict(A_ub=np.array(rows), b_ub=np.array(rhs)) if rows else {}
    free = [(None, None)] * d
    feas = linprog(np.zeros(d), bounds=free, method="highs", **kw)
    assert feas.status in (0, 2), feas.message
    if feas.status == 2:
        return None
    ext = np.full((2, r), np.nan)
    for i in np.nonzero(~_explicit(l, u))[0]:
        for side, sg in enumerate((1.0, -1.0)):
            res = linprog(sg * A[i], bounds=free, method="highs", **kw)
            if res.status == 0:
                ext[side, i] = sg * float(res.fun)
            elif res.status in (2, 3):                      # (feasible, and HiGHS does not solve it: unbounded)
                ext[side, i] = -sg * INF
    return ext[0], ext[1]


@functools.lru_cache(maxsize=None)
def _family(shape):
    """(the batch, the twin's answers in both modes, HiGHS's answer per polyhedron) of one shape: computed once, shared by the
    tests, left unchanged."""
    batch = implicit_cases.family_batch(shape, SEEDS)
    return batch, _twin(*batch, tol=TOL), _twin(*batch, tol=TOL, all_extremes=True), [_highs(*(a[k] for a in batch)) for k in range(len(SEEDS))]


@pytest.mark.parametrize("shape", SHAPES)
def test_the_twin_against_highs(shape):
    (A, l, u), fast, full, ref = _family(shape)
    r = shape[0]
    extremes = left_out = narrow = planted = 0
    for k, ext in enumerate(ref):
        if ext is None:
            for got in (fast, full):
                assert got["status"][k] == EMPTY and got["fail_row"][k] == -1, (shape, k)
                assert np.all(got["how"][k][~_explicit(l[k], u[k])] == UNDECIDED)
            continue
        assert fast["status"][k] == OK and full["status"][k] == OK, (shape, k, fast["status"][k], full["status"][k])
        ex = _explicit(l[k], u[k])
        for i in range(r):
            if ex[i]:
                for got in (fast, full):
                    assert got["eq"][k, i] == 1 and got["how"][k, i] == EXPLICIT and got["vals"][k, i] == 0.5 * (l[k, i] + u[k, i])
                continue
            lo, hi = ext[0][i], ext[1][i]
            extremes += 2
            known = 0
            for name, v in (("lo", lo), ("hi", hi)):
                if np.isnan(v):
                    left_out += 1
                    continue
                known += 1
                g = full[name][k, i]
                if np.isinf(v):
                    assert g == v, (shape, k, i, name, g, v)                      # +-inf exactly where HiGHS says unbounded
                else:
                    assert abs(g - v) <= 1e-8 * max(1.0, abs(v)), (shape, k, i, name, g, v)
            if known < 2:
                continue
            if np.isfinite(lo) and np.isfinite(hi) and TOL / 10 < hi - lo < 10 * TOL:
                narrow += 1
                continue
            want = bool(np.isfinite(lo) and np.isfinite(hi) and abs(lo - hi) <= TOL)
            for got in (fast, full):
                assert bool(got["eq"][k, i]) == want, (shape, k, i, lo, hi, got["how"][k, i])
                if want:
                    assert abs(got["vals"][k, i] - 0.5 * (lo + hi)) <= 1e-7 and got["how"][k, i] == IMPLICIT
                else:
                    assert got["vals"][k, i] == INF
            planted += want and i >= r - 2
    assert narrow == 0                                       # no row's range lies near the tolerance
    assert left_out <= 0.01 * extremes, (left_out, extremes)
    if r >= 4:
        feasible_even = sum(1 for k, ext in enumerate(ref) if ext is not None and SEEDS[k] % 2 == 0)
        assert planted == 2 * feasible_even > 0              # both rows of every planted equality are found


def test_every_outcome_occurs_and_points_save_lps():
    seen, saved = set(), 0
    for shape in SHAPES:
        (A, l, u), fast, full, ref = _family(shape)
        seen |= set(fast["how"].ravel().tolist())
        assert BY_POINTS not in full["how"] and not set(fast["status"].tolist()) - {OK, EMPTY}
        ok = fast["status"] == OK
        assert np.all(fast["lps"][ok] <= full["lps"][ok])
        saved += int((full["lps"][ok] - fast["lps"][ok]).sum())
        # lo / hi hold a number exactly where an LP computed it
        free = ~_explicit(l, u) & ok[:, None]
        assert not np.isnan(full["lo"][free]).any() and not np.isnan(full["hi"][free]).any()
        assert np.isnan(full["lo"][~free]).all() and np.isnan(fast["hi"][fast["how"] == BY_POINTS]).all()
        assert np.array_equal(full["lps"][ok], 1 + 2 * free.sum(1)[ok])
    # (the family has no explicit equality: the hand cases and the host routes have them)
    assert seen == {UNDECIDED, IMPLICIT, BY_POINTS, BY_EXTREMES, UNBOUNDED} and saved > 0


def test_hand_cases():
    # x1 >= 1, x1 + x2 <= 1, x2 >= 0 pins x = (1, 0)
    for every in (False, True):
        got = _one(*PINNED, all_extremes=every)
        assert got["status"] == OK and got["eq"].tolist() == [1, 1, 1] and np.allclose(got["vals"], [1.0, 1.0, 0.0], atol=1e-12)
        assert got["how"].tolist() == [IMPLICIT] * 3 and got["lps"] == 7 and got["fail_row"] == -1
    # a free row: unbounded both ways; in the default mode the minimum settles it
    A = np.array([[1.0, 0.0], [0.0, 1.0]]); l = np.array([-INF, 0.0]); u = np.array([INF, 1.0])
    got = _one(A, l, u)
    assert got["status"] == OK and got["how"][0] == UNBOUNDED and got["lo"][0] == -INF and np.isnan(got["hi"][0])
    assert got["eq"].tolist() == [0, 0] and got["vals"].tolist() == [INF, INF]
    got = _one(A, l, u, all_extremes=True)
    assert got["how"].tolist() == [UNBOUNDED, BY_EXTREMES] and got["lo"].tolist() == [-INF, 0.0] and got["hi"].tolist() == [INF, 1.0]
    # a one-row empty set: by crossed bounds (no LP is started) and by an all-zero row; two contradictory rows by the Farkas vector
    got = _one([[1.0]], [1.0], [0.0])
    assert got["status"] == EMPTY and got["how"].tolist() == [UNDECIDED] and got["lps"] == 0 and got["fail_row"] == -1
    got = _one([[0.0, 0.0]], [1.0], [2.0])
    assert got["status"] == EMPTY and got["iters"] == 0 and got["lps"] == 1 and got["vals"].tolist() == [INF]
    got = _one([[1.0, 0.0], [1.0, 0.0]], [-INF, 1.0], [-1.0, INF])
    assert got["status"] == EMPTY and got["lps"] == 1 and got["how"].tolist() == [UNDECIDED] * 2 and got["eq"].tolist() == [0, 0]
    # an all-explicit polyhedron runs the feasibility solve alone
    got = _one(np.eye(2), [1.0, 2.0], [1.0, 2.0 + 5e-5])
    assert got["status"] == OK and got["lps"] == 1 and got["how"].tolist() == [EXPLICIT] * 2 and got["vals"].tolist() == [1.0, 2.0 + 2.5e-5]
    assert np.isnan(got["lo"]).all() and np.isnan(got["hi"]).all()
    # ... and an empty one of them is still EMPTY
    got = _one([[1.0], [1.0]], [1.0, 2.0], [1.0, 2.0])
    assert got["status"] == EMPTY and got["eq"].tolist() == [1, 1]


def test_the_iteration_limit_names_its_row():
    """max_iters = 1 on the family at 16 x 8: where the feasibility solve ends within one step, the first objective that needs two
    ends the polyhedron and fail_row names it; the rows after it keep the answers of the full run, those from it on are undecided."""
    (A, l, u), full, _, _ = _family((16, 8))
    cut = _twin(A, l, u, tol=TOL, opts=dict(max_iters=1))
    named = np.nonzero((cut["status"] == ITER_LIMIT) & (cut["fail_row"] >= 0))[0]
    assert named.size >= 5
    for k in named:
        i = int(cut["fail_row"][k])
        assert i < 16 and full["status"][k] == OK and not _explicit(l[k], u[k])[i]
        assert np.array_equal(cut["how"][k, i + 1:], full["how"][k, i + 1:]) and np.array_equal(cut["eq"][k, i + 1:], full["eq"][k, i + 1:])
        assert np.all(cut["how"][k, :i + 1] == UNDECIDED) and not cut["eq"][k, :i + 1].any() and np.all(cut["vals"][k, :i + 1] == INF)
        assert 2 <= cut["lps"][k] <= full["lps"][k] and cut["iters"][k] <= cut["lps"][k]      # one step per solve at the most
    # a feasibility solve that needs more than one step: ITER_LIMIT without a row
    early = np.nonzero((cut["status"] == ITER_LIMIT) & (cut["fail_row"] == -1))[0]
    for k in early:
        assert cut["lps"][k] == 1 and cut["iters"][k] == 1 and np.all(cut["how"][k] == UNDECIDED)
    # a polyhedron that ends within the limit keeps its answer
    same = np.nonzero(cut["status"] != ITER_LIMIT)[0]
    assert all(np.array_equal(cut[key][same], full[key][same], equal_nan=True) for key in ("status", "eq", "vals", "lo", "hi", "lps"))


def test_steps_1_to_8_do_not_see_crossed_bounds():
    """Why crossed bounds are settled before the LP: the simplex keeps a nonbasic row at one of its bounds and never compares the
    two, so on {1 <= x <= 0} with c = 0 the loop ends OPTIMAL and only step 9's check objects (FAILURE, not INFEASIBLE)."""
    A = np.array([[1.0]]); l = np.array([1.0]); u = np.array([0.0])
    o = dict(polyhedra.LP_DEFAULT_OPTS)
    S = polyhedra_host._lp_setup(A, l, u, np.zeros(1), o)
    assert S.zbad is None and polyhedra_host._lp_loop(S) == polyhedra.LP_OPTIMAL
    got = polyhedra.solve_lps_host(colmajor(A[None]), l[None], u[None], [0], cost=np.zeros((1, 1)))
    assert got["status"][0] == polyhedra.LP_FAILURE
    assert _one(A, l, u)["status"] == EMPTY


def test_point_refutation_on_the_bounded_polytopes():
    """Default mode on bounded_batch 48 x 24: fewer LPs than rows, every row refuted, the same verdicts as by the extremes."""
    A, l, u = lp_cases.bounded_batch(100, 2, 48, 24)
    fast = _twin(A, l, u, tol=1e-6)
    full = _twin(A, l, u, tol=1e-6, all_extremes=True)
    assert np.all(fast["status"] == OK) and np.all(fast["lps"] < 48) and np.all(full["lps"] == 97)
    assert np.array_equal(fast["eq"], full["eq"]) and not fast["eq"].any()
    assert (fast["how"] == BY_POINTS).sum() > 48 and np.all(full["how"] == BY_EXTREMES)
    assert fast["iters"].sum() < full["iters"].sum()


# ---- the host routes on an engine that has implicit_bounds ---------------------------------------------------------------------
def make_spy():
    from oracle_engine import OracleEngine

    class Spy(OracleEngine):
        """The oracle engine with solve_lps and implicit_bounds made from the twins; the calls are counted where they arrive
        (the base class counts reads of the attributes, probes included)."""

        def __init__(self):
            super().__init__()
            self.shapes = []                                # (r, d) per implicit_bounds call
            self.node_solves = self.lp_calls = 0

        def solve_nodes(self, *a, **k):
            self.node_solves += 1
            return OracleEngine.solve_nodes(self, *a, **k)

        def solve_lps(self, Ac, l, u, poly_of, cost=None, obj_row=None, obj_sign=None, opts=None):
            self.lp_calls += 1
            return polyhedra.solve_lps_host(Ac, l, u, poly_of, cost=cost, obj_row=obj_row, obj_sign=obj_sign, opts=opts)

        def implicit_bounds(self, Ac, l, u, tol=1e-4, all_extremes=False, opts=None):
            self.shapes.append((Ac.shape[2], Ac.shape[1]))
            return polyhedra.implicit_bounds_host(Ac, l, u, tol=tol, all_extremes=all_extremes, opts=opts)

    return Spy()


def _random_polys(seed, count, dmax=5, mmax=8):
    """(tests/test_lp_host.py's generator, stated again)"""
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


def test_implicit_bounds_batch_on_the_spy_engine():
    polys = _random_polys(11, 40)
    spy = make_spy()
    empty, _, _ = polyhedra.exemplar_slack_batch(polys, spy, tol=1e-4)
    keep = [p for p, e in zip(polys, empty) if not e] + [PINNED]
    assert len(keep) >= 20
    spy = make_spy()
    got = polyhedra.implicit_bounds_batch(keep, spy, route="polyhedron")
    assert spy.node_solves == 0 and spy.lp_calls == 0
    assert sorted(spy.shapes) == sorted({A.shape for A, _, _ in keep})        # one call per shape
    want = polyhedra.implicit_bounds_batch(keep, spy, route="jobs")
    assert spy.node_solves > 0 and spy.lp_calls > 0
    for (eq, vals), (eq0, vals0) in zip(got, want):
        assert eq.dtype == bool and np.array_equal(eq, eq0) and np.all(np.abs(vals[eq] - vals0[eq]) <= 1e-7)
        assert np.all(vals[~eq] == INF)
    assert list(got[-1][0]) == [True, True, True] and np.allclose(got[-1][1], [1.0, 1.0, 0.0], atol=1e-9)
    assert any(eq.any() for eq, _ in got[:-1])
    # the default route is the jobs'; an engine without the method keeps it whatever is asked
    from oracle_engine import OracleEngine
    plain = polyhedra.implicit_bounds_batch(keep[-3:], OracleEngine(), route="polyhedron")
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(plain, want[-3:]))
    spy = make_spy()
    polyhedra.implicit_bounds_batch(keep[-3:], spy)
    assert not spy.shapes and spy.lp_calls > 0
    assert polyhedra.implicit_bounds_batch([], spy, route="polyhedron") == []
    with pytest.raises(ValueError):
        polyhedra.implicit_bounds_batch(keep[-3:], spy, route="rows")


def test_the_polyhedron_route_raises_like_the_jobs():
    spy = make_spy()
    crossed = (np.array([[1.0]]), np.array([1.0]), np.array([0.0]))
    with pytest.raises(RuntimeError, match=r"Empty set \(polyhedron 1\)"):
        polyhedra.implicit_bounds_batch([PINNED, crossed], spy, route="polyhedron")
    empty = (np.array([[1.0, 0.0], [1.0, 0.0]]), np.array([-INF, 1.0]), np.array([-1.0, INF]))   # x1 <= -1 and x1 >= 1
    with pytest.raises(RuntimeError, match=r"Empty set \(polyhedron 2\)"):
        polyhedra.implicit_bounds_batch([PINNED, PINNED, empty, PINNED, empty], spy, route="polyhedron")
    with pytest.raises(RuntimeError, match=r"Empty set \(polyhedron 2\)"):
        polyhedra.implicit_bounds_batch([PINNED, PINNED, empty, PINNED, empty], spy, route="jobs")

    class Cut(type(spy)):
        def implicit_bounds(self, Ac, l, u, tol=1e-4, all_extremes=False, opts=None):
            return polyhedra.implicit_bounds_host(Ac, l, u, tol=tol, opts=dict(max_iters=1))

    A, l, u = lp_cases.bounded_batch(100, 1, 16, 8)
    row = int(polyhedra.implicit_bounds_host(colmajor(A), l, u, opts=dict(max_iters=1))["fail_row"][0])
    with pytest.raises(RuntimeError, match=rf"status {ITER_LIMIT} on polyhedron 1, row {row}$"):
        polyhedra.implicit_bounds_batch([PINNED, (A[0], l[0], u[0])], Cut(), route="polyhedron")


def test_shapes_beyond_the_limits_take_the_route_of_the_jobs():
    wide = (np.eye(2, 257), np.array([0.0, -1.0]), np.array([0.0, 1.0]))
    spy = make_spy()
    got = polyhedra.implicit_bounds_batch([PINNED, wide], spy, route="polyhedron")
    assert spy.shapes == [(3, 2)] and spy.lp_calls == 1
    assert list(got[0][0]) == [True] * 3 and list(got[1][0]) == [True, False] and got[1][1][0] == 0.0
    # an empty polyhedron beyond the limits with a lower number than an empty one within them: the lowest-numbered is named
    wide_empty = (np.vstack([np.eye(1, 257), np.eye(1, 257)]), np.array([-INF, 1.0]), np.array([-1.0, INF]))   # x1 <= -1 and x1 >= 1
    empty = (np.array([[1.0, 0.0], [1.0, 0.0]]), np.array([-INF, 1.0]), np.array([-1.0, INF]))
    with pytest.raises(RuntimeError, match=r"Empty set \(polyhedron 1\)"):
        polyhedra.implicit_bounds_batch([PINNED, wide_empty, empty], make_spy(), route="polyhedron")
    with pytest.raises(RuntimeError, match=r"Empty set \(polyhedron 1\)"):
        polyhedra.implicit_bounds_batch([PINNED, empty, wide_empty], make_spy(), route="polyhedron")


def test_check_convexity_items_on_the_spy_engine():
    """The convexity check through the spy: the same equality masks reach convexity_nodes by either route, and the same error."""
    from test_convexity_host import MSG, _leaf, convexity_restated
    from qpn_amd import algorithm, examples, qp_processing
    assert qp_processing.IMPLICIT_BOUNDS_ROUTE == "jobs"

    def engine():
        spy = make_spy()
        spy.masks = []

        def convexity_nodes(Qc, Ac, eq, tol=1e-6):
            spy.masks.append(np.array(eq, copy=True))
            return convexity_restated(Qc, Ac, eq, tol)[:3]
        spy.convexity_nodes = convexity_nodes
        return spy

    def items_of(net):
        return [(pid, []) for pid in sorted(net.qps)]

    # a leaf that is convex only on the implicit equality x2 = 0 (two one-sided rows), next to one that needs none
    runs = {}
    for route in ("jobs", "polyhedron"):
        spy = engine()
        qp_processing.check_convexity_items(_leaf(pinned=True, players=2, nonconvex=(0,)), items_of(_leaf(pinned=True, players=2)), spy,
                                            route=route)
        assert bool(spy.shapes) == (route == "polyhedron") and (spy.node_solves == 0 and spy.lp_calls == 0) == (route == "polyhedron")
        runs[route] = spy.masks
        bad = _leaf(pinned=False, players=2, nonconvex=(1,))
        with pytest.raises(qp_processing.NonConvexQPError) as err:
            qp_processing.check_convexity_items(bad, items_of(bad), engine(), route=route)
        assert err.value.pid == sorted(bad.qps)[1] and str(err.value) == MSG.format(err.value.pid)
    assert len(runs["jobs"]) == len(runs["polyhedron"]) >= 1 and all(np.array_equal(a, b) for a, b in zip(runs["jobs"], runs["polyhedron"]))
    assert any(m.any() for m in runs["polyhedron"])
    # solve() with the option on: the module constant is the default of both functions
    runs = {}
    for route in ("jobs", "polyhedron"):
        spy = engine()
        qp_processing.IMPLICIT_BOUNDS_ROUTE = route
        try:
            ret = algorithm.solve(examples.setup("synthetic_pairs", pairs=3, n=3, m=2, check_convexity=True), engine=spy)
        finally:
            qp_processing.IMPLICIT_BOUNDS_ROUTE = "jobs"
        assert ret["solved"] and bool(spy.shapes) == (route == "polyhedron")
        runs[route] = (spy.masks, ret["x_opt"])
    assert len(runs["jobs"][0]) == len(runs["polyhedron"][0]) >= 1
    assert all(np.array_equal(a, b) for a, b in zip(runs["jobs"][0], runs["polyhedron"][0]))
    assert np.array_equal(runs["jobs"][1], runs["polyhedron"][1])


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_symbol_and_its_signature():
    from qpn_amd import _lib
    assert "qpn_implicit_bounds" in _lib.ABI_SYMBOLS
    lib = _lib.load_library()
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert list(lib.qpn_implicit_bounds.argtypes) == [vp, i32, i32, i32, vp, vp, vp, ctypes.c_double, i32, ctypes.POINTER(_lib.LpOpts),
                                                       vp, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_int]
    assert (_lib.IB_OK, _lib.IB_EMPTY, _lib.IB_ITER_LIMIT, _lib.IB_FAILURE) == (OK, EMPTY, ITER_LIMIT, FAILURE)
    assert (_lib.IB_HOW_UNDECIDED, _lib.IB_HOW_EXPLICIT, _lib.IB_HOW_IMPLICIT, _lib.IB_HOW_BY_POINTS, _lib.IB_HOW_BY_EXTREMES,
            _lib.IB_HOW_UNBOUNDED) == (UNDECIDED, EXPLICIT, IMPLICIT, BY_POINTS, BY_EXTREMES, UNBOUNDED)
    assert (polyhedra.IB_OK, polyhedra.IB_EMPTY, polyhedra.IB_ITER_LIMIT, polyhedra.IB_FAILURE) == (OK, EMPTY, ITER_LIMIT, FAILURE)
    assert _lib.IB_ALL_EXTREMES == polyhedra.IB_ALL_EXTREMES == 1
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qpn_hip.h")).read()
    for name, v in (("QPN_IB_OK", OK), ("QPN_IB_EMPTY", EMPTY), ("QPN_IB_ITER_LIMIT", ITER_LIMIT), ("QPN_IB_FAILURE", FAILURE),
                    ("QPN_IB_HOW_UNDECIDED", UNDECIDED), ("QPN_IB_HOW_EXPLICIT", EXPLICIT), ("QPN_IB_HOW_IMPLICIT", IMPLICIT),
                    ("QPN_IB_HOW_BY_POINTS", BY_POINTS), ("QPN_IB_HOW_BY_EXTREMES", BY_EXTREMES), ("QPN_IB_HOW_UNBOUNDED", UNBOUNDED)):
        assert f"{name} = {v}" in header, name
    assert "#define QPN_IB_ALL_EXTREMES 1" in header
