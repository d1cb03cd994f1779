"""polyhedra.exemplar_polys_host, the numpy twin and normative statement of qpn_exemplar_polys (one job per polyhedron whose
bounds may be open), without a GPU: the planted family of tests/exemplar_cases.py against its plant and HiGHS, hand cases,
exemplar_slack_batch / combine_at with route="polyhedron" on an engine that has `exemplar_polys` (a spy built from the twin over
the oracle engine) against today's route, and the new symbol with its ctypes signature."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest
from scipy.optimize import linprog

import degenerate_cases
import exemplar_cases
import lp_cases
from exemplar_cases import EMPTY_OPEN, EMPTY_SLACK, FAILURE, ITER_LIMIT, KINDS, MEMBER, MEMBER_BAND, TOL

from qpn_amd import polyhedra
from qpn_amd.engine import colmajor
from qpn_amd.programs import Poly

INF = np.inf
SHAPES = [((1, 1), 20), ((3, 2), 20), ((8, 4), 20), ((24, 8), 20), ((40, 24), 4), ((130, 80), 1)]       # (shape, seeds per kind)


def _twin(A, l, u, ol=None, oh=None, **kw):
    return polyhedra.exemplar_polys_host(colmajor(A), l, u, ol, oh, **kw)


def _one(A, l, u, ol=None, oh=None, **kw):
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    f = lambda a: None if a is None else np.asarray(a)[None]
    return {k: v[0] for k, v in _twin(A[None], np.asarray(l, float)[None], np.asarray(u, float)[None], f(ol), f(oh), **kw).items()}


def _highs_eps(A, l, u, cap=1.0):
    """The optimal slack of the same LP by HiGHS."""
    A2, l2, _ = polyhedra.exemplar_rows(A, l, u, cap)
    fin = np.isfinite(l2)
    res = linprog(np.eye(1, A2.shape[1], A2.shape[1] - 1)[0], A_ub=-A2[fin], b_ub=-l2[fin], bounds=[(None, None)] * A2.shape[1], method="highs")
    assert res.status == 0, res.message
    return res.fun


@pytest.mark.parametrize("shape,seeds", SHAPES)
def test_the_family_against_its_plant_and_highs(shape, seeds):
    n, d = shape
    A, l, u, ol, oh, empty, how = exemplar_cases.family_batch(shape, 5 * seeds)
    got = _twin(A, l, u, ol, oh, tol=TOL)
    closed = _twin(A, l, u, tol=TOL)                             # the same LPs: the flags touch nothing but the rule
    assert np.array_equal(got["empty"].astype(bool), empty) and np.array_equal(got["how"], how)
    assert not np.isin(got["how"], (ITER_LIMIT, FAILURE)).any()
    assert np.array_equal(got["lam"], closed["lam"]) and np.array_equal(got["eps"], closed["eps"]) and np.array_equal(got["iters"], closed["iters"])
    assert np.all(got["x"][empty] == 0.0) and np.array_equal(got["x"][~empty], closed["x"][~empty])
    assert np.all((got["row"] >= 0) == (how == EMPTY_OPEN)) and np.all(closed["row"] == -1)
    for t in range(len(A)):
        kind = KINDS[t % 5]
        eps = got["eps"][t]
        assert abs(eps - _highs_eps(A[t], l[t], u[t])) <= 1e-8, (t, kind)
        assert abs(abs(eps) - TOL) > 1e-5
        assert eps <= -0.05 if kind == "fat" else abs(eps - 1.0) <= 1e-9 if kind == "gap" else abs(eps) <= 1e-9
        x = got["x"][t]
        if not empty[t]:                                        # the member: inside the closed polyhedron up to the band
            assert np.all(A[t] @ x >= l[t] - 2 * TOL) and np.all(A[t] @ x <= u[t] + 2 * TOL)
        if kind.startswith("thin"):                             # in the band: the multipliers certify the optimum of the slack LP
            A2, l2, u2 = polyhedra.exemplar_rows(A[t], l[t], u[t])
            c = np.eye(1, d + 1, d)[0]
            xe = np.concatenate([closed["x"][t], [eps]])
            lp_cases.check_certificates(A2, l2, u2, c, dict(status=lp_cases.OPTIMAL, x=xe, obj=eps, lam=got["lam"][t], ray=np.zeros(d + 1)))
        if kind == "thin_open":                                 # the unique dual: 1/2 on both sides of the pinned row, the lowest open one
            k = int(np.nonzero(l[t] == u[t])[0][0])
            lam = got["lam"][t]
            assert abs(lam[k] - 0.5) <= 1e-9 and abs(lam[n + k] - 0.5) <= 1e-9 and np.all(np.abs(np.delete(lam, [k, n + k])) <= 1e-9)
            assert got["row"][t] == 2 * k


def test_the_hand_cases():
    """tests/test_polyhedra.py's four: {0 < x <= 1}, {0 < x <= 0}, {0 <= x <= 0} and a point of the plane with one open bound."""
    one = np.array([[1.0]])
    a = _one(one, [0.0], [1.0], [1], [0], tol=1e-4)
    b = _one(one, [0.0], [0.0], [1], [0], tol=1e-4)
    c = _one(one, [0.0], [0.0], tol=1e-4)
    d = _one(np.array([[1.0, 1.0], [1.0, -1.0]]), [0.0, 0.0], [0.0, 0.0], [0, 0], [1, 0], tol=1e-4)
    assert [bool(r["empty"]) for r in (a, b, c, d)] == [False, True, False, True]
    assert [int(r["how"]) for r in (a, b, c, d)] == [MEMBER, EMPTY_OPEN, MEMBER_BAND, EMPTY_OPEN]
    assert a["eps"] == -0.5 and a["x"][0] == 0.5
    assert b["row"] == 0 and d["row"] == 1 and a["row"] == c["row"] == -1
    assert not b["x"].any() and not d["x"].any() and c["x"][0] == 0.0


@pytest.mark.parametrize("what", ["A", "l", "u", "l=+inf", "u=-inf"])
def test_non_finite_data_is_a_failure_with_zeros(what):
    A, l, u, ol, oh, _ = exemplar_cases.planted(3, 12, 4, "fat")
    A, l, u, _ = degenerate_cases.with_nonfinite((A, l, u, np.zeros(4)), what)
    got = _one(A, l, u, ol, oh, tol=TOL)
    assert got["how"] == FAILURE and got["empty"] == 0 and np.isnan(got["eps"]) and got["row"] == -1 and got["iters"] == 0
    assert not got["x"].any() and not got["lam"].any()


def test_the_iteration_limit():
    A, l, u, ol, oh, empty, _ = exemplar_cases.family_batch((8, 4), 10)
    full = _twin(A, l, u, ol, oh, tol=TOL)
    cut = _twin(A, l, u, ol, oh, tol=TOL, opts=dict(max_iters=1))
    long = full["iters"] > 1
    assert long.sum() >= 8
    assert np.all(cut["how"][long] == ITER_LIMIT) and np.all(cut["iters"][long] == 1) and not cut["empty"][long].any()
    assert np.all(np.isnan(cut["eps"][long])) and not cut["x"][long].any() and not cut["lam"][long].any() and np.all(cut["row"][long] == -1)
    assert np.array_equal(cut["how"][~long], full["how"][~long])


def test_an_open_flag_on_an_infinite_bound_is_ignored():
    """{x >= 0, x <= 0} as two one-sided rows: the infinite sides flagged open change nothing, the finite ones decide."""
    A = np.array([[1.0], [1.0]]); l = np.array([0.0, -INF]); u = np.array([INF, 0.0])
    flagged = _one(A, l, u, [0, 1], [1, 0], tol=TOL)
    assert flagged["how"] == MEMBER_BAND and flagged["row"] == -1 and abs(flagged["eps"]) <= 1e-12
    assert _one(A, l, u, [1, 1], [1, 0], tol=TOL)["row"] == 0 and _one(A, l, u, [0, 1], [1, 1], tol=TOL)["row"] == 3
    # the family with every infinite side flagged: the answers of the flags it has
    A, l, u, ol, oh, empty, how = exemplar_cases.family_batch((8, 4), 25)
    more = _twin(A, l, u, ol | np.isinf(l), oh | np.isinf(u), tol=TOL)
    assert np.array_equal(more["how"], how) and np.isinf(l).any() and np.isinf(u).any()


# ---- the host routes on an engine that has exemplar_polys -------------------------------------------------------------------------
def make_spy():
    from oracle_engine import OracleEngine

    class Spy(OracleEngine):
        """The oracle engine with solve_lps and exemplar_polys made from the twins; the calls are counted where they arrive."""

        def __init__(self):
            super().__init__()
            self.shapes = []                                # (n, d) per exemplar_polys call
            self.node_solves = self.lp_calls = 0

        def solve_nodes(self, *a, **k):
            self.node_solves += 1
            return OracleEngine.solve_nodes(self, *a, **k)

        def solve_lps(self, Ac, l, u, poly_of, cost=None, obj_row=None, obj_sign=None, opts=None):
            self.lp_calls += 1
            return polyhedra.solve_lps_host(Ac, l, u, poly_of, cost=cost, obj_row=obj_row, obj_sign=obj_sign, opts=opts)

        def exemplar_polys(self, Ac, l, u, open_lo=None, open_hi=None, tol=1e-2, slack_cap=1.0, opts=None):
            self.shapes.append((Ac.shape[2], Ac.shape[1]))
            return polyhedra.exemplar_polys_host(Ac, l, u, open_lo, open_hi, tol=tol, slack_cap=slack_cap, opts=opts)

    return Spy()


def test_exemplar_slack_batch_on_the_spy_engine():
    from oracle_engine import OracleEngine
    polys, plant = exemplar_cases.family_polys()
    square = Poly(np.eye(2), [1.0, 2.0], [1.0, 2.0])                      # the square-equality shortcut stays on the host
    norows = (np.zeros((0, 2)), np.zeros(0), np.zeros(0))
    polys += [square, norows]; plant = np.concatenate([plant, [False, False]])
    spy = make_spy()
    empty, example, eps = polyhedra.exemplar_slack_batch(polys, spy, tol=TOL, route="polyhedron")
    assert spy.node_solves == 0 and spy.lp_calls == 0
    assert sorted(spy.shapes) == [(1, 1), (3, 2), (8, 4)]                  # one call per shape, closed and open items alike
    want, example0, eps0 = polyhedra.exemplar_slack_batch(polys, OracleEngine(), tol=TOL)
    assert np.array_equal(empty, want) and np.array_equal(empty, plant)
    answered = ~np.isnan(eps0)                                            # (the shortcut -- here the 6 closed 1 x 1 points -- and n = 0 give no eps, by either route)
    assert np.array_equal(np.isnan(eps), ~answered) and np.all(np.abs(eps[answered] - eps0[answered]) <= 1e-8) and answered.sum() == 39
    assert np.allclose(example[-2], [1.0, 2.0]) and example[-1] is None
    for p, e, x in zip(polys[:-2], empty, example):
        assert (x is None) == bool(e)
        if not e:
            assert np.all(p.A @ x >= p.l - 2 * TOL) and np.all(p.A @ x <= p.u + 2 * TOL)
    assert np.array_equal(polyhedra.isempty_slack_batch(polys, spy, tol=TOL, route="polyhedron"), plant)
    # the default is today's route; an engine without the method keeps it whatever is asked
    spy = make_spy()
    assert np.array_equal(polyhedra.exemplar_slack_batch(polys, spy, tol=TOL)[0], plant)
    assert not spy.shapes and spy.lp_calls > 0 and spy.node_solves > 0
    assert np.array_equal(polyhedra.exemplar_slack_batch(polys, OracleEngine(), tol=TOL, route="polyhedron")[0], plant)
    assert np.array_equal(polyhedra.exemplar_slack_batch(polys, make_spy(), tol=TOL, route="nodes")[0], plant)
    with pytest.raises(ValueError):
        polyhedra.exemplar_slack_batch(polys, spy, route="rows")


def test_shapes_beyond_the_limits_take_todays_route():
    wide = (np.eye(2, 256), np.array([0.0, -1.0]), np.array([0.0, 1.0]))
    inside = Poly(np.array([[1.0]]), [0.0], [0.0], open_lo=[True])
    spy = make_spy()
    empty, example, _ = polyhedra.exemplar_slack_batch([inside, wide], spy, tol=TOL, route="polyhedron")
    assert spy.shapes == [(1, 1)] and spy.lp_calls == 1 and list(empty) == [True, False] and example[1].shape == (256,)


def test_strict_names_the_item_that_got_no_answer():
    class Cut(type(make_spy())):
        def exemplar_polys(self, Ac, l, u, open_lo=None, open_hi=None, tol=1e-2, slack_cap=1.0, opts=None):
            return polyhedra.exemplar_polys_host(Ac, l, u, open_lo, open_hi, tol=tol, slack_cap=slack_cap, opts=dict(max_iters=1))

    polys, _ = exemplar_cases.family_polys(shapes=((8, 4),), count=5)
    point = Poly(np.array([[1.0]]), [0.0], [1.0])                        # one step solves it
    with pytest.raises(RuntimeError, match=rf"exemplar status {ITER_LIMIT} on item 1$"):
        polyhedra.exemplar_slack_batch([point] + polys, Cut(), tol=TOL, route="polyhedron")
    empty, example, eps = polyhedra.exemplar_slack_batch([point] + polys, Cut(), tol=TOL, route="polyhedron", strict=False)
    assert not empty.any() and example[0] is not None and all(x is None for x in example[1:]) and np.isnan(eps[1:]).all()
    nan = (np.array([[np.nan, 1.0]]), np.array([0.0]), np.array([1.0]))
    with pytest.raises(RuntimeError, match=rf"exemplar status {FAILURE} on item 0$"):
        polyhedra.exemplar_slack_batch([nan], make_spy(), tol=TOL, route="polyhedron")


def test_combine_at_on_the_hand_worked_kink():
    """tests/test_level_batch.py's kink y = max(x, 0) with S1 = R1, S2 = the kink alone: the same membership assertions by either
    route, and the polyhedron route without a node solve or a solve_lps call."""
    from oracle_engine import OracleEngine
    from qpn_amd import qp_processing
    from qpn_amd.qp_processing import combine_at
    assert qp_processing.EMPTINESS_ROUTE == "nodes"
    R1 = Poly(np.array([[0.0, 1.0], [1.0, 0.0]]), [0.0, -INF], [0.0, 0.0])
    R2 = Poly(np.array([[1.0, -1.0], [0.0, 1.0]]), [0.0, 0.0], [0.0, INF])
    S1 = Poly(np.array([[0.0, 1.0], [1.0, 0.0]]), [0.0, -INF], [0.0, 0.0])
    S2 = Poly(np.array([[1.0, 0.0], [0.0, 1.0]]), [0.0, 0.0], [0.0, 0.0])
    x = np.zeros(2)
    spy = make_spy()
    out = combine_at([[R1], [R2]], [[S1], [S2]], x, spy, route="polyhedron")
    assert spy.shapes and spy.node_solves == 0 and spy.lp_calls == 0
    want = combine_at([[R1], [R2]], [[S1], [S2]], x, OracleEngine())
    # (the product {y = 0, x <= 0, x - y > 0} has eps = 0 with optimal duals that are not unique: the simplex puts them on the two
    #  sides of y = 0, the node solver on the open bound, so the routes may differ in that one thin piece -- DESIGN section 5j)
    assert len(out) >= 2 and len(want) >= 2
    inside = lambda pt: any(P.contains(np.array(pt, float), tol=1e-9) for P in out)
    assert inside((0.0, 0.0))
    assert inside((-1.0, 0.0))                    # optimal under R1, outside R2: stays in the graph
    assert not inside((1.0, 1.0))                 # in R2 but not optimal under it: must go
    assert not inside((1.0, 0.5)) and not inside((-1.0, 1.0))        # outside both regions: complement-only products are skipped
    for P in out:
        assert P.vectorize()[0].shape[0] >= 2
    # the module constant is combine_many's default
    spy = make_spy()
    qp_processing.EMPTINESS_ROUTE = "polyhedron"
    try:
        again = combine_at([[R1], [R2]], [[S1], [S2]], x, spy)
    finally:
        qp_processing.EMPTINESS_ROUTE = "nodes"
    assert spy.shapes and spy.node_solves == 0 and len(again) == len(out)
    spy = make_spy()
    combine_at([[R1], [R2]], [[S1], [S2]], x, spy)
    assert not spy.shapes and spy.node_solves > 0


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_symbol_and_its_signature():
    from qpn_amd import _lib
    assert "qpn_exemplar_polys" in _lib.ABI_SYMBOLS
    vp, i32, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    values = (MEMBER, MEMBER_BAND, EMPTY_SLACK, EMPTY_OPEN, ITER_LIMIT, FAILURE)
    assert (_lib.EX_MEMBER, _lib.EX_MEMBER_BAND, _lib.EX_EMPTY_SLACK, _lib.EX_EMPTY_OPEN, _lib.EX_ITER_LIMIT, _lib.EX_FAILURE) == values
    assert (polyhedra.EX_MEMBER, polyhedra.EX_MEMBER_BAND, polyhedra.EX_EMPTY_SLACK, polyhedra.EX_EMPTY_OPEN, polyhedra.EX_ITER_LIMIT,
            polyhedra.EX_FAILURE) == values
    assert (_lib.EX_MAX_N, _lib.EX_MAX_D) == (polyhedra.EX_MAX_N, polyhedra.EX_MAX_D) == (511, 255)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qpn_hip.h")).read()
    assert "int qpn_exemplar_polys(qpn_ctx *ctx" in header and "#define QPN_ABI_VERSION 1" in header
    for name, v in zip(("MEMBER", "MEMBER_BAND", "EMPTY_SLACK", "EMPTY_OPEN", "ITER_LIMIT", "FAILURE"), values):
        assert f"QPN_EX_{name} = {v}" in header, name
    if os.path.exists(_lib.LIB_PATH):                                   # where the library is built
        lib = _lib.load_library()
        assert list(lib.qpn_exemplar_polys.argtypes) == [vp, i32, i32, i32, vp, vp, vp, vp, vp, f64, f64, ctypes.POINTER(_lib.LpOpts),
                                                          vp, vp, vp, vp, vp, vp, vp, ctypes.c_int]
        assert lib.qpn_abi_version() == 1
