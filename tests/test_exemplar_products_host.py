"""polyhedra_host.exemplar_products_host, the numpy twin of qpn_exemplar_products, and the host functions that
use the entry, without a GPU: planted polyhedra cut into products of pieces against the twin of the whole polyhedron, bit for bit;
the closure test on points planted with a margin; bad factors; isempty_products and combine_at with route="products" on a spy engine
served by the twins."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

import exemplar_cases
import products_cases
import qpn_amd  # noqa: F401
from exemplar_cases import FAILURE, TOL
from products_cases import POINT_TOL
from qpn_amd import polyhedra, qp_processing
from qpn_amd.engine import colmajor
from qpn_amd.programs import Poly
from twin_engine import TwinEngine

INF = np.inf
NOT_NEAR = 6
SHARED = exemplar_cases.OUTPUTS                   # the outputs the entry shares with qpn_exemplar_polys


class Spy(TwinEngine):
    """The twin engine plus exemplar_products, served by its twin and logged like the others."""

    def exemplar_products(self, A, l, u, open_lo, open_hi, piece_row, factors, n, point=None, point_of=None, point_tol=1e-6, tol=1e-2,
                          slack_cap=1.0, opts=None):
        assert piece_row.dtype == np.int32 and factors.dtype == np.int32 and (point_of is None or point_of.dtype == np.int32)
        assert open_lo.dtype == np.uint8 and open_hi.dtype == np.uint8
        self._note("exemplar_products", A, l, u, open_lo, open_hi, piece_row, factors, point, point_of)
        return polyhedra.exemplar_products_host(A, l, u, open_lo, open_hi, piece_row, factors, n, point=point, point_of=point_of,
                                                point_tol=point_tol, tol=tol, slack_cap=slack_cap, opts=opts)

    def count(self, *methods):
        return sum(1 for m, _ in self.log if m in methods)


NODE_CALLS = ("exemplar_polys", "solve_lps", "solve_nodes")


# ---- the twin ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 2), (8, 4), (24, 8)])
def test_cut_polyhedra_equal_the_twin_of_the_whole(shape):
    c = products_cases.cut_batch(shape, 20)
    A, l, u, ol, oh = c["whole"]
    want = polyhedra.exemplar_polys_host(colmajor(A), l, u, ol, oh, tol=TOL)
    got = polyhedra.exemplar_products_host(*c["pool"], c["piece_row"], c["factors"], c["n"], tol=TOL)
    exemplar_cases.same_bits(got, want, "cut")
    assert np.array_equal(got["how"], c["how"]) and np.array_equal(got["empty"].astype(bool), c["empty"]) and got["near"].all()
    assert got["near"].dtype == np.uint8
    # the cuts hold what they are meant to: every k, an empty run, slots without a factor
    used = (c["factors"] >= 0).sum(1)
    sizes = np.diff(c["piece_row"])
    assert sorted(set(used)) == [1, 2, 3, 5] and (sizes == 0).any() and ((c["factors"] == -1).sum(1) >= 2).all()
    assert not np.array_equal(np.sort(c["factors"][c["factors"] >= 0]), c["factors"][c["factors"] >= 0])     # the pool is shuffled


def _closure_case(shape, count=20):
    """The `fat` polyhedra of a cut batch, each asked twice: at the plant's own x0 and at x0 moved 0.01 beyond one bound.
    -> (the batch, factors [2 f, slots], points [2 f, d], point_of, the rows moved beyond [f], the polyhedra [f])."""
    n, d = shape
    c = products_cases.cut_batch(shape, count)
    A, l, u, _, _ = c["whole"]
    fat = [t for t in range(count) if exemplar_cases.KINDS[t % 5] == "fat"]
    points, rows = [], []
    for t in fat:
        x0 = products_cases.plant_x0(t, n, d, "fat")
        s0 = A[t] @ x0
        assert np.all(s0 - l[t] >= products_cases.MARGIN) and np.all(u[t] - s0 >= products_cases.MARGIN)
        p, row = products_cases.closure_points(A[t], l[t], u[t], x0)
        points += [x0, p]; rows.append(row)
    factors = np.repeat(c["factors"][fat], 2, axis=0)
    return c, factors, np.array(points), np.arange(2 * len(fat), dtype=np.int32), np.array(rows), fat


@pytest.mark.parametrize("shape", [(3, 2), (8, 4), (24, 8)])
def test_the_closure_test_on_planted_points(shape):
    n, d = shape
    c, factors, points, point_of, rows, fat = _closure_case(shape)
    got = polyhedra.exemplar_products_host(*c["pool"], c["piece_row"], factors, n, point=points, point_of=point_of, point_tol=POINT_TOL, tol=TOL)
    A, l, u, ol, oh = (v[fat] for v in c["whole"])
    whole = polyhedra.exemplar_polys_host(colmajor(A), l, u, ol, oh, tol=TOL)
    exemplar_cases.same_bits({k: np.ascontiguousarray(got[k][0::2]) for k in SHARED}, whole, "at x0")
    assert got["near"].tolist() == [1, 0] * len(fat)
    off = {k: got[k][1::2] for k in got}
    assert np.array_equal(off["row"], rows) and np.all(off["how"] == NOT_NEAR) and not off["iters"].any() and not off["empty"].any()
    assert np.isnan(off["eps"]).all() and not off["x"].any() and not off["lam"].any()
    # closed relations whatever the flags: a point on an open bound is near
    pool = (np.array([[1.0, 0.0], [0.0, 1.0]]), np.array([0.0, 0.0]), np.array([1.0, 1.0]), np.array([1, 0], np.uint8), np.array([0, 1], np.uint8))
    on = polyhedra.exemplar_products_host(*pool, [0, 1, 2], [[0, 1]], 2, point=[[0.0, 1.0], [0.0, 1.0 + 1e-3]], point_of=[0], tol=TOL)
    assert on["near"].tolist() == [1] and on["how"].tolist() == [exemplar_cases.MEMBER]
    far = polyhedra.exemplar_products_host(*pool, [0, 1, 2], [[0, 1], [1, 0]], 2, point=[[0.0, 1.0], [0.0, 1.0 + 1e-3]], point_of=[1, 1], tol=TOL)
    assert far["near"].tolist() == [0, 0] and far["row"].tolist() == [3, 1]                # row counts PRODUCT rows


def test_bad_factors_raise_on_host_arrays_and_fail_on_device_arrays():
    c = products_cases.cut_batch((8, 4), 10)
    pieces = len(c["piece_row"]) - 1
    twin = lambda f, **kw: polyhedra.exemplar_products_host(*c["pool"], c["piece_row"], f, c["n"], tol=TOL, **kw)
    good = twin(c["factors"])
    bads = []
    for value in (pieces, -2):
        f = c["factors"].copy(); f[3, np.nonzero(f[3] >= 0)[0][0]] = value
        bads.append(f)
    sizes = np.diff(c["piece_row"])
    own = [int(v) for v in c["factors"][5] if v >= 0]
    big = max(own, key=lambda p: sizes[p])                                       # (a piece of product 5 that has rows)
    f = c["factors"].copy(); f[5][f[5] == big] = -1                              # one piece missing: the rows do not add up to n
    bads.append(f)
    f = c["factors"].copy(); f[5, np.nonzero(f[5] == -1)[0][0]] = big            # ... and one piece twice
    bads.append(f)
    for f in bads:
        with pytest.raises(ValueError):
            twin(f)
    with pytest.raises(ValueError):
        twin(c["factors"], point=np.zeros((1, 4)), point_of=np.full(10, 1))
    with pytest.raises(ValueError):
        twin(c["factors"], point=np.zeros((1, 4)))
    # what device arrays answer: those products alone fail, with zeros
    f = c["factors"].copy()
    f[3, np.nonzero(f[3] >= 0)[0][0]] = pieces; f[6, np.nonzero(f[6] >= 0)[0][0]] = -2
    got = twin(f, device=True)
    rest = np.delete(np.arange(10), [3, 6])
    exemplar_cases.same_bits({k: got[k][rest] for k in SHARED}, {k: good[k][rest] for k in SHARED}, "the rest")
    assert np.all(got["how"][[3, 6]] == FAILURE) and not got["near"][[3, 6]].any() and not got["empty"][[3, 6]].any()
    assert not got["x"][[3, 6]].any() and not got["lam"][[3, 6]].any() and not got["iters"][[3, 6]].any() and got["near"][rest].all()


# ---- the front end ----------------------------------------------------------------------------------------------------------------
def _as_pieces(c):
    A, l, u, ol, oh = c["pool"]
    pr = c["piece_row"]
    return [(A[a:b], l[a:b], u[a:b], (ol[a:b] != 0) & np.isfinite(l[a:b]), (oh[a:b] != 0) & np.isfinite(u[a:b])) for a, b in zip(pr[:-1], pr[1:])]


def test_isempty_products_groups_by_shape_and_keeps_the_shortcuts_on_the_host():
    small, large = products_cases.cut_batch((3, 2), 10), products_cases.cut_batch((8, 4), 10)
    pieces = _as_pieces(small)
    products = [tuple(int(f) for f in row if f >= 0) for row in small["factors"]]
    base = len(pieces)
    pieces += _as_pieces(large)
    products += [tuple(base + int(f) for f in row if f >= 0) for row in large["factors"]]
    plant = np.concatenate([small["empty"], large["empty"]])
    # the square-equality shortcut (n == d, closed, l == u), one piece of no rows alone, and 33 factors
    base = len(pieces)
    pieces += [(np.eye(2)[:1], np.array([1.0]), np.array([1.0]), np.zeros(1, bool), np.zeros(1, bool)),
               (np.eye(2)[1:], np.array([2.0]), np.array([2.0]), np.zeros(1, bool), np.zeros(1, bool)),
               (np.zeros((0, 2)), np.zeros(0), np.zeros(0), np.zeros(0, bool), np.zeros(0, bool)),
               (np.array([[1.0, 1.0]]), np.array([5.0]), np.array([INF]), np.zeros(1, bool), np.zeros(1, bool))]
    products += [(base, base + 1), (base + 2,), (base + 3, base, base + 1), (base,) + (base + 2,) * 32]
    plant = np.concatenate([plant, [False, False, True, False]])
    spy = Spy()
    near, empty = polyhedra.isempty_products(pieces, products, spy, tol=TOL)
    assert near.all() and np.array_equal(empty, plant)
    calls = [(m, s) for m, s in spy.log]
    assert [m for m, _ in calls].count("exemplar_products") == 2 and spy.count("solve_lps", "solve_nodes") == 0       # (d, n) = (2, 3) and (4, 8)
    assert spy.count("exemplar_polys") == 1                     # the 33 factors: beyond the limits, the way of route="polyhedron"
    pools = sorted({s[0] for m, s in calls if m == "exemplar_products"})
    assert pools == ["float64[%d, 2]" % (small["pool"][0].shape[0] + 3), "float64[%d, 4]" % large["pool"][0].shape[0]]   # a pool per d
    # with points: the front end's verdicts are the twin's, shortcut products tested on the host
    pts = [np.array([1.0, 2.0]), np.array([0.0, 0.0])]
    near, empty = polyhedra.isempty_products(pieces[base:], [(0, 1), (0, 1), (3, 0, 1), (3, 0, 1)], Spy(), tol=TOL, points=pts, point_of=[0, 1, 0, 1])
    assert near.tolist() == [True, False, False, False] and empty.tolist() == [False, False, False, False]
    # a product without an answer raises, the lowest-numbered one is named
    bad = (np.array([[np.nan, 1.0]]), np.array([0.0]), np.array([1.0]), np.zeros(1, bool), np.zeros(1, bool))
    with pytest.raises(RuntimeError, match=rf"exemplar status {FAILURE} on product 1$"):
        polyhedra.isempty_products(pieces[base:] + [bad], [(3,), (4,)], Spy(), tol=TOL)
    assert polyhedra.isempty_products(pieces[base:] + [bad], [(3,), (4,)], Spy(), tol=TOL, strict=False)[1].tolist() == [False, False]


# ---- combine_at -------------------------------------------------------------------------------------------------------------------
def _kink():
    """tests/test_level_batch.py's hand-worked kink y = max(x, 0) with S1 = R1, S2 = the kink alone."""
    R1 = Poly(np.array([[0.0, 1.0], [1.0, 0.0]]), [0.0, -INF], [0.0, 0.0])
    R2 = Poly(np.array([[1.0, -1.0], [0.0, 1.0]]), [0.0, 0.0], [0.0, INF])
    S1 = Poly(np.array([[0.0, 1.0], [1.0, 0.0]]), [0.0, -INF], [0.0, 0.0])
    S2 = Poly(np.array([[1.0, 0.0], [0.0, 1.0]]), [0.0, 0.0], [0.0, 0.0])
    return [[R1], [R2]], [[S1], [S2]], np.zeros(2)


def _same_pieces(got, want):
    assert len(got) == len(want)
    for P, Q in zip(got, want):
        for a, b in zip(P.vectorize() + (P.open_lo, P.open_hi), Q.vectorize() + (Q.open_lo, Q.open_hi)):
            assert a.dtype == b.dtype and np.array_equal(a, b)


def test_combine_at_on_the_kink_by_products_equals_the_polyhedron_route(monkeypatch):
    regions, solutions, x = _kink()
    old = Spy()
    want = qp_processing.combine_at(regions, solutions, x, old, route="polyhedron")
    assert old.count("exemplar_polys") >= 1 and old.count("exemplar_products") == 0 and len(want) >= 2
    spy = Spy()
    got = qp_processing.combine_at(regions, solutions, x, spy, route="products")
    _same_pieces(got, want)
    assert spy.count(*NODE_CALLS) == 0 and spy.count("exemplar_products") >= 1
    # the module constant is combine_many's default
    assert qp_processing.EMPTINESS_ROUTE == "nodes"
    monkeypatch.setattr(qp_processing, "EMPTINESS_ROUTE", "products")
    spy = Spy()
    _same_pieces(qp_processing.combine_at(regions, solutions, x, spy), want)
    assert spy.count(*NODE_CALLS) == 0 and spy.count("exemplar_products") >= 1
    # a point off the kink: the device's closure test drops what Poly.contains dropped
    for pt in ((-1.0, 0.0), (0.5, 0.5)):
        a = qp_processing.combine_at(regions, solutions, np.array(pt), Spy(), route="polyhedron")
        _same_pieces(qp_processing.combine_at(regions, solutions, np.array(pt), Spy(), route="products"), a)
    # the size guard comes back as it did
    many = ([[regions[0][0]]] * 4, [[solutions[0][0]] * 6] * 4)
    with pytest.raises(RuntimeError, match="Too many solutions"):
        qp_processing.combine_at(*many, x, Spy(), route="products")


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_symbol_and_its_signature():
    from qpn_amd import _lib
    assert "qpn_exemplar_products" in _lib.ABI_SYMBOLS
    assert _lib.EX_NOT_NEAR == polyhedra.EX_NOT_NEAR == NOT_NEAR and _lib.PROD_MAX_K == polyhedra.PROD_MAX_K == 32
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qpn_hip.h")).read()
    assert "int qpn_exemplar_products(qpn_ctx *ctx" in header and "#define QPN_ABI_VERSION 1" in header and "QPN_EX_NOT_NEAR = 6" in header
    if os.path.exists(_lib.LIB_PATH):                                   # where the library is built
        vp, i32, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
        lib = _lib.load_library()
        assert list(lib.qpn_exemplar_products.argtypes) == [vp, i32, i32, vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, vp, i32, vp, vp, f64, f64, f64,
                                                             ctypes.POINTER(_lib.LpOpts)] + [vp] * 8 + [ctypes.c_int]
