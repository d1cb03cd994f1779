"""polyhedra.issubset_pairs_host, the numpy twin and normative statement of qpn_issubset_pairs (one job per pair P1 ⊆ P2), without a
GPU: the seeded family of tests/subset_cases.py against HiGHS, what the outputs claim, hand cases, and issubset_batch /
remove_subsets_many on an engine that has `issubset_pairs` (a spy built from the twin over the oracle engine) against the plain
oracle engine's emptiness queries."""
from __future__ import annotations

import functools

import numpy as np
import pytest
from scipy.optimize import linprog

import subset_cases
from subset_cases import BY_OPTIMUM, BY_POINT, EMPTY, FAILURE, HOLDS, ITER_LIMIT, UNBOUNDED

from qpn_amd import algorithm, examples, polyhedra
from qpn_amd.engine import colmajor

TOL = 1e-6
SEEDS = list(range(48))


def _twin(A1, l1, u1, A2, l2, u2, pi=None, pj=None, **kw):
    n = len(A1)
    return polyhedra.issubset_pairs_host(colmajor(A1), l1, u1, colmajor(A2), l2, u2, np.arange(n) if pi is None else pi,
                                         np.arange(n) if pj is None else pj, **kw)


def _highs(A1, l1, u1, A2, l2, u2):
    """One pair by HiGHS.  -> None when P1 is infeasible, else the list of (2 i + side, minimum - (dir * bound), -inf when
    unbounded) over the finite bounds of P2."""
    rows, rhs = [], []
    for i in range(A1.shape[0]):
        if np.isfinite(u1[i]): rows.append(A1[i]); rhs.append(u1[i])
        if np.isfinite(l1[i]): rows.append(-A1[i]); rhs.append(-l1[i])
    kw = dict(A_ub=np.array(rows) if rows else None, b_ub=np.array(rhs) if rows else None, bounds=[(None, None)] * A1.shape[1],
              method="highs")
    if linprog(np.zeros(A1.shape[1]), **kw).status == 2:
        return None
    out = []
    for i in range(A2.shape[0]):
        for side, (dirn, bound) in enumerate(((1.0, l2[i]), (-1.0, -u2[i]))):
            if np.isfinite(bound):
                r = linprog(dirn * A2[i], **kw)
                assert r.status in (0, 3), r.status
                out.append((2 * i + side, -np.inf if r.status == 3 else r.fun - bound))
    return out


@functools.lru_cache(maxsize=None)
def _family(shape):
    """(the batch, the twin's answer, HiGHS's answer per pair) of one shape: computed once, shared by the tests, left unchanged."""
    batch = subset_cases.family_batch(shape, SEEDS)
    return batch, _twin(*batch), [_highs(*(a[q] for a in batch)) for q in range(len(SEEDS))]


@pytest.mark.parametrize("shape", subset_cases.SHAPES)
def test_the_twin_against_highs(shape):
    _, got, ref = _family(shape)
    left_out, verdicts = 0, set()
    for q, margins in enumerate(ref):
        if margins is None:
            assert got["how"][q] == EMPTY and got["sub"][q] == 1, (shape, q)
            continue
        smallest = min((m for _, m in margins), default=np.inf)
        if abs(smallest + TOL) <= 1e-7:                     # the smallest margin within 1e-7 of the threshold: either verdict
            left_out += 1
            continue
        want = smallest >= -TOL
        assert bool(got["sub"][q]) == want and (got["how"][q] == HOLDS) == want, (shape, q, smallest, got["how"][q])
        verdicts.add(want)
    assert left_out <= 0.02 * len(ref)
    assert verdicts == {True, False}


def test_every_outcome_occurs_over_the_shapes():
    seen = set()
    for shape in subset_cases.SHAPES:
        seen |= set(_family(shape)[1]["how"].tolist())
    assert {BY_POINT, BY_OPTIMUM, UNBOUNDED, EMPTY, HOLDS} <= seen
    assert not seen & {ITER_LIMIT, FAILURE}


@pytest.mark.parametrize("shape", subset_cases.SHAPES)
def test_what_the_outputs_claim(shape):
    (A1, l1, u1, A2, l2, u2), got, ref = _family(shape)
    for q in range(len(SEEDS)):
        how, b, val = int(got["how"][q]), int(got["bound"][q]), got["val"][q]
        finite = int(np.isfinite(l2[q]).sum() + np.isfinite(u2[q]).sum())
        assert got["sub"][q] == (1 if how in (HOLDS, EMPTY) else 0)
        assert 1 <= got["lps"][q] <= 1 + finite
        if b != -1:
            i, side = divmod(b, 2)
            assert 0 <= i < shape[1] and np.isfinite((l2, u2)[side][q, i])
            beta = l2[q, i] if side == 0 else -u2[q, i]
        if how in (BY_POINT, BY_OPTIMUM):
            assert b != -1 and val < beta - TOL
        elif how == UNBOUNDED:
            assert b != -1 and val == 0.0
            assert dict(ref[q])[b] == -np.inf               # HiGHS finds that bound's objective unbounded too
        else:
            assert b == -1 and val == 0.0
        if how == BY_OPTIMUM:                               # a certified optimum: HiGHS's minimum of that bound
            assert abs(dict(ref[q])[b] - (val - beta)) <= 1e-7
        if how == HOLDS:
            assert all(m >= -TOL - 1e-7 for _, m in ref[q])


def _box(lo, hi, d=2):
    return np.eye(d), np.full(d, float(lo)), np.full(d, float(hi))


def _one(P1, P2, **kw):
    got = _twin(*(np.asarray(a)[None] for a in P1), *(np.asarray(a)[None] for a in P2), **kw)
    return {k: v[0] for k, v in got.items()}


def test_hand_cases():
    inner, outer = _box(-1, 1), _box(-2, 2)
    got = _one(inner, outer)                                # (the same rows with wider bounds: all P1's own)
    assert got["how"] == HOLDS and got["sub"] == 1 and got["bound"] == -1 and got["lps"] == 1
    got = _one(inner, (2.0 * np.eye(2), np.full(2, -4.0), np.full(2, 4.0)))
    assert got["how"] == HOLDS and got["sub"] == 1 and got["bound"] == -1 and got["lps"] == 5     # four bounds, none P1's own
    got = _one(outer, inner)
    assert got["how"] in (BY_POINT, BY_OPTIMUM) and got["sub"] == 0 and got["val"] < -1.0 - TOL
    # a box against itself: every bound is one of P1's own rows
    got = _one(inner, inner)
    assert got["how"] == HOLDS and got["lps"] == 1 and got["iters"] == 0
    # ... and still when P2 states the rows in another order with wider bounds
    got = _one(inner, (np.eye(2)[::-1].copy(), np.full(2, -1.5), np.full(2, 1.0 + 5e-7)))
    assert got["how"] == HOLDS and got["lps"] == 1
    # a box against a slab it sticks out of: x + y <= 1 cuts the corner (1, 1)
    slab = (np.array([[1.0, 1.0]]), np.array([-np.inf]), np.array([1.0]))
    got = _one(inner, slab)
    assert got["how"] in (BY_POINT, BY_OPTIMUM) and got["bound"] == 1 and got["sub"] == 0
    if got["how"] == BY_OPTIMUM:
        assert got["val"] == -2.0
    assert _one(_box(-0.25, 0.25), slab)["how"] == HOLDS
    # an open P1 (x <= 1, y in [-1, 1]) against a bounded P2
    open1 = (np.eye(2), np.array([-np.inf, -1.0]), np.array([1.0, 1.0]))
    got = _one(open1, outer)
    assert got["how"] == UNBOUNDED and got["bound"] == 0 and got["sub"] == 0 and got["val"] == 0.0
    # an empty P1
    got = _one((np.array([[1.0, 0.0], [1.0, 0.0]]), np.array([-np.inf, 1.0]), np.array([-1.0, np.inf])), inner)
    assert got["how"] == EMPTY and got["sub"] == 1 and got["lps"] == 1
    got = _one((np.zeros((1, 2)), np.array([1.0]), np.array([2.0])), inner)                       # 0'x >= 1
    assert got["how"] == EMPTY and got["sub"] == 1 and got["iters"] == 0


def test_the_iteration_limit():
    shape = (16, 16, 8)
    batch, full, _ = _family(shape)
    cut = _twin(*batch, opts=dict(max_iters=1))
    long = full["iters"] > full["lps"]                      # some solve of the pair takes more than one step: it is cut there
    assert long.sum() >= 8 and np.all(cut["how"][long] == ITER_LIMIT)
    assert not cut["sub"][long].any() and not cut["val"][long].any()
    assert np.all(cut["iters"] <= cut["lps"])               # one step per solve at the most
    same = ~long
    assert np.array_equal(cut["how"][same], full["how"][same]) and np.array_equal(cut["val"][same], full["val"][same])


def test_indices_out_of_range_fail_alone():
    A1, l1, u1, A2, l2, u2 = subset_cases.family_batch((3, 2, 2), [0, 1, 2])
    got = _twin(A1, l1, u1, A2[:2], l2[:2], u2[:2], pi=np.array([0, 3, -1, 1, 2]), pj=np.array([0, 0, 1, 2, 1]))
    ok = _twin(A1, l1, u1, A2[:2], l2[:2], u2[:2], pi=np.array([0, 2]), pj=np.array([0, 1]))
    assert got["how"][1:4].tolist() == [FAILURE] * 3 and got["bound"][1:4].tolist() == [-1] * 3
    for k in ("sub", "val", "lps", "iters"):
        assert not got[k][1:4].any()
    for k in subset_cases.OUTPUTS:
        assert np.array_equal(got[k][[0, 4]], ok[k])


def test_shared_and_mixed_packs():
    """r1 != r2, B1 != B2, and a first piece shared by several pairs: a pair's answer depends on its two pieces alone."""
    A1, l1, u1, A2, l2, u2 = subset_cases.family_batch((5, 4, 2), range(6))
    pi = np.array([0, 0, 0, 5, 3]); pj = np.array([0, 1, 2, 2, 3])
    got = _twin(A1, l1, u1, A2[:4], l2[:4], u2[:4], pi=pi, pj=pj)
    for q in range(len(pi)):
        one = _one((A1[pi[q]], l1[pi[q]], u1[pi[q]]), (A2[pj[q]], l2[pj[q]], u2[pj[q]]))
        assert all(got[k][q] == one[k] for k in subset_cases.OUTPUTS)


# ---- the host routes on an engine that has issubset_pairs ----------------------------------------------------------------------
def make_spy():
    from oracle_engine import OracleEngine

    class Spy(OracleEngine):
        """The oracle engine with issubset_pairs made from the twin."""

        def __init__(self):
            super().__init__()
            self.shapes = []                                # (r1, r2, d) per call
            self.node_solves = 0

        def solve_nodes(self, *a, **k):
            self.node_solves += 1
            return OracleEngine.solve_nodes(self, *a, **k)

        def issubset_pairs(self, A1c, l1, u1, A2c, l2, u2, pi, pj, tol=1e-6, opts=None):
            assert pi.dtype == np.int32 and pj.dtype == np.int32 and pi.max() < len(A1c) and pj.max() < len(A2c)
            self.shapes.append((A1c.shape[2], A2c.shape[2], A1c.shape[1]))
            return polyhedra.issubset_pairs_host(A1c, l1, u1, A2c, l2, u2, pi, pj, tol=tol, opts=opts)

    return Spy()


def _boxes_and_slabs(seed, count, d=3):
    """(tests/test_polyhedra.py's generator, stated again)"""
    rng = np.random.default_rng(seed)
    polys = []
    for t in range(count):
        c = rng.standard_normal(d); h = 0.2 + rng.random(d) * (2.0 if t % 2 else 0.6)
        G = np.eye(d) if t % 3 else np.linalg.qr(rng.standard_normal((d, d)))[0]
        l = G @ c - h; u = G @ c + h
        if t % 4 == 3: u[0] = np.inf                     # an unbounded slab
        polys.append((G, l, u))
    return polys


def test_issubset_batch_on_the_spy_engine():
    from oracle_engine import OracleEngine
    polys = _boxes_and_slabs(3, 9) + [(np.eye(3), np.full(3, -50.0), np.full(3, 50.0))]
    polys.append((np.array([[1.0, 1.0, 0.0]]), np.array([-np.inf]), np.array([60.0])))            # one row: a second shape
    polys.append((np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]]), np.array([-np.inf, 1.0]), np.array([-1.0, np.inf])))   # empty
    pairs = [(polys[i], polys[j]) for i in range(len(polys)) for j in range(len(polys)) if i != j]
    spy = make_spy()
    got = polyhedra.issubset_batch(pairs, spy)
    want = polyhedra.issubset_batch(pairs, OracleEngine())
    assert np.array_equal(got, want) and want.any() and not want.all()
    assert spy.node_solves == 0 and len(spy.shapes) == len(set(spy.shapes)) == 7                  # three shapes a side; two have one member
    assert np.array_equal(polyhedra.issubset_batch_chunked(pairs, make_spy(), chunk_bytes=400), want)
    kept, mask = polyhedra.remove_subsets(polys, make_spy())
    kept0, mask0 = polyhedra.remove_subsets(polys, OracleEngine())
    assert np.array_equal(mask, mask0) and [id(p) for p in kept] == [id(p) for p in kept0]
    assert polyhedra.issubset_batch([], spy).shape == (0,)


def test_chunks_count_the_packs():
    """On the packed route a chunk's bytes are those of its distinct polyhedra and its indices, not of padded queries."""
    polys = _boxes_and_slabs(5, 6)
    pairs = [(polys[i], polys[j]) for i in range(6) for j in range(6) if i != j]
    one = (9 + 6) * 8                                       # a 3 x 3 polyhedron with its bounds
    spy = make_spy()
    polyhedra.issubset_batch_chunked(pairs, spy, chunk_bytes=12 * one + 30 * 8)                   # all of it: six first, six second pieces
    assert len(spy.shapes) == 1
    spy = make_spy()
    polyhedra.issubset_batch_chunked(pairs, spy, chunk_bytes=12 * one + 30 * 8 - 1)
    assert len(spy.shapes) == 2


def _level_lists(engine, **net):
    """The lists remove_subsets_many is given by the levels of one solve()."""
    seen = []
    orig = algorithm.remove_subsets_many

    def recording(lists, eng, *a, **k):
        seen.append([None if polys is None else list(polys) for polys in lists])
        return orig(lists, eng, *a, **k)
    algorithm.remove_subsets_many = recording
    try:
        ret = algorithm.solve(examples.setup("synthetic_pairs", **net), engine=engine)
    finally:
        algorithm.remove_subsets_many = orig
    assert ret["solved"]
    return seen


def test_remove_subsets_many_on_the_spy_engine():
    from oracle_engine import OracleEngine
    levels = _level_lists(OracleEngine(), pairs=12, n=8, m=8)
    assert sum(1 for lists in levels for polys in lists if polys is not None and len(polys) >= 2) >= 3
    calls = 0
    for prefilter in (True, False):
        for lists in levels:
            spy = make_spy()
            want = polyhedra.remove_subsets_many(lists, OracleEngine(), prefilter=prefilter)
            got = polyhedra.remove_subsets_many(lists, spy, prefilter=prefilter)
            assert len(want) == len(got)
            for w, g in zip(want, got):
                assert (w is None and g is None) or [id(P) for P in w] == [id(P) for P in g]
            calls += len(spy.shapes)
    assert calls >= 1
