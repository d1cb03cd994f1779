"""The numpy twins of the three LP entries (polyhedra.solve_lps_host, issubset_pairs_host, implicit_bounds_host) on degenerate
polyhedra whose answers are known by construction (tests/degenerate_cases.py): many rows through one vertex, a polyhedron that is
one point, a degenerate apex, the assignment polytope, rows repeated at scales 2**-20 .. 2**20, and non-finite data.

On every job: no certified outcome contradicts the plant (no INFEASIBLE / EMPTY on a set that has a point, no UNBOUNDED on a bounded
one, no wrong `sub`), no FAILURE and no ITER_LIMIT, objectives and extremes within 1e-8 * max(1, |planted|) (tests/test_lp_host.py's
bar against HiGHS), and lp_cases.check_certificates on every output of solve_lps_host."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment, linprog

import qpn_amd  # noqa: F401
from qpn_amd import polyhedra, polyhedra_host
from qpn_amd.engine import colmajor

import degenerate_cases as dc
import implicit_cases as ic
import lp_cases
import subset_cases as sc
from lp_cases import FAILURE, OPTIMAL

RTOL = 1e-8
PINNED = [((24, 6), range(20)), ((64, 12), range(20)), ((130, 24), range(8))]
SMALLER = PINNED[:2]


def _close(got, want):
    want = np.asarray(want, dtype=np.float64)
    return np.abs(np.asarray(got) - want) <= RTOL * np.maximum(1.0, np.abs(want))


def _row_lps(A, l, u):
    """Every (row, sign) LP over one polyhedron, cold.  -> (the twin's answer, the jobs' rows, signs)."""
    po, orow, osg = dc.row_jobs(A.shape[0])
    return polyhedra.solve_lps_host(colmajor(A[None]), l[None], u[None], po, obj_row=orow, obj_sign=osg), orow, osg


def _highs_min(c, A, l, u):
    rows = np.vstack([A[np.isfinite(u)], -A[np.isfinite(l)]]); rhs = np.concatenate([u[np.isfinite(u)], -l[np.isfinite(l)]])
    res = linprog(c, A_ub=rows, b_ub=rhs, bounds=[(None, None)] * A.shape[1], method="highs")
    assert res.status == 0, res.message
    return float(res.fun)


@pytest.mark.parametrize("shape,seeds", PINNED, ids=lambda v: str(v) if isinstance(v, tuple) else "")
def test_every_row_lp_over_a_single_point_is_optimal_at_it(shape, seeds):
    r, d = shape
    for seed in seeds:
        A, l, u, x0 = dc.pinned(seed, r, d)
        got, orow, osg = _row_lps(A, l, u)
        assert np.all(got["status"] == OPTIMAL), (seed, np.unique(got["status"], return_counts=True))
        want = osg * (A[orow] @ x0)
        err = np.abs(got["obj"] - want) / np.maximum(1.0, np.abs(want))
        assert np.all(err <= RTOL), (seed, err.max())
        assert np.all(got["iters"] < 50 * (r + 1 + d) + 100)
        for t in range(len(orow)):
            lp_cases.check_certificates(A, l, u, osg[t] * A[orow[t]], {k: v[t] for k, v in got.items()})


@pytest.mark.parametrize("shape,seeds", PINNED, ids=lambda v: str(v) if isinstance(v, tuple) else "")
def test_every_row_of_a_single_point_is_an_implicit_equality(shape, seeds):
    r, d = shape
    for seed in seeds:
        A, l, u, x0 = dc.pinned(seed, r, d)
        got = polyhedra.implicit_bounds_host(colmajor(A[None]), l[None], u[None], tol=1e-6)
        assert got["status"][0] == ic.OK, (seed, got["status"][0], got["fail_row"][0])
        assert got["eq"][0].all() and set(got["how"][0].tolist()) <= {ic.EXPLICIT, ic.IMPLICIT}
        assert np.all(np.abs(got["vals"][0] - A @ x0) <= 1e-6), (seed, np.abs(got["vals"][0] - A @ x0).max())


@pytest.mark.parametrize("shape,seeds", SMALLER + [((130, 24), range(6))], ids=lambda v: str(v) if isinstance(v, tuple) else "")
def test_a_single_point_inside_and_outside_a_box(shape, seeds):
    r, d = shape
    for seed in seeds:
        A, l, u, x0 = dc.pinned(seed, r, d)
        inside, outside = dc.box(x0 - 1e-3, x0 + 1e-3), dc.box(x0 + 1e-3, x0 + 1.0)
        second = tuple(np.stack([a, b]) for a, b in zip(inside, outside))
        got = polyhedra.issubset_pairs_host(colmajor(A[None]), l[None], u[None], colmajor(second[0]), second[1], second[2], [0, 0], [0, 1])
        assert got["how"].tolist()[0] == sc.HOLDS and got["how"][1] in (sc.BY_POINT, sc.BY_OPTIMUM), (seed, got["how"])
        assert got["sub"].tolist() == [1, 0]
        assert got["val"][1] < x0[got["bound"][1] // 2] + 1e-3 - 1e-6 and got["bound"][1] % 2 == 0      # a lower bound of the box refutes


@pytest.mark.parametrize("shape,seeds", SMALLER, ids=lambda v: str(v) if isinstance(v, tuple) else "")
def test_all_extremes_of_a_polytope_with_a_degenerate_apex(shape, seeds):
    r, d = shape
    for seed in seeds:
        A, l, u, x0 = dc.capped(seed, r, d)
        got = polyhedra.implicit_bounds_host(colmajor(A[None]), l[None], u[None], tol=1e-6, all_extremes=True)
        assert got["status"][0] == ic.OK, (seed, got["status"][0], got["fail_row"][0])
        lo, hi = got["lo"][0], got["hi"][0]
        assert np.all(_close(lo[:r], l[:r])), (seed, np.abs(lo[:r] - l[:r]).max())          # every cone row reaches its bound at x0
        want_hi = np.array([-_highs_min(-A[i], A, l, u) for i in range(r + 1)])
        assert np.all(_close(hi, want_hi)), (seed, np.abs(hi - want_hi).max())
        assert _close(lo[r], c_x0 := u[r] - 1.0) and hi[r] <= u[r] + 1e-6 * abs(u[r]), (seed, lo[r], c_x0, hi[r])
        l2, u2 = dc.relaxed(l, u)
        sub = polyhedra.issubset_pairs_host(colmajor(A[None]), l[None], u[None], colmajor(A[None]), l2[None], u2[None], [0], [0])
        assert sub["how"][0] == sc.HOLDS and sub["sub"][0] == 1, (seed, sub["how"][0])


@pytest.mark.parametrize("k", [3, 5, 8])
def test_the_assignment_polytope(k):
    for seed in range(4):
        A, l, u, c = dc.assignment(seed, k)
        d = k * k
        got = polyhedra.solve_lps_host(colmajor(A[None]), l[None], u[None], [0], cost=c[None])
        got = {key: v[0] for key, v in got.items()}
        rows, cols = linear_sum_assignment(c.reshape(k, k))
        want = float(c.reshape(k, k)[rows, cols].sum())
        assert got["status"] == OPTIMAL and _close(got["obj"], want), (seed, got["status"], got["obj"], want)
        lp_cases.check_certificates(A, l, u, c, got)
        if k == 8 and seed:                                     # (129 warm solves of 80 x 64 each: one seed at k = 8, all four below)
            continue
        ib = polyhedra.implicit_bounds_host(colmajor(A[None]), l[None], u[None], tol=1e-6, all_extremes=True)
        assert ib["status"][0] == ic.OK, (ib["status"][0], ib["fail_row"][0])
        assert np.array_equal(np.nonzero(ib["how"][0] == ic.EXPLICIT)[0], d + np.arange(2 * k))
        assert np.all(np.abs(ib["lo"][0][:d]) <= RTOL) and np.all(_close(ib["hi"][0][:d], 1.0))
        assert np.array_equal(ib["eq"][0], np.arange(d + 2 * k) >= d)


@pytest.mark.parametrize("row_scales", [False, True])
@pytest.mark.parametrize("shape", [(30, 6), (90, 16)])
def test_rows_repeated_at_many_scales_against_highs_on_the_base_polytope(shape, row_scales):
    r, d = shape
    for seed in range(20):
        A, l, u, c, base = dc.scaled_copies(seed, r, d, row_scales)
        got = polyhedra.solve_lps_host(colmajor(A[None]), l[None], u[None], [0], cost=c[None])
        got = {key: v[0] for key, v in got.items()}
        want = _highs_min(c, *base)
        assert got["status"] == OPTIMAL and _close(got["obj"], want), (seed, got["status"], got["obj"], want)
        lp_cases.check_certificates(A, l, u, c, got)
        Ab, lb, ub = base                                       # the point lies in the base polytope
        assert np.all(Ab @ got["x"] >= lb - 1e-6 * np.maximum(1.0, np.abs(lb))) and np.all(Ab @ got["x"] <= ub + 1e-6 * np.maximum(1.0, np.abs(ub)))


def test_the_cone_reaches_the_lowest_id_rule(monkeypatch):
    """min c'x over r = 130 rows through one vertex, c inside their normal cone: OPTIMAL at the vertex; and with LP_BLAND_AFTER out of
    reach at least one case takes different steps -- the family runs the branch "after 20 zero-length steps the lowest eligible id"."""
    runs = {}
    assert polyhedra.LP_BLAND_AFTER == 20
    for bland in (20, 10 ** 9):
        monkeypatch.setattr(polyhedra_host, "LP_BLAND_AFTER", bland)       # (patched where _lp_loop reads it)
        for seed in range(10):
            A, l, u, c, x0 = dc.cone(seed, 130, 24)
            got = polyhedra.solve_lps_host(colmajor(A[None]), l[None], u[None], [0], cost=c[None])
            runs[bland, seed] = {key: v[0] for key, v in got.items()}
            if bland == 20:
                assert got["status"][0] == OPTIMAL and _close(got["obj"][0], c @ x0), (seed, got["status"][0], got["obj"][0], c @ x0)
                lp_cases.check_certificates(A, l, u, c, runs[bland, seed])
    differ = [s for s in range(10) if runs[20, s]["iters"] != runs[10 ** 9, s]["iters"] or not np.array_equal(runs[20, s]["lam"], runs[10 ** 9, s]["lam"])]
    assert differ, "no case of cone(seed, 130, 24) takes the lowest-id branch"


@pytest.mark.parametrize("what", dc.NONFINITE_KINDS)
def test_non_finite_data_fails_with_zeros(what):
    A, l, u, c = dc.with_nonfinite(dc.cone(3, 12, 4), what)
    got = polyhedra.solve_lps_host(colmajor(A[None]), l[None], u[None], [0], cost=c[None])
    got = {key: v[0] for key, v in got.items()}
    assert got["status"] == FAILURE and 0 <= got["iters"] <= 50 * sum(A.shape) + 100
    assert not got["lam"].any() and not got["ray"].any()
    lp_cases.check_certificates(A, l, u, c, got)
    if what != "c":                                             # the polyhedron's own data: the feasibility solve fails the same way
        if what in ("A", "l", "u"):                             # (an infinite bound is settled by implicit_bounds' step (0) before it)
            ib = polyhedra.implicit_bounds_host(colmajor(A[None]), l[None], u[None], tol=1e-6)
            assert ib["status"][0] == ic.FAILURE and not ib["eq"][0].any() and ib["lps"][0] == 1 and ib["iters"][0] == 0
        sub = polyhedra.issubset_pairs_host(colmajor(A[None]), l[None], u[None], colmajor(np.eye(4)[None]), np.zeros((1, 4)), np.ones((1, 4)), [0], [0])
        assert sub["how"][0] == sc.FAILURE and sub["sub"][0] == 0


def test_a_non_finite_row_of_the_second_piece_fails_the_pair():
    """The objective of a warm solve is a row of P2 and passes no screen: a NaN or an infinity in it makes every comparison of the
    pricing false, the loop ends OPTIMAL at once, the check fails, and after the rebuild again: FAILURE at that bound, sub = 0."""
    A, l, u, _, x0 = dc.cone(3, 12, 4)
    for bad in (np.nan, np.inf):
        A2 = np.eye(4); A2[2, 1] = bad
        got = polyhedra.issubset_pairs_host(colmajor(A[None]), l[None], (l + 1.0)[None], colmajor(A2[None]), (x0 - 5.0)[None], (x0 + 5.0)[None], [0], [0])
        assert got["how"][0] == sc.FAILURE and got["sub"][0] == 0 and got["bound"][0] == 4 and got["val"][0] == 0.0


def _count_rebuilds(monkeypatch):
    n = [0]
    real = polyhedra_host._lp_rebuild               # (patched where _lp_finish looks it up)

    def counted(S, c):
        n[0] += 1
        return real(S, c)

    monkeypatch.setattr(polyhedra_host, "_lp_rebuild", counted)
    return n


def test_the_inputs_of_the_gpu_tests_reach_the_rebuild(monkeypatch):
    """tests/test_gpu_lp_degenerate.py compares the kernels with the twins on these inputs to exercise the kernel's rebuild of the
    dictionary: the twin must take it on them, in every kernel class and in all three entries.  The class boundaries at d = 24 and
    d = 128 are those of the slice formula of csrc/qpn_lp.hip (the GPU tests compute them from the library): 56, 57 and 139 rows."""
    n = _count_rebuilds(monkeypatch)

    def rebuilds(f, *args, **kw):
        n[0] = 0
        f(*args, **kw)
        return n[0]

    def implicit(case):
        A, l, u = case[:3]
        return rebuilds(polyhedra.implicit_bounds_host, colmajor(A[None]), l[None], u[None], tol=1e-6)

    def rows(case, jobs=None):
        A, l, u = case[:3]
        po, orow, osg = dc.row_jobs(A.shape[0])
        if jobs is not None:
            po = np.zeros(len(jobs), np.int32); orow = [j[0] for j in jobs]; osg = [j[1] for j in jobs]
        return rebuilds(polyhedra.solve_lps_host, colmajor(A[None]), l[None], u[None], po, obj_row=orow, obj_sign=osg)

    def box(case, first):
        A, l, u, x0 = case
        I = np.eye(len(x0))[:first]
        return rebuilds(polyhedra.issubset_pairs_host, colmajor(A[None]), l[None], u[None], colmajor(I[None]), (x0[:first] - 1e-3)[None],
                        (x0[:first] + 1e-3)[None], [0], [0])

    # the wavefront class: (65, 12) and the largest r at d = 24
    assert implicit(dc.pinned(0, 64, 12)) >= 1 and rows(dc.pinned(1, 64, 12)) >= 1
    assert implicit(dc.pinned(1, 55, 24)) >= 1 and box(dc.pinned(0, 55, 24), 16) >= 1
    # the workgroup class: the smallest r at d = 24, and (131, 24) with the job list of the GPU test
    assert implicit(dc.pinned(1, 56, 24)) >= 1
    big = dc.pinned(0, 130, 24)
    wrongly = [(1, -1), (35, 1), (43, -1), (55, 1), (71, 1), (110, -1), (114, -1), (115, -1)]
    assert rows(big, wrongly) == 8 and implicit(big) >= 8 and box(big, 24) >= 1
    # the workspace class
    assert implicit(dc.pinned(1, 138, 128)) >= 1


def test_a_failed_certificate_leaves_zeros():
    """A check that cannot pass (check_tol = 0 on Gaussian data: the dual residual is never exactly zero): the end is not certified,
    the dictionary is rebuilt and the loop run once more, the check fails again -- FAILURE, with lam and ray zero."""
    seen = 0
    for seed in range(40, 56):
        A, l, u, c, _ = lp_cases.family_case(seed, shape=(16, 8))
        kw = dict(cost=c[None])
        full = polyhedra.solve_lps_host(colmajor(A[None]), l[None], u[None], [0], **kw)
        got = polyhedra.solve_lps_host(colmajor(A[None]), l[None], u[None], [0], opts=dict(check_tol=0.0), **kw)
        if got["status"][0] != FAILURE:
            continue
        seen += 1
        assert not got["lam"].any() and not got["ray"].any() and got["iters"][0] >= full["iters"][0]
        assert full["status"][0] != FAILURE and (full["lam"].any() or full["ray"].any())
    assert seen >= 8
