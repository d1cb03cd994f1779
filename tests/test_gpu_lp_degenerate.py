"""qpn_solve_lps, qpn_issubset_pairs and qpn_implicit_bounds (csrc/qpn_lp.hip) on the degenerate polyhedra of
tests/degenerate_cases.py: bit for bit against the numpy twins in host and device mode, and the planted answers checked on the
kernel's own outputs.  These inputs take the paths the Gaussian families never take: the rebuild of the dictionary after an end
that is not certified, the lowest-id rule after 20 zero-length steps, exact ties after row scaling,
and the data screen next to good jobs in one workgroup."""
from __future__ import annotations

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment, linprog

import degenerate_cases as dc
import implicit_cases as ic
import lp_cases
import subset_cases as sc
from lp_cases import FAILURE, OPTIMAL
from test_gpu_lp import _same_bits as lp_same_bits

pytestmark = pytest.mark.gpu

RTOL = 1e-8                                                  # tests/test_lp_host.py's bar against HiGHS


def _np(got):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in got.items()}


def _dev(engine, a, dtype):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=f"cuda:{engine.device}")


def _lps(engine, A, l, u, poly_of, opts=None, **obj):
    """solve_lps in host and device mode against the twin, bit for bit.  -> the KERNEL's host-mode answer."""
    from qpn_amd import polyhedra
    from qpn_amd.engine import colmajor
    Ac = colmajor(A)
    want = polyhedra.solve_lps_host(Ac, l, u, poly_of, opts=opts, **obj)
    got = _np(engine.solve_lps(Ac, l, u, poly_of, opts=opts, **obj))
    lp_same_bits(got, want, "host mode")
    dobj = {k: _dev(engine, v, np.float64 if k == "cost" else np.int32) for k, v in obj.items()}
    dgot = engine.solve_lps(*(_dev(engine, a, np.float64) for a in (Ac, l, u)), _dev(engine, poly_of, np.int32), opts=opts, **dobj)
    assert all(hasattr(v, "cpu") for v in dgot.values())
    lp_same_bits(dgot, want, "device mode")
    return got


def _subset(engine, A1, l1, u1, A2, l2, u2, pi, pj, **kw):
    """issubset_pairs in host and device mode against the twin, bit for bit.  -> the KERNEL's host-mode answer."""
    from qpn_amd import polyhedra
    from qpn_amd.engine import colmajor
    pi = np.asarray(pi, np.int32); pj = np.asarray(pj, np.int32)
    host = (colmajor(A1), l1, u1, colmajor(A2), l2, u2)
    want = polyhedra.issubset_pairs_host(*host, pi, pj, **kw)
    got = _np(engine.issubset_pairs(*host, pi, pj, **kw))
    sc.same_bits(got, want, "host mode")
    dgot = engine.issubset_pairs(*(_dev(engine, a, np.float64) for a in host), _dev(engine, pi, np.int32), _dev(engine, pj, np.int32), **kw)
    assert all(hasattr(v, "cpu") for v in dgot.values())
    sc.same_bits(dgot, want, "device mode")
    return got


def _implicit(engine, A, l, u, **kw):
    """implicit_bounds in host and device mode against the twin, bit for bit.  -> the KERNEL's host-mode answer."""
    from qpn_amd import polyhedra
    from qpn_amd.engine import colmajor
    host = (colmajor(A), l, u)
    want = polyhedra.implicit_bounds_host(*host, **kw)
    got = _np(engine.implicit_bounds(*host, **kw))
    ic.same_bits(got, want, "host mode")
    dgot = engine.implicit_bounds(*(_dev(engine, a, np.float64) for a in host), **kw)
    assert all(hasattr(v, "cpu") for v in dgot.values())
    ic.same_bits(dgot, want, "device mode")
    return got


def _close(got, want):
    want = np.asarray(want, dtype=np.float64)
    return np.abs(np.asarray(got) - want) <= RTOL * np.maximum(1.0, np.abs(want))


def _stack(cases):
    return tuple(np.stack([c[k] for c in cases]) for k in range(3))


def _rows_are_optimal_at_the_point(A, l, u, x0, poly_of, obj_row, obj_sign, got):
    assert np.all(got["status"] == OPTIMAL), np.unique(got["status"], return_counts=True)
    want = obj_sign * np.einsum("td,td->t", A[poly_of, obj_row], x0[poly_of])
    assert np.all(_close(got["obj"], want)), np.abs(got["obj"] - want).max()
    for t in range(len(poly_of)):
        b = poly_of[t]
        lp_cases.check_certificates(A[b], l[b], u[b], obj_sign[t] * A[b, obj_row[t]], {k: v[t] for k, v in got.items()})


def _boxes(x0, first):
    """The boxes x0 +- 1e-3 and [x0 + 1e-3, x0 + 1] on the first `first` coordinates, as two second pieces."""
    I = np.eye(len(x0))[:first]
    return np.stack([I, I]), np.stack([x0[:first] - 1e-3, x0[:first] + 1e-3]), np.stack([x0[:first] + 1e-3, x0[:first] + 1.0])


def _point_in_and_out_of_a_box(engine, A, l, u, x0, first):
    got = _subset(engine, A[None], l[None], u[None], *_boxes(x0, first), [0, 0], [0, 1])
    assert got["how"][0] == sc.HOLDS and got["how"][1] in (sc.BY_POINT, sc.BY_OPTIMUM) and got["sub"].tolist() == [1, 0], got["how"]


@pytest.mark.parametrize("shape", [(24, 6), (64, 12)])
def test_a_single_point_through_the_three_entries(engine, shape):
    """pinned(seed, r, d), seeds 0 and 1: every (row, sign) LP cold, the implicit bounds, the point in and out of a box."""
    r, d = shape
    cases = [dc.pinned(seed, r, d) for seed in (0, 1)]
    A, l, u = _stack(cases); x0 = np.stack([c[3] for c in cases])
    assert engine.lp_kernel_class(r + 1, d) == 0
    poly_of, obj_row, obj_sign = dc.row_jobs(r + 1, polys=2)
    got = _lps(engine, A, l, u, poly_of, obj_row=obj_row, obj_sign=obj_sign)
    _rows_are_optimal_at_the_point(A, l, u, x0, poly_of, obj_row, obj_sign, got)
    ib = _implicit(engine, A, l, u, tol=1e-6)
    assert np.all(ib["status"] == ic.OK) and ib["eq"].all()
    assert np.all(np.abs(ib["vals"] - np.einsum("brd,bd->br", A, x0)) <= 1e-6)
    for b in range(2):
        _point_in_and_out_of_a_box(engine, A[b], l[b], u[b], x0[b], d)


@pytest.mark.parametrize("shape", [(24, 6), (64, 12)])
def test_all_extremes_of_a_polytope_with_a_degenerate_apex(engine, shape):
    r, d = shape
    cases = [dc.capped(seed, r, d) for seed in (0, 1)]
    A, l, u = _stack(cases)
    ib = _implicit(engine, A, l, u, tol=1e-6, all_extremes=True)
    assert np.all(ib["status"] == ic.OK) and np.all(ib["lps"] == 1 + 2 * (r + 1))
    assert np.all(_close(ib["lo"][:, :r], l[:, :r])) and np.all(_close(ib["lo"][:, r], u[:, r] - 1.0))
    for b in range(2):                                          # the upper extremes: an independent solver on the same data
        rows = np.vstack([A[b, r:], -A[b, :r]]); rhs = np.concatenate([u[b, r:], -l[b, :r]])
        for i in (0, r // 2, r):
            res = linprog(-A[b, i], A_ub=rows, b_ub=rhs, bounds=[(None, None)] * d, method="highs")
            assert res.status == 0 and _close(ib["hi"][b, i], -res.fun), (b, i, ib["hi"][b, i], -res.fun)
    l2, u2 = dc.relaxed(l, u)
    sub = _subset(engine, A, l, u, A, l2, u2, [0, 1], [0, 1])
    assert np.all(sub["how"] == sc.HOLDS) and np.all(sub["sub"] == 1)


def test_the_assignment_polytope(engine):
    k, d = 5, 25
    cases = [dc.assignment(seed, k) for seed in range(4)]
    A, l, u = _stack(cases); c = np.stack([case[3] for case in cases])
    got = _lps(engine, A, l, u, np.arange(4, dtype=np.int32), cost=c)
    for b in range(4):
        rows, cols = linear_sum_assignment(c[b].reshape(k, k))
        assert got["status"][b] == OPTIMAL and _close(got["obj"][b], c[b].reshape(k, k)[rows, cols].sum())
        lp_cases.check_certificates(A[b], l[b], u[b], c[b], {key: v[b] for key, v in got.items()})
    ib = _implicit(engine, A, l, u, tol=1e-6, all_extremes=True)
    assert np.all(ib["status"] == ic.OK) and np.all((ib["how"] == ic.EXPLICIT) == (np.arange(d + 2 * k) >= d))
    assert np.all(np.abs(ib["lo"][:, :d]) <= RTOL) and np.all(_close(ib["hi"][:, :d], 1.0))


def _class_shapes(engine):
    """(the largest wave-class r, the smallest workgroup-class r, the smallest workspace-class r) at d = 24, 24, 128."""
    r0 = max(r for r in range(1, 200) if engine.lp_kernel_class(r, 24) == 0)
    r2 = min(r for r in range(1, 1025) if engine.lp_kernel_class(r, 128) == 2)
    return (r0, 24), (r0 + 1, 24), (r2, 128)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_a_single_point_at_the_class_boundaries(engine, which):
    """pinned(seed, r - 1, d) has r rows: row LPs cold over seeds 0 and 1, the implicit bounds of seed 1, the point of seed 0 in and
    out of a box on its first coordinates.  The twin takes 3.4 s for the 279 warm solves of the implicit bounds at 139 x 128, so the
    workspace class gets four row LPs and a box on four coordinates where the others get twelve and sixteen."""
    r, d = _class_shapes(engine)[which]
    assert engine.lp_kernel_class(r, d) == which and (which == 0 or engine.lp_kernel_class(r - 1, d) == which - 1)
    cases = [dc.pinned(seed, r - 1, d) for seed in (0, 1)]
    A, l, u = _stack(cases); x0 = np.stack([c[3] for c in cases])
    rows = [0, 0, r // 2, r // 2, r - 1, r - 1] if which < 2 else [r // 2, r - 1]
    poly_of = np.repeat([0, 1], len(rows)).astype(np.int32)
    obj_row = np.tile(rows, 2).astype(np.int32); obj_sign = np.tile([1, -1], len(rows)).astype(np.int32)
    got = _lps(engine, A, l, u, poly_of, obj_row=obj_row, obj_sign=obj_sign)
    _rows_are_optimal_at_the_point(A, l, u, x0, poly_of, obj_row, obj_sign, got)
    ib = _implicit(engine, A[1:], l[1:], u[1:], tol=1e-6)
    assert ib["status"][0] == ic.OK and ib["eq"].all() and np.all(np.abs(ib["vals"][0] - A[1] @ x0[1]) <= 1e-6)
    _point_in_and_out_of_a_box(engine, A[0], l[0], u[0], x0[0], 16 if which < 2 else 4)


# pinned(0, 130, 24): the (row, sign) LPs the commit before the dictionary was ever rebuilt answered INFEASIBLE -- with a Farkas
# vector that passed its check -- on a polyhedron that is one point (all 262 jobs of the seed were run through that commit's
# solve_lps_host; these eight were the ones not OPTIMAL), and eight of the others.
WRONGLY_INFEASIBLE = [(1, -1), (35, 1), (43, -1), (55, 1), (71, 1), (110, -1), (114, -1), (115, -1)]
OTHERS = [(0, 1), (0, -1), (35, -1), (64, 1), (64, -1), (115, 1), (130, 1), (130, -1)]


def test_the_rows_once_answered_infeasible_and_the_warm_chains_that_failed(engine):
    """(131, 24), seed 0: the job list above, then the implicit bounds and the point in and out of a box -- 263 and 49 warm solves from
    one dictionary, which end uncertified a dozen times and are rebuilt."""
    A, l, u, x0 = dc.pinned(0, 130, 24)
    assert engine.lp_kernel_class(131, 24) == 1
    jobs = WRONGLY_INFEASIBLE + OTHERS
    poly_of = np.zeros(len(jobs), np.int32); obj_row = np.array([j[0] for j in jobs], np.int32); obj_sign = np.array([j[1] for j in jobs], np.int32)
    got = _lps(engine, A[None], l[None], u[None], poly_of, obj_row=obj_row, obj_sign=obj_sign)
    _rows_are_optimal_at_the_point(A[None], l[None], u[None], x0[None], poly_of, obj_row, obj_sign, got)
    ib = _implicit(engine, A[None], l[None], u[None], tol=1e-6)
    assert ib["status"][0] == ic.OK and ib["eq"].all() and np.all(np.abs(ib["vals"][0] - A @ x0) <= 1e-6)
    _point_in_and_out_of_a_box(engine, A, l, u, x0, 24)


def test_the_cone_takes_the_lowest_id_rule(engine):
    """cone(seed, 130, 24), seeds 0..3: each takes other steps when the lowest-id rule is out of reach (67 / 63, 117 / 91, 92 / 55,
    64 / 43 steps with and without it in the twin; tests/test_lp_degenerate_host.py asserts that the family reaches the branch)."""
    cases = [dc.cone(seed, 130, 24) for seed in range(4)]
    A, l, u = _stack(cases); c = np.stack([case[3] for case in cases]); x0 = np.stack([case[4] for case in cases])
    got = _lps(engine, A, l, u, np.arange(4, dtype=np.int32), cost=c)
    assert np.all(got["status"] == OPTIMAL) and np.all(_close(got["obj"], np.einsum("bd,bd->b", c, x0)))
    assert got["iters"].min() > 20
    for b in range(4):
        lp_cases.check_certificates(A[b], l[b], u[b], c[b], {key: v[b] for key, v in got.items()})


def test_exact_ties_after_row_scaling(engine):
    """scaled_copies(seed, 30, 6, row_scales=False): the copies of a row are exact ties after scaling; the reference is HiGHS on the
    base polytope."""
    cases = [dc.scaled_copies(seed, 30, 6, False) for seed in range(20)]
    A, l, u = _stack(cases); c = np.stack([case[3] for case in cases])
    got = _lps(engine, A, l, u, np.arange(20, dtype=np.int32), cost=c)
    for b, case in enumerate(cases):
        Ab, lb, ub = case[4]
        res = linprog(c[b], A_ub=np.vstack([Ab, -Ab]), b_ub=np.concatenate([ub, -lb]), bounds=[(None, None)] * 6, method="highs")
        assert res.status == 0 and got["status"][b] == OPTIMAL and _close(got["obj"][b], res.fun), (b, got["status"][b], got["obj"][b], res.fun)
        lp_cases.check_certificates(A[b], l[b], u[b], c[b], {key: v[b] for key, v in got.items()})


def test_non_finite_data_next_to_good_jobs(engine):
    """Eleven jobs of 12 x 4 in one call, the wavefront class with four jobs per workgroup: the six kinds of non-finite data at the
    jobs 1, 2, 4, 7, 8, 10, good jobs between them, a last workgroup of three.  The bad jobs answer FAILURE at step 0 with zeros, as
    the twin does; the good ones what they answer in a call without the bad ones, to the bit."""
    from qpn_amd import polyhedra
    from qpn_amd.engine import colmajor
    good = [dc.cone(seed, 12, 4)[:4] for seed in (3, 4, 5, 6, 7)]
    bad = [dc.with_nonfinite(dc.cone(3, 12, 4), what) for what in dc.NONFINITE_KINDS]
    order = [("g", 0), ("b", 0), ("b", 1), ("g", 1), ("b", 2), ("g", 2), ("g", 3), ("b", 3), ("b", 4), ("g", 4), ("b", 5)]
    cases = [(good if kind == "g" else bad)[k] for kind, k in order]
    is_bad = np.array([kind == "b" for kind, _ in order])
    assert len(cases) % 4 != 0 and engine.lp_kernel_class(12, 4) == 0
    A, l, u = _stack(cases); c = np.stack([case[3] for case in cases])
    want = polyhedra.solve_lps_host(colmajor(A), l, u, np.arange(11), cost=c)
    got = _lps(engine, A, l, u, np.arange(11, dtype=np.int32), cost=c)
    assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["iters"], want["iters"])
    assert np.all(got["status"][is_bad] == FAILURE) and np.all(got["status"][~is_bad] == OPTIMAL) and not got["iters"][is_bad].any()
    for key in ("x", "obj", "lam", "ray"):
        assert np.array_equal(got[key][is_bad], want[key][is_bad], equal_nan=True), key
        assert not got[key][is_bad].any(), key
    alone = _lps(engine, A[~is_bad], l[~is_bad], u[~is_bad], np.arange(5, dtype=np.int32), cost=c[~is_bad])
    lp_same_bits({k: np.ascontiguousarray(v[~is_bad]) for k, v in got.items()}, alone, "good jobs next to bad ones")


def test_non_finite_data_through_the_feasibility_solve_and_in_the_second_piece(engine):
    """The screen inside lp_feasible: the five kinds in the polyhedron's own data as first pieces of qpn_issubset_pairs next to a good
    pair (six pairs, two workgroups), and the NaN kinds as polyhedra of qpn_implicit_bounds next to a good one (an infinite bound is
    settled by its step (0)).  A row of the second piece is the objective of a warm solve and passes no screen: a NaN or an infinity
    there ends that pair FAILURE through the check, as in the twin."""
    clean = dc.cone(3, 12, 4)
    A0, l0, x0 = clean[0], clean[1], clean[4]
    good = (A0, l0, l0 + 1.0)
    kinds = [k for k in dc.NONFINITE_KINDS if k != "c"]
    first = [good] + [dc.with_nonfinite(clean, k)[:3] for k in kinds]
    A1, l1, u1 = _stack(first)
    A2 = np.stack([np.eye(4)] * 3); A2[1, 2, 1] = np.nan; A2[2, 2, 1] = np.inf
    l2 = np.stack([x0 - 5.0] * 3); u2 = np.stack([x0 + 5.0] * 3)
    pi = [0, 1, 2, 3, 4, 5, 0, 0]; pj = [0, 0, 0, 0, 0, 0, 1, 2]
    sub = _subset(engine, A1, l1, u1, A2, l2, u2, pi, pj)
    assert sub["how"].tolist() == [sc.HOLDS] + [sc.FAILURE] * 7 and sub["sub"].tolist() == [1] + [0] * 7
    assert sub["lps"][1:6].tolist() == [1] * 5 and not sub["iters"][1:6].any() and sub["bound"][6:].tolist() == [4, 4]
    nan = [good] + [dc.with_nonfinite(clean, k)[:3] for k in ("A", "l", "u")]
    ib = _implicit(engine, *_stack(nan), tol=1e-6)
    assert ib["status"].tolist() == [ic.OK] + [ic.FAILURE] * 3 and not ib["eq"][1:].any() and not ib["iters"][1:].any()


def test_a_certificate_that_fails_after_the_rebuild_leaves_zeros(engine):
    """check_tol = 0 on Gaussian data: no dual residual is exactly zero, so the check fails, the dictionary is rebuilt, the loop runs
    once more and the check fails again: FAILURE with lam = ray = 0 from the kernel, where the same jobs at the default tolerance
    return their multipliers and rays."""
    A, l, u, cost, _, _, _ = lp_cases.family_batch((16, 8), list(range(40, 56)))
    poly_of = np.arange(16, dtype=np.int32)
    full = _lps(engine, A, l, u, poly_of, cost=cost)
    got = _lps(engine, A, l, u, poly_of, cost=cost, opts=dict(check_tol=0.0))
    failed = got["status"] == FAILURE
    assert failed.sum() >= 8 and not got["lam"][failed].any() and not got["ray"][failed].any()
    assert np.all(got["iters"][failed] >= full["iters"][failed]) and np.all(full["status"][failed] != FAILURE)
    assert np.all(full["lam"][failed].any(axis=1) | full["ray"][failed].any(axis=1))
