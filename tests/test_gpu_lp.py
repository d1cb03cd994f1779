"""qpn_solve_lps (csrc/qpn_lp.hip) against its numpy twin polyhedra.solve_lps_host, bit for bit on every output, in every kernel
class and both memory modes; its argument errors; and the host functions that use it -- implicit_bounds_batch, exemplar_slack_batch,
check_convexity end to end -- against the node-AVI route they took before (an engine wrapper that hides solve_lps)."""
from __future__ import annotations

import numpy as np
import pytest

import lp_cases
from lp_cases import FAILURE, INFEASIBLE, ITER_LIMIT, OPTIMAL, UNBOUNDED

pytestmark = pytest.mark.gpu

OUTPUTS = ("status", "iters", "x", "obj", "lam", "ray")


def _same_bits(got, want, what):
    for k in OUTPUTS:
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else np.asarray(got[k])
        w = np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        diff = np.nonzero(np.atleast_1d(g.view(np.uint8).reshape(g.shape[0], -1) != w.view(np.uint8).reshape(w.shape[0], -1)).any(axis=1))[0]
        assert diff.size == 0, (what, k, diff[:8], g[diff[:2]], w[diff[:2]])


def _both_modes(engine, A, l, u, poly_of, opts=None, **obj):
    """The kernel in host and in device mode against the twin.  -> the twin's answer."""
    import torch
    from qpn_amd import polyhedra
    from qpn_amd.engine import colmajor
    Ac = colmajor(A)
    want = polyhedra.solve_lps_host(Ac, l, u, poly_of, opts=opts, **obj)
    _same_bits(engine.solve_lps(Ac, l, u, poly_of, opts=opts, **obj), want, "host mode")
    dv = f"cuda:{engine.device}"
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dv)
    i = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=dv)
    dobj = {k: (f(v) if k == "cost" else i(v)) for k, v in obj.items()}
    got = engine.solve_lps(f(Ac), f(l), f(u), i(poly_of), opts=opts, **dobj)
    assert all(hasattr(v, "cpu") for v in got.values())
    _same_bits(got, want, "device mode")
    return want


@pytest.mark.parametrize("shape", [(1, 1), (3, 2), (2, 3), (5, 2), (16, 8)])
def test_small_shapes_equal_the_twin_bit_for_bit(engine, shape):
    r, d = shape
    seeds = list(range(40, 56))
    A, l, u, cost, poly_of, obj_row, obj_sign = lp_cases.family_batch(shape, seeds)
    assert engine.lp_kernel_class(r, d) == 0
    a = _both_modes(engine, A, l, u, np.arange(len(seeds), dtype=np.int32), cost=cost)
    b = _both_modes(engine, A, l, u, poly_of[:64], obj_row=obj_row[:64], obj_sign=obj_sign[:64])       # at most 64 jobs per call
    for t in range(len(seeds)):
        lp_cases.check_certificates(A[t], l[t], u[t], cost[t], {k: v[t] for k, v in a.items()})
    seen = set(a["status"].tolist()) | set(b["status"].tolist())
    assert seen <= {OPTIMAL, INFEASIBLE, UNBOUNDED}
    if shape == (16, 8):
        assert seen == {OPTIMAL, INFEASIBLE, UNBOUNDED} and a["iters"].max() > 3


def test_all_outcomes_and_the_iteration_limit(engine):
    """64 cases of the family in one call, and the same jobs cut off after three steps."""
    shape = (12, 6)
    seeds = list(range(64))
    A, l, u, cost, _, _, _ = lp_cases.family_batch(shape, seeds)
    full = _both_modes(engine, A, l, u, np.arange(64, dtype=np.int32), cost=cost)
    assert {OPTIMAL, INFEASIBLE, UNBOUNDED} == set(full["status"].tolist())
    cut = _both_modes(engine, A, l, u, np.arange(64, dtype=np.int32), cost=cost, opts=dict(max_iters=3))
    long = full["iters"] > 3
    assert long.any() and np.all(cut["status"][long] == ITER_LIMIT) and np.all(cut["iters"][long] == 3)
    assert np.array_equal(cut["status"][~long], full["status"][~long])


def _class_shapes(engine):
    """(the largest wave-class shape, the smallest workgroup-class shape, the smallest workspace-class shape) at d = 24, 24, 128."""
    r0 = max(r for r in range(1, 200) if engine.lp_kernel_class(r, 24) == 0)
    r2 = min(r for r in range(1, 1025) if engine.lp_kernel_class(r, 128) == 2)
    return (r0, 24), (r0 + 1, 24), (r2, 128)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_class_boundaries_equal_the_twin_bit_for_bit(engine, which):
    r, d = _class_shapes(engine)[which]
    assert engine.lp_kernel_class(r, d) == which and (which == 0 or engine.lp_kernel_class(r - 1, d) == which - 1)
    A, l, u = lp_cases.bounded_batch(7 + which, 3, r, d)
    u[0, 1] = l[0, 1]                                             # an equality row
    A[1, 1:, 0] = 0.0                                             # x_0 in row 0 alone, open below: that row has no minimum
    l[1] = A[1] @ np.ones(d) - 1.0; u[1] = l[1] + 2.0; l[1, 0] = -np.inf
    A[2, 1] = A[2, 0]; l[2, 1] = u[2, 0] + 1.0; u[2, 1] = np.inf  # a contradictory pair
    poly_of = np.array([0, 0, 1, 1, 1, 2], np.int32)
    obj_row = np.array([0, r - 1, 0, 0, 2, 3], np.int32); obj_sign = np.array([1, -1, 1, -1, -1, 1], np.int32)
    want = _both_modes(engine, A, l, u, poly_of, obj_row=obj_row, obj_sign=obj_sign)
    assert want["status"].tolist() == [OPTIMAL, OPTIMAL, UNBOUNDED, OPTIMAL, OPTIMAL, INFEASIBLE]
    assert want["iters"][:5].min() > 3
    for t in range(6):
        lp_cases.check_certificates(A[poly_of[t]], l[poly_of[t]], u[poly_of[t]], obj_sign[t] * A[poly_of[t], obj_row[t]],
                                    {k: v[t] for k, v in want.items()})


def test_workspace_class_runs_a_second_chunk(engine):
    """More jobs of the workspace class than one chunk of the workspace holds: a class-2 slice is larger than 156 KiB and a chunk is
    256 MiB, so 1685 jobs take at least two launches of the one launcher all three entries share (`first` > 0 in the second).  One
    polyhedron, six distinct objectives in turn, cut off after three steps: the twin solves six LPs, every job equals its own."""
    import torch
    from qpn_amd import polyhedra
    from qpn_amd.engine import colmajor
    r, d = _class_shapes(engine)[2]
    jobs = (256 << 20) // (156 << 10) + 5
    assert engine.lp_kernel_class(r, 128) == 2 and d == 128 and jobs == 1685
    A, l, u = lp_cases.bounded_batch(31, 1, r, d)
    Ac = colmajor(A)
    t = np.arange(jobs)
    poly_of = np.zeros(jobs, np.int32); obj_row = (t % 3).astype(np.int32); obj_sign = np.where(t % 6 < 3, 1, -1).astype(np.int32)
    opts = dict(max_iters=3)
    six = polyhedra.solve_lps_host(Ac, l, u, poly_of[:6], obj_row=obj_row[:6], obj_sign=obj_sign[:6], opts=opts)
    assert np.all(six["iters"] == 3) and len(set(six["obj"].tolist())) == 6
    want = {k: np.ascontiguousarray(v[t % 6]) for k, v in six.items()}
    _same_bits(engine.solve_lps(Ac, l, u, poly_of, obj_row=obj_row, obj_sign=obj_sign, opts=opts), want, "host mode")
    dv = f"cuda:{engine.device}"
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dv)
    i = lambda a: torch.as_tensor(a, device=dv)
    got = engine.solve_lps(f(Ac), f(l), f(u), i(poly_of), obj_row=i(obj_row), obj_sign=i(obj_sign), opts=opts)
    assert all(hasattr(v, "cpu") for v in got.values())
    _same_bits(got, want, "device mode")


def test_jobs_sharing_a_polyhedron(engine):
    """2 r jobs over the first polyhedron next to two over a second one: every job reads its polyhedron in place."""
    r, d = 11, 5
    A, l, u = lp_cases.bounded_batch(3, 2, r, d)
    poly_of = np.concatenate([np.zeros(2 * r), np.ones(2)]).astype(np.int32)
    obj_row = np.concatenate([np.repeat(np.arange(r), 2), [4, 4]]).astype(np.int32)
    obj_sign = np.tile([1, -1], r + 1).astype(np.int32)
    want = _both_modes(engine, A, l, u, poly_of, obj_row=obj_row, obj_sign=obj_sign)
    assert np.all(want["status"] == OPTIMAL)
    lo, hi = want["obj"][0::2], -want["obj"][1::2]                 # the extremes of every row: inside its bounds, lo <= hi
    rows = obj_row[0::2]; b = poly_of[0::2]
    assert np.all(lo <= hi + 1e-9) and np.all(lo >= l[b, rows] - 1e-6) and np.all(hi <= u[b, rows] + 1e-6)


def test_argument_errors(engine):
    import torch
    from qpn_amd.engine import QpnError, colmajor
    A, l, u = lp_cases.bounded_batch(5, 2, 4, 3)
    Ac = colmajor(A)
    ok = dict(obj_row=np.zeros(3, np.int32), obj_sign=np.ones(3, np.int32))
    for poly_of, obj in (([0, 2, 1], ok), ([0, -1, 1], ok), ([0, 1, 1], dict(ok, obj_row=np.array([0, 4, 0], np.int32))),
                         ([0, 1, 1], dict(ok, obj_row=np.array([0, -1, 0], np.int32)))):
        with pytest.raises(QpnError, match="bad argument|out of range"):
            engine.solve_lps(Ac, l, u, np.array(poly_of, np.int32), **obj)
    # the same indices in device arrays: that job alone fails, with zeros
    dv = f"cuda:{engine.device}"
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dv)
    got = engine.solve_lps(f(Ac), f(l), f(u), f(np.array([0, 2, -1, 1, 1], np.int32)), obj_row=f(np.array([0, 0, 0, 4, 1], np.int32)),
                           obj_sign=f(np.ones(5, np.int32)))
    st = got["status"].cpu().numpy()
    assert st.tolist() == [OPTIMAL, FAILURE, FAILURE, FAILURE, OPTIMAL]
    assert not got["x"][1:4].any() and not got["lam"][1:4].any() and not got["iters"][1:4].any()
    # sizes beyond the limits
    for r, d in ((1025, 2), (2, 257)):
        with pytest.raises(QpnError, match="size"):
            engine.solve_lps(np.zeros((1, d, r)), np.zeros((1, r)), np.ones((1, r)), np.zeros(1, np.int32), cost=np.zeros((1, d)))
    assert engine.lp_kernel_class(1025, 2) == -1 and engine.lp_kernel_class(1024, 256) == 2


# ---- the host functions on the LP route against the node-AVI route ---------------------------------------------------------
class _WithoutLps:
    """The engine without solve_lps: the host functions take the route they took before."""

    def __init__(self, eng):
        self._eng = eng

    def __getattr__(self, name):
        if name == "solve_lps":
            raise AttributeError(name)
        return getattr(self._eng, name)


def _random_polys(seed, count, dmax=6, mmax=10):
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
        if t % 3 == 1 and m >= 2:                      # contradictory pair: a'x <= -1 and a'x >= +1
            A[1] = A[0]; l[0], u[0] = -np.inf, c[0] - 1.0; l[1], u[1] = c[0] + 1.0, np.inf
        if t % 3 == 2 and m >= 2:                      # an equality row
            u[0] = l[0] = c[0]
        out.append((A, l, u))
    return out


def _node_solves(engine):
    return sum(v for k, v in engine.calls.items() if k.startswith("qpn_solve_nodes") or k == "qpn_solve_avi_batch")


def test_implicit_bounds_on_the_lp_route(engine):
    from qpn_amd import polyhedra
    polys = _random_polys(11, 40, dmax=5, mmax=8)
    polys = [p for p, e in zip(polys, polyhedra.isempty_batch(polys, engine)) if not e]
    pinned = (np.array([[1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]), np.array([1.0, -np.inf, 0.0]), np.array([np.inf, 1.0, np.inf]))
    polys.append(pinned)
    n0, s0 = engine.calls["qpn_solve_lps"], _node_solves(engine)
    got = polyhedra.implicit_bounds_batch(polys, engine)
    n1, s1 = engine.calls["qpn_solve_lps"], _node_solves(engine)
    want = polyhedra.implicit_bounds_batch(polys, _WithoutLps(engine))
    s2 = _node_solves(engine)
    shapes = {A.shape for A, l, u in polys if not np.all((l == u) | np.isclose(l, u, rtol=0, atol=1e-4))}
    assert n1 - n0 == len(shapes) and engine.calls["qpn_solve_lps"] == n1
    assert s1 - s0 == 1 and s2 - s1 >= 2                        # the emptiness projection alone; before: it and the LPs
    assert len(polys) >= 20
    for (eq, vals), (eq0, vals0) in zip(got, want):
        assert np.array_equal(eq, eq0)
        assert np.all(np.abs(vals[eq] - vals0[eq]) <= 1e-7)
    assert list(got[-1][0]) == [True, True, True] and np.allclose(got[-1][1], [1.0, 1.0, 0.0], atol=1e-9)
    with pytest.raises(RuntimeError):
        polyhedra.implicit_bounds_batch([(np.array([[1.0]]), np.array([1.0]), np.array([0.0]))], engine)


def test_exemplar_slack_on_the_lp_route(engine):
    from qpn_amd import polyhedra
    polys = _random_polys(12, 40, dmax=5, mmax=8)
    n0 = engine.calls["qpn_solve_lps"]
    empty, example, eps = polyhedra.exemplar_slack_batch(polys, engine, tol=1e-4)
    assert engine.calls["qpn_solve_lps"] > n0
    empty0, _, eps0 = polyhedra.exemplar_slack_batch(polys, _WithoutLps(engine), tol=1e-4)
    assert np.array_equal(empty, empty0) and empty.any() and not empty.all()
    assert np.all(np.abs(eps - eps0) <= 1e-8)
    for (A, l, u), e, x in zip(polys, empty, example):
        assert (x is None) == bool(e)
        if not e:
            assert np.all(A @ x >= l - 2e-4) and np.all(A @ x <= u + 2e-4)


def test_check_convexity_solves_its_lps_on_the_lp_kernel(engine):
    from qpn_amd import algorithm, examples
    off = algorithm.solve(examples.setup("synthetic_pairs", pairs=20, n=8, m=8), engine=engine)
    before = engine.calls["qpn_solve_lps"]
    on = algorithm.solve(examples.setup("synthetic_pairs", pairs=20, n=8, m=8, check_convexity=True), engine=engine)
    assert engine.calls["qpn_solve_lps"] > before
    assert on["solved"] and off["solved"]
    assert on["x_opt"].tobytes() == off["x_opt"].tobytes()
