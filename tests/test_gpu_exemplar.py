"""qpn_exemplar_polys (csrc/qpn_lp.hip) against its numpy twin polyhedra.exemplar_polys_host, bit for bit on every output, in every
kernel class and both memory modes, on the planted family of tests/exemplar_cases.py; its argument errors; and the host functions
that use it -- exemplar_slack_batch / combine_at with route="polyhedron" against today's route, solve() end to end with
qp_processing.EMPTINESS_ROUTE switched."""
from __future__ import annotations

import numpy as np
import pytest

import exemplar_cases
import goldenio as G
from exemplar_cases import EMPTY_OPEN, FAILURE, ITER_LIMIT, TOL

pytestmark = pytest.mark.gpu

INF = np.inf


def _both_modes(engine, A, l, u, ol, oh, **kw):
    """The kernel in host and in device mode against the twin.  -> the twin's answer."""
    import torch
    from qpn_amd import polyhedra
    from qpn_amd.engine import colmajor
    Ac = colmajor(A)
    want = polyhedra.exemplar_polys_host(Ac, l, u, ol, oh, **kw)
    exemplar_cases.same_bits(engine.exemplar_polys(Ac, l, u, ol, oh, **kw), want, "host mode")
    dv = f"cuda:{engine.device}"
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dv)
    b = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.uint8), device=dv)
    got = engine.exemplar_polys(f(Ac), f(l), f(u), b(ol), b(oh), **kw)
    assert all(hasattr(v, "cpu") for v in got.values())
    exemplar_cases.same_bits(got, want, "device mode")
    return want


@pytest.mark.parametrize("shape", [(1, 1), (3, 2), (8, 4), (24, 8)])
def test_the_family_equals_the_twin_bit_for_bit(engine, shape):
    """50 polyhedra, the five kinds mixed: the last workgroup of the wavefront class holds two of its four."""
    n, d = shape
    n0 = engine.calls["qpn_exemplar_polys"]
    A, l, u, ol, oh, empty, how = exemplar_cases.family_batch(shape, 50)
    assert engine.lp_kernel_class(2 * n + 1, d + 1) == 0
    want = _both_modes(engine, A, l, u, ol, oh, tol=TOL)
    assert engine.calls["qpn_exemplar_polys"] == n0 + 2
    assert np.array_equal(want["empty"].astype(bool), empty) and np.array_equal(want["how"], how)
    cut = _both_modes(engine, A, l, u, ol, oh, tol=TOL, opts=dict(max_iters=1))
    if shape == (24, 8):
        assert want["iters"].max() > 20 and (want["row"][how == EMPTY_OPEN] >= 0).all()
        assert np.all(cut["how"] == ITER_LIMIT) and np.all(cut["iters"] == 1) and np.isnan(cut["eps"]).all() and not cut["lam"].any()


def _class_shapes(engine):
    """(the largest wave-class n, the smallest workgroup-class n) at d = 12 and the smallest workspace-class n at d = 24: the class
    of a job is that of its slack LP, 2 n + 1 rows in d + 1 variables."""
    n0 = max(n for n in range(1, 120) if engine.lp_kernel_class(2 * n + 1, 13) == 0)
    n2 = min(n for n in range(1, 512) if engine.lp_kernel_class(2 * n + 1, 25) == 2)
    return (n0, 12), (n0 + 1, 12), (n2, 24)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_class_boundaries_equal_the_twin_bit_for_bit(engine, which):
    n, d = _class_shapes(engine)[which]
    cls = lambda n: engine.lp_kernel_class(2 * n + 1, d + 1)
    assert cls(n) == which and (which == 0 or cls(n - 1) == which - 1) and (which != 0 or cls(n + 1) == 1)
    A, l, u, ol, oh, empty, how = exemplar_cases.family_batch((n, d), 3 if which == 2 else 5, first=2 if which == 2 else 0)
    want = _both_modes(engine, A, l, u, ol, oh, tol=TOL)
    assert np.array_equal(want["empty"].astype(bool), empty) and np.array_equal(want["how"], how) and want["iters"].min() > 3
    if which == 2:
        assert how.tolist() == [exemplar_cases.HOW[k] for k in ("fat", "gap", "thin_open")]


def test_workspace_class_runs_a_second_chunk(engine):
    """More polyhedra of the workspace class than one chunk of the workspace holds.  A job takes its slice (more than 156 KiB in
    this class) and the rows of its slack LP ((2 n + 1) (d + 1) + 2 (2 n + 1) doubles) and a chunk is 256 MiB, so the count below is
    more than a chunk holds and the launcher's second chunk runs (`first` > 0).  Five distinct polyhedra, one of each kind, in
    turn: the twin solves five, every job equals its own."""
    import torch
    from qpn_amd import polyhedra
    from qpn_amd.engine import colmajor
    n, d = _class_shapes(engine)[2]
    rows_bytes = ((2 * n + 1) * (d + 1) + 2 * (2 * n + 1)) * 8
    count = (256 << 20) // ((156 << 10) + rows_bytes) + 5
    assert engine.lp_kernel_class(2 * n + 1, d + 1) == 2 and 500 < count < 1000
    A, l, u, ol, oh, empty, how = exemplar_cases.family_batch((n, d), 5, first=10)
    five = polyhedra.exemplar_polys_host(colmajor(A), l, u, ol, oh, tol=TOL)
    assert np.array_equal(five["how"], how)
    t = np.arange(count) % 5
    want = {k: np.ascontiguousarray(v[t]) for k, v in five.items()}
    host = (np.ascontiguousarray(colmajor(A)[t]), l[t], u[t], ol[t], oh[t])
    exemplar_cases.same_bits(engine.exemplar_polys(*host, tol=TOL), want, "host mode")
    dv = f"cuda:{engine.device}"
    got = engine.exemplar_polys(*(torch.as_tensor(np.ascontiguousarray(a), device=dv) for a in host), tol=TOL)
    assert all(hasattr(v, "cpu") for v in got.values())
    exemplar_cases.same_bits(got, want, "device mode")


def test_argument_errors_and_null_flags(engine):
    from qpn_amd import polyhedra
    from qpn_amd.engine import QpnError, colmajor
    # sizes beyond the limits
    for n, d in ((512, 2), (2, 256)):
        with pytest.raises(QpnError, match="size"):
            engine.exemplar_polys(np.zeros((1, d, n)), np.zeros((1, n)), np.ones((1, n)))
    assert engine.lp_kernel_class(2 * 511 + 1, 255 + 1) == 2
    # inconsistent shapes
    A, l, u, ol, oh, empty, how = exemplar_cases.family_batch((3, 2), 10)
    for bad in ((colmajor(A), l[:3], u, ol, oh), (colmajor(A), l, u[:, :2], ol, oh), (colmajor(A)[0], l, u, ol, oh), (colmajor(A), l, u, ol[:4], oh)):
        with pytest.raises(QpnError, match="inconsistent shapes"):
            engine.exemplar_polys(*bad)
    # no polyhedron
    got = engine.exemplar_polys(np.zeros((0, 2, 3)), np.zeros((0, 3)), np.zeros((0, 3)))
    assert got["empty"].shape == (0,) and got["lam"].shape == (0, 7)
    # null flags mean closed: the answer of zero flags, and of one array alone
    zero = np.zeros_like(ol)
    closed = _both_modes(engine, A, l, u, None, None, tol=TOL)
    exemplar_cases.same_bits(closed, polyhedra.exemplar_polys_host(colmajor(A), l, u, zero, zero, tol=TOL), "zero flags")
    assert np.all(closed["row"] == -1) and not closed["empty"][how == EMPTY_OPEN].any()
    _both_modes(engine, A, l, u, ol, None, tol=TOL)
    _both_modes(engine, A, l, u, None, oh, tol=TOL)
    # data the screen rejects: that polyhedron alone fails, with zeros
    A[4, 1, 1] = np.nan; l[7, 0] = INF
    bad = _both_modes(engine, A, l, u, ol, oh, tol=TOL)
    assert np.all(bad["how"][[4, 7]] == FAILURE) and np.array_equal(np.delete(bad["how"], [4, 7]), np.delete(how, [4, 7]))
    assert not bad["x"][[4, 7]].any() and not bad["lam"][[4, 7]].any() and np.isnan(bad["eps"][[4, 7]]).all()


# ---- the host functions on the polyhedron route against today's route ------------------------------------------------------------
def _node_solves(engine):
    return sum(v for k, v in engine.calls.items() if k.startswith("qpn_solve_nodes") or k == "qpn_solve_avi_batch")


def test_exemplar_slack_batch_on_the_polyhedron_route(engine):
    from qpn_amd import polyhedra
    polys, plant = exemplar_cases.family_polys(shapes=((1, 1), (3, 2), (8, 4), (24, 8)), count=15)
    e0, p0, s0 = engine.calls["qpn_exemplar_polys"], engine.calls["qpn_solve_lps"], _node_solves(engine)
    empty, example, eps = polyhedra.exemplar_slack_batch(polys, engine, tol=TOL, route="polyhedron")
    assert engine.calls["qpn_exemplar_polys"] - e0 == 4                                          # one call per shape
    assert engine.calls["qpn_solve_lps"] == p0 and _node_solves(engine) == s0                    # no LP job, no node solve
    want, _, eps0 = polyhedra.exemplar_slack_batch(polys, engine, tol=TOL)
    assert engine.calls["qpn_exemplar_polys"] - e0 == 4 and engine.calls["qpn_solve_lps"] > p0 and _node_solves(engine) > s0
    assert np.array_equal(empty, want) and np.array_equal(empty, plant)
    answered = ~np.isnan(eps0)
    assert np.array_equal(np.isnan(eps), ~answered) and np.all(np.abs(eps[answered] - eps0[answered]) <= 1e-8)
    for p, e, x in zip(polys, empty, example):
        assert (x is None) == bool(e)
        if not e:
            assert np.all(p.A @ x >= p.l - 2 * TOL) and np.all(p.A @ x <= p.u + 2 * TOL)
    assert np.array_equal(polyhedra.isempty_slack_batch(polys, engine, tol=TOL, route="polyhedron"), plant)


def test_combine_at_on_the_kink_on_the_polyhedron_route(engine):
    """tests/test_level_batch.py's hand-worked kink: the same membership assertions with the emptiness tests on qpn_exemplar_polys."""
    from qpn_amd.programs import Poly
    from qpn_amd.qp_processing import combine_at
    R1 = Poly(np.array([[0.0, 1.0], [1.0, 0.0]]), [0.0, -INF], [0.0, 0.0])
    R2 = Poly(np.array([[1.0, -1.0], [0.0, 1.0]]), [0.0, 0.0], [0.0, INF])
    S1 = Poly(np.array([[0.0, 1.0], [1.0, 0.0]]), [0.0, -INF], [0.0, 0.0])
    S2 = Poly(np.array([[1.0, 0.0], [0.0, 1.0]]), [0.0, 0.0], [0.0, 0.0])
    e0, p0, s0 = engine.calls["qpn_exemplar_polys"], engine.calls["qpn_solve_lps"], _node_solves(engine)
    out = combine_at([[R1], [R2]], [[S1], [S2]], np.zeros(2), engine, route="polyhedron")
    assert engine.calls["qpn_exemplar_polys"] > e0 and engine.calls["qpn_solve_lps"] == p0 and _node_solves(engine) == s0
    assert len(out) >= 2
    inside = lambda pt: any(P.contains(np.array(pt, float), tol=1e-9) for P in out)
    assert inside((0.0, 0.0))
    assert inside((-1.0, 0.0))                    # optimal under R1, outside R2: stays in the graph
    assert not inside((1.0, 1.0))                 # in R2 but not optimal under it: must go
    assert not inside((1.0, 0.5)) and not inside((-1.0, 1.0))        # outside both regions: complement-only products are skipped
    for P in out:
        assert P.vectorize()[0].shape[0] >= 2


def test_reference_end_to_end_cases_on_the_polyhedron_route(engine, monkeypatch):
    """tests/test_gpu_host_logic.py's test_reference_end_to_end_cases_on_gpu with qp_processing.EMPTINESS_ROUTE = "polyhedron": the same
    assertions, and every combine_many asks its emptiness questions of qpn_exemplar_polys alone."""
    from qpn_amd import algorithm, examples, qp_processing
    from qpn_amd.qp_processing import local_recipe_count
    assert qp_processing.EMPTINESS_ROUTE == "nodes"
    monkeypatch.setattr(qp_processing, "EMPTINESS_ROUTE", "polyhedron")
    inner = qp_processing.combine_many
    ran = []

    def counted(jobs, x, eng, **kw):
        prods = 0
        for regions, solutions in jobs:
            try:
                prods += len(qp_processing._combine_products(regions, solutions, x)[2])
            except RuntimeError:
                pass
        before = (engine.calls["qpn_exemplar_polys"], engine.calls["qpn_solve_lps"], _node_solves(engine))
        out = inner(jobs, x, eng, **kw)
        ran.append((prods, engine.calls["qpn_exemplar_polys"] - before[0], engine.calls["qpn_solve_lps"] - before[1], _node_solves(engine) - before[2]))
        return out

    monkeypatch.setattr(qp_processing, "combine_many", counted)
    c = G.load("simple_bilevel_cases.json")
    assert len(c["w"]) == 8
    e0 = engine.calls["qpn_exemplar_polys"]
    for w, xs, min_pieces in zip(c["w"], c["accepted_xy"], c["min_pieces_root_graph"]):
        net = examples.setup("simple_bilevel", gen_solution_map=True)
        ret = algorithm.solve(net, np.array(list(w) + c["x0"], float), engine=engine)
        assert ret["solved"], ret
        assert any(np.allclose(ret["x_opt"], list(w) + list(xy), atol=c["atol"]) for xy in xs), (w, ret["x_opt"])
        assert len(ret["Sol"][2]) >= min_pieces, (w, len(ret["Sol"][2]))
        assert local_recipe_count(net, 2, ret["x_opt"], ret["Sol"], engine=engine) >= min_pieces, w
    print("combine_many calls (products, exemplar, solve_lps, node solves):", ran)
    assert all(lp == 0 and nodes == 0 for _, _, lp, nodes in ran)
    assert all(ex >= 1 for prods, ex, _, _ in ran if prods)                # it rises whenever combine_many had a question
    assert (engine.calls["qpn_exemplar_polys"] > e0) == any(prods for prods, _, _, _ in ran)
