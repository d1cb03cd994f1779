"""QPNetOptions.check_convexity on the host logic: check_qp_convexity (src/qp_processing.jl:39-55), its wiring into
verify_solution / process_qp / process_level / solve, and the default-off path.  The engine is the CPU oracle with a numpy
`convexity_nodes` that restates the reference's steps 2-5 (svd + eigvalsh); the -m gpu twin checks the HIP kernel against
the same restatement."""
from __future__ import annotations

import numpy as np
import pytest

import qpn_amd  # noqa: F401
from qpn_amd import algorithm, examples
from qpn_amd.level_batch import process_level
from qpn_amd.programs import Poly, QPNet
from qpn_amd.qp_processing import (NonConvexQPError, check_convexity_items, check_qp_convexity, process_qp,
                                   verify_solution)

INF = np.inf
MSG = "QP {} is not convex. Exiting."


def convexity_restated(Qc, Ac, eq, tol=1e-6):
    """numpy restatement of check_qp_convexity's steps 2-5 on engine-layout blocks (Qc [b, n, n], Ac [b, n, m] column-major,
    eq [b, m]): rank by Julia's rule over the selected rows that are not all zero, Z from the full SVD, eigvalsh of
    Z' (Qd + Qd') Z.  -> (convex [b], min_eig [b], null_dim [b], sv [b] the singular values, thr [b] the rank threshold)."""
    Qc = np.asarray(Qc, dtype=np.float64); Ac = np.asarray(Ac, dtype=np.float64); eq = np.asarray(eq)
    batch, n = Qc.shape[0], Qc.shape[-1]
    convex = np.zeros(batch, np.int32); lam = np.zeros(batch); nd = np.zeros(batch, np.int32)
    svs, thrs = [], []
    for b in range(batch):
        Qd = Qc[b].T
        A = Ac[b].T if Ac.shape[-1] else np.zeros((0, n))
        rows = eq[b].astype(bool) & np.any(A != 0, axis=1) if A.shape[0] else np.zeros(0, bool)
        Ae = A[rows]
        if not (np.all(np.isfinite(Qd)) and np.all(np.isfinite(Ae))):
            convex[b], lam[b], nd[b] = 0, np.nan, -1
            svs.append(None); thrs.append(None)
            continue
        if Ae.shape[0]:
            _, sv, Vt = np.linalg.svd(Ae, full_matrices=True)
            thr = min(Ae.shape) * np.finfo(float).eps * sv.max()
            r = int(np.sum(sv > thr))
            Z = Vt[r:].T
        else:
            sv, thr, r, Z = np.zeros(0), 0.0, 0, np.eye(n)
        svs.append(sv); thrs.append(thr)
        H = Z.T @ (Qd + Qd.T) @ Z
        nd[b] = n - r
        if H.size == 0:
            convex[b], lam[b] = 1, INF
        else:
            lam[b] = float(np.linalg.eigvalsh(H).min())
            convex[b] = int(lam[b] > -tol)
    return convex, lam, nd, svs, thrs


def _engine():
    from oracle_engine import OracleEngine

    class ConvexityOracle(OracleEngine):
        def convexity_nodes(self, Qc, Ac, eq, tol=1e-6):
            cvx, lam, nd, _, _ = convexity_restated(Qc, Ac, eq, tol)
            return cvx, lam, nd

    return ConvexityOracle()


def _plain():
    from oracle_engine import OracleEngine
    return OracleEngine()


def _leaf(pinned=False, players=1, nonconvex=(0,)):
    """`players` independent one-node QPs on (x1, x2) each; player k's Q_dd is diag(1, -1) if k in `nonconvex`, else I.
    Every player has the box x1 in [-1, 1]; `pinned` adds x2 >= 0 and x2 <= 0 as two rows with l < u."""
    net = QPNet(2 * players)
    for k in range(players):
        cols = [2 * k, 2 * k + 1]
        rows = [net.add_constraint(np.array([[1.0, 0.0]]), [-1.0], [1.0], cols=cols)]
        if pinned:
            rows.append(net.add_constraint(np.array([[0.0, 1.0]]), [0.0], [INF], cols=cols))
            rows.append(net.add_constraint(np.array([[0.0, 1.0]]), [-INF], [0.0], cols=cols))
        Q = np.diag([1.0, -1.0]) if k in nonconvex else np.eye(2)
        net.add_qp(Q, np.array([0.5, 0.0]), rows, cols, idx=cols)
    net.add_edges([])
    net.assign_constraint_groups()
    net.default_initialization = np.zeros(2 * players)
    return net


def _same(a, b):
    assert a["solved"] == b["solved"]
    if a["solved"]:
        assert np.array_equal(a["x_opt"], b["x_opt"])
    else:
        assert np.array_equal(a["x_fail"], b["x_fail"])


@pytest.mark.parametrize("name,kw", [("simple_bilevel", {}), ("synthetic_pairs", dict(pairs=3, n=3, m=2))])
def test_default_off_makes_no_convexity_call_and_changes_nothing(name, kw):
    eng = _engine()
    got = algorithm.solve(examples.setup(name, **kw), engine=eng)
    assert eng.calls["convexity_nodes"] == 0
    _same(got, algorithm.solve(examples.setup(name, **kw), engine=_plain()))


def test_non_convex_leaf_raises_and_solve_reports_it():
    eng = _engine()
    net = _leaf()
    pid = next(iter(net.qps))
    qp = net.qps[pid]
    P = net.constraints[qp.constraint_indices[0]].poly
    with pytest.raises(NonConvexQPError) as ei:
        check_qp_convexity(qp.f.Q, P.A, P.l, P.u, net.decision_inds(pid), pid, engine=eng)
    assert ei.value.pid == pid and str(ei.value) == MSG.format(pid) and ei.value.min_eig == pytest.approx(-2.0)
    assert isinstance(ei.value, RuntimeError)
    with pytest.raises(NonConvexQPError) as ei:
        verify_solution(qp, pid, [P], net.decision_inds(pid), np.zeros(2), True, engine=eng)
    assert ei.value.pid == pid
    net.set_options(check_convexity=True)
    with pytest.raises(NonConvexQPError) as ei:
        process_qp(net, pid, np.zeros(2), {}, engine=eng)
    assert ei.value.pid == pid
    res = algorithm.solve(net, engine=eng)
    assert res["solved"] is False and res["error"] == MSG.format(pid) and res["x_opt"] is None


def test_equality_found_by_implicit_bounds_makes_the_leaf_convex():
    eng = _engine()
    net = _leaf(pinned=True)
    pid = next(iter(net.qps))
    qp = net.qps[pid]
    cons = [net.constraints[c].poly for c in qp.constraint_indices]
    A = np.vstack([P.A for P in cons]); l = np.concatenate([P.l for P in cons]); u = np.concatenate([P.u for P in cons])
    assert np.all(l < u)                                       # no explicit equality: only implicit_bounds sees x2 = 0
    lam, nd = check_qp_convexity(qp.f.Q, A, l, u, net.decision_inds(pid), pid, engine=eng)
    assert nd == 1 and lam == pytest.approx(2.0)
    net.set_options(check_convexity=True)
    res = algorithm.solve(net, engine=eng)
    assert eng.calls["convexity_nodes"] >= 1
    _same(res, algorithm.solve(_leaf(pinned=True), engine=_plain()))


@pytest.mark.parametrize("name,kw", [("simple_bilevel", {}), ("synthetic_pairs", dict(pairs=3, n=3, m=2))])
def test_convex_net_same_result_with_the_option_on(name, kw):
    eng = _engine()
    on = algorithm.solve(examples.setup(name, check_convexity=True, **kw), engine=eng)
    assert eng.calls["convexity_nodes"] >= 1
    _same(on, algorithm.solve(examples.setup(name, **kw), engine=_plain()))


def test_results_are_kept_per_node_and_pieces():
    eng = _engine()
    net = _leaf(players=2, nonconvex=())
    players = sorted(net.qps)
    pin = Poly.from_local(4, [2, 3], np.array([[0.0, 1.0]]), [0.0], [0.0])       # x4 = 0: on player 2's variables
    items = [(players[0], []), (players[1], [pin])]
    check_convexity_items(net, items, eng)
    assert eng.calls["convexity_nodes"] == 1                    # one call for the one record shape
    check_convexity_items(net, items, eng)                      # same nodes, same pieces: nothing new to check
    assert eng.calls["convexity_nodes"] == 1
    check_convexity_items(net, [(players[1], [Poly(pin.A, pin.l, pin.u)])], eng)   # another piece object: checked again
    assert eng.calls["convexity_nodes"] == 2


def test_first_failure_in_player_order():
    eng = _engine()
    net = _leaf(players=3, nonconvex=(1, 2))
    net.set_options(check_convexity=True)
    players = sorted(net.qps)
    with pytest.raises(NonConvexQPError) as ei:
        process_level(net, players, np.zeros(6), {}, engine=eng)
    assert ei.value.pid == players[1]
    with pytest.raises(NonConvexQPError) as ei:
        process_level(net, players[::-1], np.zeros(6), {}, engine=eng)
    assert ei.value.pid == players[2]


def test_first_failure_in_product_order():
    """Sub-piece combinations are checked in Iterators.product order: under a piece that pins x2 the node is convex, under
    one that does not it is not; the first combination that is not raises."""
    eng = _engine()
    net = _leaf()
    pid = next(iter(net.qps))
    pin = Poly(np.array([[0.0, 1.0]]), [0.0], [0.0])
    free = Poly(np.array([[0.0, 1.0]]), [-1.0], [1.0])
    check_convexity_items(net, [(pid, [pin])], eng)            # convex
    with pytest.raises(NonConvexQPError) as ei:
        check_convexity_items(net, [(pid, [pin]), (pid, [free])], eng)
    assert ei.value.pid == pid
