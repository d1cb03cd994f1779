"""qpn_convexity_nodes (csrc/qpn_convexity.hip) against the numpy restatement of check_qp_convexity
(test_convexity_host.convexity_restated), and QPNetOptions.check_convexity end to end on the HIP engine."""
from __future__ import annotations

import numpy as np
import pytest

from test_convexity_host import MSG, convexity_restated

pytestmark = pytest.mark.gpu

TOL = 1e-6
SIZES = [1, 4, 16, 31, 32, 33, 48, 64, 96, 128, 129, 200, 256]


def _orth(g, n):
    Q, R = np.linalg.qr(g.standard_normal((n, n)))
    return Q * np.sign(np.diag(R))


def _batch(n, m, g):
    """Nodes of every kind the kernel has to tell apart: skew parts, PSD with exact zero eigenvalues, smallest eigenvalue at
    -tol (1 +- 1e-4), indefinite; rows with random masks, duplicated and dependent equality rows.  -> (Qc, Ac, eq)."""
    Qds, As, eqs = [], [], []
    for kind in KINDS:
        A = g.standard_normal((m, n))
        eq = (g.random(m) < 0.5).astype(np.uint8)
        if kind == "skew":
            G = g.standard_normal((n, n)); K = g.standard_normal((n, n))
            Qd = G @ G.T / n + (K - K.T)
        elif kind == "psd_zero":
            G = g.standard_normal((n, max(1, n // 2)))
            Qd = G @ G.T / n
        elif kind in ("edge_in", "edge_out"):
            lam = g.uniform(0.5, 2.0, n)
            lam[0] = -TOL * (1 - 1e-4 if kind == "edge_in" else 1 + 1e-4)
            U = _orth(g, n)
            S = (U * lam) @ U.T
            S = 0.5 * (S + S.T)
            Qd = 0.5 * S
            eq[:] = 0                                           # Z = I: the eigenvalue is H's own
        elif kind == "indefinite":
            Qd = g.standard_normal((n, n))
        else:
            G = g.standard_normal((n, n))
            Qd = G @ G.T / n - 0.5 * np.eye(n)
            if m >= 3:                                          # duplicated and dependent rows, all selected
                A[1] = A[0]
                A[2] = 2.0 * A[0] - 0.5 * A[1 if m > 1 else 0]
                eq[:3] = 1
        Qds.append(Qd); As.append(A); eqs.append(eq)
    Qc = np.ascontiguousarray(np.swapaxes(np.stack(Qds), 1, 2))
    Ac = np.ascontiguousarray(np.swapaxes(np.stack(As), 1, 2)) if m else np.zeros((len(Qds), n, 0))
    eq = np.stack(eqs) if m else np.zeros((len(Qds), 0), np.uint8)
    return Qc, Ac, eq


def _clear(sv, thr):
    """the rank decision is not within reach of rounding: no singular value near the threshold"""
    if sv is None or sv.size == 0:
        return True
    return not np.any((sv > thr / 16) & (sv < thr * 16))


KINDS = ("skew", "psd_zero", "edge_in", "edge_out", "indefinite", "dependent")


@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_restatement(engine, n, capsys):
    import torch
    g = np.random.Generator(np.random.Philox(key=[7, n]))
    dropped = dict.fromkeys(KINDS, 0)
    for m in sorted({0, n // 2, 2 * n}):
        Qc, Ac, eq = _batch(n, m, g)
        cvx, lam, nd = engine.convexity_nodes(Qc, Ac, eq, tol=TOL)
        rc, rl, rn, svs, thrs = convexity_restated(Qc, Ac, eq, tol=TOL)
        S = Qc + np.swapaxes(Qc, 1, 2)
        for b in range(len(rc)):
            if not _clear(svs[b], thrs[b]):
                dropped[KINDS[b]] += 1
                continue
            assert nd[b] == rn[b], (n, m, b)
            assert cvx[b] == rc[b], (n, m, b, lam[b], rl[b])
            if np.isinf(rl[b]):
                assert np.isinf(lam[b]) and lam[b] > 0
            else:
                assert abs(lam[b] - rl[b]) <= 1e-9 * max(1.0, np.linalg.norm(S[b], 2)), (n, m, b, lam[b], rl[b])
        # inert padding rows (all zero, whatever their mask bit) change nothing
        pad = 16
        Ac2 = np.concatenate([Ac, np.zeros((Ac.shape[0], n, pad))], axis=2)
        eq2 = np.concatenate([eq, np.ones((eq.shape[0], pad), np.uint8)], axis=1)
        c2, l2, n2 = engine.convexity_nodes(Qc, Ac2, eq2, tol=TOL)
        assert np.array_equal(c2, cvx) and np.array_equal(l2, lam) and np.array_equal(n2, nd)
        # host and device inputs: the same outputs
        dev = "cuda:0"
        cd, ld, nd_d = engine.convexity_nodes(torch.tensor(Qc, device=dev), torch.tensor(Ac, device=dev),
                                              torch.tensor(eq, device=dev), tol=TOL)
        torch.cuda.synchronize()
        assert np.array_equal(cd.cpu().numpy(), cvx) and np.array_equal(ld.cpu().numpy(), lam)
        assert np.array_equal(nd_d.cpu().numpy(), nd)
    # Random rows sit clear of the rank threshold: nothing of the five kinds without planted dependence is left out.  The
    # `dependent` kind can be (the rounding residue of its dependent rows lands near the threshold); that kind is compared node
    # by node, with the rank known, in test_gpu_convexity_reference.
    with capsys.disabled():
        print(f"\n[convexity restatement n={n}] `dependent` nodes left out by the clearness filter: {dropped['dependent']} of 3")
    assert all(dropped[k] == 0 for k in KINDS if k != "dependent"), dropped


@pytest.mark.parametrize("n", [4, 48, 200])
def test_non_finite_input_is_not_convex(engine, n):
    g = np.random.Generator(np.random.Philox(key=[8, n]))
    Qc, Ac, eq = _batch(n, n, g)
    Qc[0, 0, 0] = np.nan
    Ac[1, 0, 0] = np.inf; eq[1, 0] = 1
    Ac[2, 0, 0] = np.nan; eq[2, 0] = 0                           # not selected: ignored
    cvx, lam, nd = engine.convexity_nodes(Qc, Ac, eq, tol=TOL)
    assert cvx[0] == 0 and np.isnan(lam[0]) and cvx[1] == 0 and np.isnan(lam[1])
    assert not np.isnan(lam[2])


def test_shapes_out_of_range_are_refused(engine):
    from qpn_amd.engine import QpnError
    with pytest.raises(QpnError):
        engine.convexity_nodes(np.zeros((1, 257, 257)), np.zeros((1, 257, 0)), np.zeros((1, 0), np.uint8))


def test_pairs_with_the_check_equal_pairs_without(engine):
    from qpn_amd import algorithm, examples
    off = algorithm.solve(examples.setup("synthetic_pairs", pairs=200, n=16, m=16), engine=engine)
    before = engine.calls["qpn_convexity_nodes"]
    on = algorithm.solve(examples.setup("synthetic_pairs", pairs=200, n=16, m=16, check_convexity=True), engine=engine)
    assert engine.calls["qpn_convexity_nodes"] > before
    assert on["solved"] == off["solved"]
    key = "x_opt" if off["solved"] else "x_fail"
    assert np.array_equal(on[key], off[key])


def _pair_with_bad_follower():
    """leader x0 (convex, box), followers (x1, x2) and (x3, x4) with boxes; the second follower's Q_dd = diag(1, -1)."""
    from qpn_amd.programs import QPNet
    net = QPNet(5)
    lead_c = net.add_constraint(np.array([[1.0]]), [-1.0], [1.0], cols=[0])
    fol = []
    for k, cols in enumerate(([1, 2], [3, 4])):
        c = net.add_constraint(np.eye(2), [-1.0, -1.0], [1.0, 1.0], cols=cols)
        Q = np.diag([1.0, -1.0]) if k == 1 else np.eye(2)
        Qf = np.zeros((3, 3)); Qf[1:, 1:] = Q; Qf[0, 1] = Qf[1, 0] = 0.2
        fol.append(net.add_qp(Qf, np.array([0.0, 0.1, 0.0]), [c], cols, idx=[0] + cols))
    lead = net.add_qp(np.eye(1), np.array([0.3]), [lead_c], [0], idx=[0])
    net.add_edges([(lead, f) for f in fol])
    net.assign_constraint_groups()
    net.default_initialization = np.zeros(5)
    return net, lead, fol


def test_non_convex_follower_is_reported(engine):
    from qpn_amd import NonConvexQPError, algorithm
    from qpn_amd.level_batch import process_level
    net, lead, fol = _pair_with_bad_follower()
    net.set_options(check_convexity=True)
    with pytest.raises(NonConvexQPError) as ei:
        process_level(net, sorted(fol), np.zeros(5), {}, engine=engine)
    assert ei.value.pid == fol[1] and ei.value.min_eig == pytest.approx(-2.0)
    res = algorithm.solve(net, engine=engine)
    assert res["solved"] is False and res["error"] == MSG.format(fol[1])
