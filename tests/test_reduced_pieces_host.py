"""qpn_reduced_pieces checked as SETS, on the CPU: the reference and the constants of tests/reduced_cases.py against the CPU twin
(tests/oracle_engine.py::OracleEngine.reduced_pieces) at every shape and kind the GPU test runs, three wrong eliminations that the
set-level check must catch, and the degenerate pieces' flags.  GPU side: tests/test_gpu_reduced_pieces.py."""
import numpy as np
import pytest

import reduced_cases as rc
from oracle import binding as ob
from oracle_engine import OracleEngine


@pytest.mark.parametrize("case", rc.CASES, ids=rc.case_id)
def test_twin_pieces_are_the_reference_sets(oracle, case):
    """The twin's rows let in every reference point inside the piece (TAU_IN) and keep out every one outside it (TAU_OUT) or off
    its equality manifold; the reference points themselves are balanced between the classes."""
    shape, kind = case
    c = rc.case(shape, kind)
    ins, out, skipped = rc.check_balance(shape, c["points"])
    got = rc.twin_output(shape, kind)
    worst = rc.check_pieces(got, c["points"])
    print(f"{rc.case_id(case)}: {len(c['K'])} pieces, inside {ins}, outside {out}, skipped {skipped}, worst inside {worst:.3e}")
    n, m, p = shape
    if kind != "mixed":           # every row two-sided: n + 2m rows are alive and each of the m columns retires one equality
        assert np.all(got[3] == n + m)
    assert np.all(got[3] <= n + 2 * m)


def _eliminate(args, K, node_of, mutate=None, tol=1e-9, ties=None):
    """The elimination the header of csrc/qpn_pieces.hip states, with one thing wrong on request:
    "bounds": l[k], u[k] are left alone; "pivot": the pivot row is not retired; "sign": f has the wrong sign.
    ties (a list): gets (pivot row, last row with an equal entry) of every pivot search that more than one row wins."""
    Qc, Rc, qd, Ac, Bc, l, u = args
    pieces = len(K)
    n = qd.shape[1]; m = l.shape[1]; p = Rc.shape[1]; N = n + m; cap = n + 2 * m
    Ar = np.zeros((pieces, n + p, cap)); lr = np.full((pieces, cap), -np.inf); ur = np.full((pieces, cap), np.inf)
    rows = np.zeros(pieces, np.int32); flags = np.zeros(pieces, np.int32)
    for t in range(pieces):
        b = int(node_of[t])
        A, lo, hi, keep = ob.local_piece(Qc[b].T, Rc[b].T.reshape(n, p), qd[b], Ac[b].T.reshape(m, n), Bc[b].T.reshape(m, p), l[b], u[b], K[t])
        alive = keep.astype(bool)
        for j in range(n, N):
            col = np.where(alive & (lo == hi) & np.isfinite(lo), np.abs(A[:, j]), 0.0)
            i = int(np.argmax(col))
            if col[i] <= tol:
                flags[t] |= int(np.any(alive & (np.abs(A[:, j]) > tol)))
                continue
            if ties is not None and np.count_nonzero(col == col[i]) > 1:
                ties.append((i, int(np.nonzero(col == col[i])[0][-1])))
            for k in np.nonzero(alive & (A[:, j] != 0.0))[0]:
                if k == i:
                    continue
                f = A[k, j] / A[i, j]
                if mutate == "sign":
                    f = -f
                A[k] = A[k] - f * A[i]; A[k, j] = 0.0
                if mutate != "bounds":
                    lo[k] = lo[k] - f * lo[i]; hi[k] = hi[k] - f * hi[i]
            alive[i] = mutate == "pivot"
        idx = np.nonzero(alive)[0][:cap]
        cols = list(range(n)) + list(range(N, N + p))
        Ar[t, :, :len(idx)] = A[np.ix_(idx, cols)].T
        lr[t, :len(idx)] = lo[idx]; ur[t, :len(idx)] = hi[idx]; rows[t] = len(idx)
    return Ar, lr, ur, rows, flags


@pytest.mark.parametrize("shape", [(5, 6, 3), (40, 33, 3)], ids=str)
def test_set_level_check_catches_wrong_eliminations(oracle, shape):
    """The local restatement equals the twin bit for bit; each of three mutations of it fails check_piece."""
    c = rc.case(shape, "gauss")
    for a, b in zip(_eliminate(c["args"], c["K"], c["node_of"]), rc.twin_output(shape, "gauss")):
        assert np.array_equal(a, b)
    for mutate in ("bounds", "pivot", "sign"):
        bad = _eliminate(c["args"], c["K"], c["node_of"], mutate)
        with pytest.raises(AssertionError):
            rc.check_pieces(bad, c["points"], flags_clear=False)
        # ... and on the node's own piece alone, the one with points of both classes
        with pytest.raises(AssertionError):
            rc.check_piece(bad[0][0], bad[1][0], bad[2][0], bad[3][0], c["points"][0])


@pytest.mark.parametrize("shape", [(64, 65, 2), (129, 129, 2), (256, 256, 2)], ids=str)
def test_box_rows_tie_in_the_pivot_search(oracle, shape):
    """The box records are the ties case in fact: pivot searches end with equal maxima, and where multiplier rows (n .. n+m-1) lie
    above row 256 the tied rows are in different strides of the kernel's loops -- in one thread's hands at 256 + 256 (rows k and
    k + 256), in two threads' with the lower row on the higher thread at 129 + 129 (rows k and k + 129 >= 256).  (At 64 + 65 the
    two rows of the second stride are constraint rows, which hold no multiplier.)"""
    c = rc.case(shape, "box")
    ties = []
    for a, b in zip(_eliminate(c["args"], c["K"], c["node_of"], ties=ties), rc.twin_output(shape, "box")):
        assert np.array_equal(a, b)
    assert len(ties) >= shape[1]
    far = [(i, k) for i, k in ties if i < 256 <= k]
    assert bool(far) == (sum(shape[:2]) > 256)
    if shape == (256, 256, 2):
        assert any((k - i) % 256 == 0 for i, k in far)
    if shape == (129, 129, 2):
        assert any(k % 256 < i % 256 for i, k in far)


@pytest.mark.parametrize("shape", rc.FLAG_SHAPES, ids=str)
def test_twin_flags_of_degenerate_pieces(oracle, shape):
    """Flags as constructed (reduced_cases.degenerate); the pieces next to the degenerate ones are clear and pass the set check."""
    d = rc.degenerate(shape)
    got = OracleEngine().reduced_pieces(*d["args"], d["K"], d["node_of"])
    assert got[4].tolist() == d["flags"].tolist(), list(zip(d["names"], got[4].tolist()))
    for t, pts in d["points"].items():
        rc.check_piece(got[0][t], got[1][t], got[2][t], got[3][t], pts)
    assert ("b: more than n active rows" in d["names"]) == (shape[1] > shape[0])


def test_reference_guards():
    """reference_points refuses the recipes it does not cover rather than answer for them."""
    rec = rc.records((5, 6, 3), "gauss")
    K = np.full(11, 2, np.uint8); K[5:] = 6
    rng = np.random.default_rng(0)
    K[5] = 8                                                          # a free multiplier on an ordinary row with l < u
    with pytest.raises(ValueError):
        rc.reference_points(rec, K, 0, rng)
    K[5] = 6; K[0] = 1
    with pytest.raises(ValueError):
        rc.reference_points(rec, K, 0, rng)
