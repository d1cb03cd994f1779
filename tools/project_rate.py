"""The two routes of a round's flagged solution-graph pieces, timed on the same pieces: 256 pieces of shape (5, 16, 6), each with
two equal active rows planted (row 1 := row 0 of [A B l u], rows 0..2 active), so that qpn_reduced_pieces flags every one.

  per_piece  what level_batch._reduce_on_host does per flagged piece: one qpn_local_pieces launch for one piece, the lifted
             piece read back, avi_solutions.eliminate_multipliers in Python -- 256 launches and read-backs.  Runs on any tree
             (the parent commit's route, unchanged here).
  batched    ONE qpn_project_pieces call on host arrays for all 256 (staging, both kernels and the read-back inside the clock),
             then the same Poly normalisation per piece, so that both routes end with the same product.  Runs where the engine
             has project_pieces; the two products are compared bit for bit first.

Warm-up rounds, then rounds with the routes alternating; one JSON line per measurement and one with the medians.
    python tools/project_rate.py [--pieces 256] [--rounds 7] [--warmup 2]"""
import argparse

import numpy as np

from rate_common import emit, report

import qpn_amd
from qpn_amd import avi_solutions, level_batch
from qpn_amd import synthetic as P
from qpn_amd.engine import colmajor
from qpn_amd.programs import Poly


def workload(pieces, n=5, m=16, p=6):
    Q, R, qd, A, B, l, u = P.synth_nodes(41, pieces, n, m, p)
    A[:, 1] = A[:, 0]; B[:, 1] = B[:, 0]; l[:, 1] = l[:, 0]; u[:, 1] = u[:, 0]
    K = np.full((pieces, n + m), 2, np.uint8); K[:, n:] = 6; K[:, n:n + 3] = 5
    rec = (colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u)
    return rec, K, np.arange(pieces, dtype=np.int32), (n, m, p)


def per_piece(eng, rec, K, n, m):
    out = []
    for t in range(len(K)):
        Ap, lp, up, keep = eng.local_pieces(*[a[t:t + 1] for a in rec], K[t][None], node_of=np.zeros(1, np.int32))
        rows = np.asarray(keep[0]).astype(bool)
        Pl = avi_solutions.eliminate_multipliers(Poly(np.asarray(Ap[0]).T[rows], np.asarray(lp[0])[rows], np.asarray(up[0])[rows],
                                                      normalise=False), n, m)
        out.append(Pl.vectorize())
    return out


def batched(eng, rec, K, node_of, n, m):
    Ar, lr, ur, rows, flags = eng.project_pieces(*rec, K, node_of, cap=level_batch.project_cap(n, m))
    assert not np.asarray(flags).any()
    return [Poly(np.ascontiguousarray(Ar[t, :, :rows[t]].T), lr[t, :rows[t]], ur[t, :rows[t]]).vectorize() for t in range(len(K))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pieces", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    eng = qpn_amd.default_engine(0)
    rec, K, node_of, (n, m, p) = workload(a.pieces)
    flags = np.asarray(eng.reduced_pieces(*rec, K, node_of)[4])
    assert np.all(flags == 1), "the workload's pieces are all flagged"
    routes = [("per_piece", lambda: per_piece(eng, rec, K, n, m))]
    if callable(getattr(eng, "project_pieces", None)):
        routes.append(("batched", lambda: batched(eng, rec, K, node_of, n, m)))
        one, two = per_piece(eng, rec, K, n, m), batched(eng, rec, K, node_of, n, m)
        same = all(x.tobytes() == y.tobytes() for u_, v_ in zip(one, two) for x, y in zip(u_, v_))
        emit(what="products", bit_equal=bool(same), rows=sorted({int(v[0].shape[0]) for v in two}))
        assert same
    for _ in range(a.warmup):
        for _, fn in routes:
            fn()
    report("flagged_pieces", routes, a.rounds, per=lambda s: {"pieces_per_s": a.pieces / s}, pieces=a.pieces, n=n, m=m, p=p)


if __name__ == "__main__":
    main()
