"""Rates of qpn_irredundant_bounds on one GPU, and what QPNetOptions.irredundant_pieces does to solve().

  flagged   256 flagged (5, 16, 6) pieces, tools/project_rate.py's workload, as qpn_project_pieces leaves them
  cases     the pieces of tests/irredundant_cases.pieces() (the twin outputs of tests/project_cases.py)
      bare_device   Engine.irredundant_bounds over packs already in HBM, one call per shape
      front_end     polyhedra.irredundant_batch on host arrays: packing, staging, the calls, the read-back, the Polys
    with the kernel's lps and iters and the rows before and after.
  solve     solve() on config 2 (robust_avoid_simple) and on `--pairs` synthetic pairs of (16, 16), the option off and on
            alternating: wall time, the rows of all pieces of the answer, and the record shapes (n, m) -> batch sizes the node
            solves and verifications of the run saw.

Warm-up rounds, then rounds with the routes alternating; a host clock around a synchronise.  One JSON line per measurement and one
with the medians.
    python tools/irredundant_rate.py [--pieces 256] [--rounds 7] [--warmup 2] [--pairs 200] [--solve-rounds 3] [--skip-solve]"""
import argparse

import numpy as np

from rate_common import emit, examples, on_device, polyhedra, qpn_amd, quiet_solve, report, timed
from qpn_amd import level_batch
from qpn_amd.engine import colmajor

import irredundant_cases
import project_rate


class Shapes:
    """The engine, with the (n, m) and batch of every solve_nodes / verify_nodes call noted."""

    def __init__(self, eng):
        self._eng, self.seen = eng, {}

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def _note(self, what, qd, l):
        key = f"{what} ({int(qd.shape[1])}, {int(l.shape[1])})"
        self.seen[key] = self.seen.get(key, 0) + int(qd.shape[0])

    def solve_nodes(self, Qc, Rc, qd, Ac, Bc, l, u, w, **kw):
        self._note("solve", qd, l)
        return self._eng.solve_nodes(Qc, Rc, qd, Ac, Bc, l, u, w, **kw)

    def verify_nodes(self, Qc, Rc, qd, Ac, Bc, l, u, xd, w, **kw):
        self._note("verify", qd, l)
        return self._eng.verify_nodes(Qc, Rc, qd, Ac, Bc, l, u, xd, w, **kw)


def rows_of(trips):
    return int(sum(np.count_nonzero(np.isfinite(l) | np.isfinite(u)) for _, l, u in trips))


def measure(what, trips, eng, rounds, warmup):
    packs = polyhedra.pack_by_shape(trips)[0]
    dev = [on_device(eng, (colmajor(A), l, u)) for _, _, A, l, u in packs]
    routes = (("bare_device", lambda: [eng.irredundant_bounds(*args) for args in dev]),
              ("front_end", lambda: polyhedra.irredundant_batch(trips, eng)))
    outs = routes[0][1]()
    pruned = routes[1][1]()
    status = np.concatenate([o["status"].cpu().numpy() for o in outs])
    info = dict(polys=len(trips), calls=len(dev), shapes=[list(p[0]) for p in packs][:6], rows_before=rows_of(trips),
                rows_after=int(sum(len(p) if hasattr(p, "vectorize") else np.count_nonzero(np.isfinite(p[1]) | np.isfinite(p[2])) for p in pruned)),
                ok=int(np.sum(status == 0)), empty=int(np.sum(status == 1)), other=int(np.sum(status > 1)),
                lps=int(sum(int(o["lps"].sum()) for o in outs)), iters=int(sum(int(o["iters"].sum()) for o in outs)))
    for _ in range(warmup):
        for _, fn in routes:
            fn()
    report(what, routes, rounds, per=lambda s: {"polys_per_s": len(trips) / s}, **info)


def solve_rounds(what, make, eng, rounds):
    """solve() with the option off and on, alternating, `rounds` rounds after one untimed pass of each."""
    answers = {}
    for on in (False, True):
        answers[on] = quiet_solve(make(on), engine=eng)
        assert answers[on]["solved"]
    emit(what=what, x_opt_max_diff=float(np.max(np.abs(answers[True]["x_opt"] - answers[False]["x_opt"]))))
    times = {False: [], True: []}
    for rnd in range(rounds):
        for on in (False, True):
            spy = Shapes(eng)
            c0 = dict(eng.calls)
            box = {}
            s = timed(lambda: box.setdefault("r", quiet_solve(make(on), engine=spy)))
            times[on].append(s)
            sol = box["r"]["Sol"]
            calls = {k: v - c0.get(k, 0) for k, v in eng.calls.items() if v != c0.get(k, 0)}
            emit(what=what, irredundant_pieces=on, round=rnd, seconds=s,
                 piece_rows=int(sum(len(p) for g in sol.values() if g is not None for p in g)),
                 pieces=int(sum(len(g) for g in sol.values() if g is not None)), records=spy.seen, calls=calls)
    emit(what=what, medians={"off": float(np.median(times[False])), "on": float(np.median(times[True]))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pieces", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=200)
    ap.add_argument("--solve-rounds", type=int, default=3)
    ap.add_argument("--skip-solve", action="store_true")
    a = ap.parse_args()
    eng = qpn_amd.default_engine(0)
    emit(what="library", path=qpn_amd._lib.LIB_PATH)

    rec, K, node_of, (n, m, p) = project_rate.workload(a.pieces)
    Ar, lr, ur, rows, flags = eng.project_pieces(*rec, K, node_of, cap=level_batch.project_cap(n, m))
    assert not np.asarray(flags).any()
    flagged = [(np.ascontiguousarray(Ar[t, :, :rows[t]].T), np.array(lr[t, :rows[t]]), np.array(ur[t, :rows[t]])) for t in range(a.pieces)]
    measure("flagged_5x16x6", flagged, eng, a.rounds, a.warmup)
    measure("project_cases", [(A, l, u) for _, A, l, u in irredundant_cases.pieces()], eng, a.rounds, a.warmup)

    if a.skip_solve:
        return
    solve_rounds("solve_config_2", lambda on: examples.setup("robust_avoid_simple", seed=1, irredundant_pieces=on), eng, a.solve_rounds)
    solve_rounds(f"solve_pairs_{a.pairs}x16x16", lambda on: examples.setup("synthetic_pairs", pairs=a.pairs, n=16, m=16, irredundant_pieces=on),
                 eng, a.solve_rounds)


if __name__ == "__main__":
    main()
