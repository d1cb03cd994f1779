"""Rates of `implicit_bounds` on one GPU: the route of the jobs (the emptiness projection on the node solver,
then two LP jobs per row that is no explicit equality through qpn_solve_lps) against qpn_implicit_bounds, one job per polyhedron,
through implicit_bounds_batch(route="polyhedron") (host arrays) and as the bare call over device tensors.

  family     the non-empty cases of lp_cases.family_case at 16 x 8, seeds 0-19
  gauss      `--polys` polytopes lp_cases.bounded_batch at 48 x 24
  pinned     20 polytopes bounded_batch(300 + s, 1, 24, 24) with 6 rows pinned by an added opposite row (12 implicit equalities each)
  stacks     the constraint stacks check_convexity sends for `--pairs` synthetic pairs of (16, 16)
  solve      solve() on those pairs with the option on, qp_processing.IMPLICIT_BOUNDS_ROUTE at each value

Three rounds, the routes alternating in each; a host clock around a synchronise.  Prints one JSON line per measurement and one
with the medians per workload and route.
usage: python tools/implicit_bounds_rate.py [--polys 2000] [--pairs 200] [--rounds 3] [--skip-solve]"""
import argparse

import numpy as np

from rate_common import convexity_stacks, emit, examples, on_device, polyhedra, qpn_amd, quiet_solve, report
from qpn_amd import qp_processing
from qpn_amd.engine import colmajor

import lp_cases


def measure(what, trips, eng, rounds, tol):
    dev = [on_device(eng, (colmajor(A), l, u)) for _, _, A, l, u in polyhedra.pack_by_shape(trips)[0]]

    def bare():
        return [eng.implicit_bounds(*args, tol=tol) for args in dev]

    routes = (("jobs", lambda: polyhedra.implicit_bounds_batch(trips, eng, tol=tol, route="jobs")),
              ("polyhedron_host", lambda: polyhedra.implicit_bounds_batch(trips, eng, tol=tol, route="polyhedron")),
              ("polyhedron_device", bare))
    answers = {name: fn() for name, fn in routes}           # one untimed pass each
    differ = sum(int(np.sum(a[0] != b[0])) for a, b in zip(answers["jobs"], answers["polyhedron_host"]))
    outs = answers["polyhedron_device"]
    rows = sum(A.shape[0] for A, _, _ in trips)
    explicit = sum(int(np.sum((np.abs(l - u) <= tol) | (l == u))) for _, l, u in trips)
    info = dict(polys=len(trips), calls=len(dev), rows=rows, lps_jobs=2 * (rows - explicit), verdicts_differ=differ,
                equalities=int(sum(int(a[0].sum()) for a in answers["polyhedron_host"])),
                lps=int(sum(int(o["lps"].sum()) for o in outs)), iters=int(sum(int(o["iters"].sum()) for o in outs)))
    report(what, routes, rounds, **info)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--polys", type=int, default=2000)
    ap.add_argument("--pairs", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-solve", action="store_true")
    a = ap.parse_args()
    eng = qpn_amd.default_engine(0)
    emit(what="library", path=qpn_amd._lib.LIB_PATH)
    tol = 1e-6

    # (a) the three workloads of the CPU count
    fam = [lp_cases.family_case(s, shape=(16, 8))[:3] for s in range(20)]
    fam = [p for p, e in zip(fam, polyhedra.isempty_batch(fam, eng)) if not e]
    measure("family_16x8", fam, eng, a.rounds, tol)
    A, l, u = lp_cases.bounded_batch(100, a.polys, 48, 24)
    measure("gauss_48x24", [(A[b], l[b], u[b]) for b in range(a.polys)], eng, a.rounds, tol)
    pinned = []
    for s in range(20):
        A, l, u = (v[0] for v in lp_cases.bounded_batch(300 + s, 1, 24, 24))
        centre = np.linalg.lstsq(A, 0.5 * (l + u), rcond=None)[0]
        at = A[:6] @ centre
        pinned.append((np.vstack([A, -A[:6]]), np.concatenate([np.full(6, -np.inf), l[6:], np.full(6, -np.inf)]),
                       np.concatenate([at, u[6:], -at])))
    measure("pinned_30x24", pinned, eng, a.rounds, tol)

    # (b) the stacks of check_convexity
    net = lambda: examples.setup("synthetic_pairs", pairs=a.pairs, n=16, m=16, check_convexity=True)
    stacks = [(np.atleast_2d(A), l, u) for A, l, u in convexity_stacks(eng, a.pairs)]
    measure("stacks_16x16", stacks, eng, a.rounds, qp_processing.CONVEXITY_TOL)

    # (c) solve() with the option on, by either route
    if a.skip_solve:
        return

    def solve_with(route):
        def run():
            qp_processing.IMPLICIT_BOUNDS_ROUTE = route
            try:
                r = quiet_solve(net(), engine=eng)
            finally:
                qp_processing.IMPLICIT_BOUNDS_ROUTE = "jobs"
            assert r["solved"]
            return r
        return run

    xs = {route: solve_with(route)()["x_opt"] for route in ("jobs", "polyhedron")}
    report("solve_check_convexity", [(route, solve_with(route)) for route in ("jobs", "polyhedron")], a.rounds, pairs=a.pairs, n=16, m=16,
           same_x_opt=bool(xs["jobs"].tobytes() == xs["polyhedron"].tobytes()))


if __name__ == "__main__":
    main()
