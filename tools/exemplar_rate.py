"""Rates of the emptiness tests `exemplar` / `isempty` on one GPU: today's route (closed polyhedra as jobs of
qpn_solve_lps over slack LPs the host expands, polyhedra with an open bound as padded node records with Q = 0 on the node solver)
against qpn_exemplar_polys, one job per polyhedron, through isempty_slack_batch / exemplar_slack_batch(route="polyhedron") (host
arrays) and as the bare call over device tensors.

  kinks      isempty_slack_batch on the products _combine_products makes at the kinks of simple_bilevel (the cases of
             tests/golden/simple_bilevel_cases.json whose solve reaches combine_many), as a level of `--nodes` such nodes
  gauss      `--polys` polytopes lp_cases.bounded_batch at 24 x 12 with random open flags, every second one with a row pinned
             l = u and open below (empty by that bound)
  bare       the same polytopes, the qpn_exemplar_polys call alone over device tensors

Today's route runs on the same engine with the method hidden.  Three rounds, the routes alternating in each; a host clock around a
synchronise.  Prints one JSON line per measurement and one with the medians per workload and route.
usage: python tools/exemplar_rate.py [--polys 2000] [--nodes 200] [--rounds 3]"""
import argparse

import numpy as np

from rate_common import emit, examples, on_device, polyhedra, qpn_amd, quiet_solve, report, without
from qpn_amd.engine import colmajor
from qpn_amd.programs import Poly

import goldenio
import lp_cases

TOL = 1e-4


def kink_products(eng):
    """The products combine_many asks about in the solves of the golden simple_bilevel cases, per case that reaches it."""
    seen = []
    real = polyhedra.isempty_slack_batch

    def capture(polys, engine, **kw):
        seen.append(list(polys))
        return real(polys, engine, **kw)

    c = goldenio.load("simple_bilevel_cases.json")
    polyhedra.isempty_slack_batch = capture
    try:
        for w in c["w"]:
            quiet_solve(examples.setup("simple_bilevel", gen_solution_map=True), np.array(list(w) + c["x0"], float), engine=eng)
    finally:
        polyhedra.isempty_slack_batch = real
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--polys", type=int, default=2000)
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    eng = qpn_amd.default_engine(0)
    old = without(eng, "exemplar_polys")                    # (the host functions take today's route)
    emit(what="library", path=qpn_amd._lib.LIB_PATH)

    # (a) a level of kinked nodes: the products of the golden kinks, `--nodes` nodes in all
    kinks = kink_products(old)
    level = [p for k in range(a.nodes) for p in kinks[k % len(kinks)]]
    routes = (("nodes", lambda: polyhedra.isempty_slack_batch(level, old, tol=TOL, route="polyhedron")),
              ("polyhedron", lambda: polyhedra.isempty_slack_batch(level, eng, tol=TOL, route="polyhedron")))
    answers = {name: fn() for name, fn in routes}           # one untimed pass each
    shapes = sorted({p.A.shape for p in level})
    report("kinks_simple_bilevel", routes, a.rounds, nodes=a.nodes, products=len(level), shapes=[list(s) for s in shapes],
           open=int(sum(bool(p.open_lo.any() or p.open_hi.any()) for p in level)), empty=int(answers["polyhedron"].sum()),
           verdicts_differ=int(np.sum(answers["nodes"] != answers["polyhedron"])))

    # (b) polytopes with random open flags, every second one empty by an open pinned row
    g = np.random.default_rng(7)
    A, l, u = lp_cases.bounded_batch(100, a.polys, 24, 12)
    ol = g.random(l.shape) < 0.5; oh = g.random(l.shape) < 0.5
    k = g.integers(0, 24, a.polys)
    for b in range(0, a.polys, 2):
        l[b, k[b]] = u[b, k[b]] = 0.5 * (l[b, k[b]] + u[b, k[b]])
        ol[b, k[b]] = True
    polys = [Poly(A[b], l[b], u[b], normalise=False, open_lo=ol[b], open_hi=oh[b]) for b in range(a.polys)]
    routes = (("nodes", lambda: polyhedra.exemplar_slack_batch(polys, old, tol=TOL, strict=False, route="polyhedron")),
              ("polyhedron", lambda: polyhedra.exemplar_slack_batch(polys, eng, tol=TOL, strict=False, route="polyhedron")))
    answers = {name: fn() for name, fn in routes}
    report("gauss_24x12_open", routes, a.rounds, polys=a.polys, empty=int(answers["polyhedron"][0].sum()),
           unanswered={name: int(np.isnan(v[2]).sum()) for name, v in answers.items()},
           verdicts_differ=int(np.sum(answers["nodes"][0] != answers["polyhedron"][0])))

    # (c) the bare call over device tensors
    dev = on_device(eng, (colmajor(A), l, u, ol.astype(np.uint8), oh.astype(np.uint8)))
    out = eng.exemplar_polys(*dev, tol=TOL)
    how = out["how"].cpu().numpy()
    report("gauss_24x12_open_bare", (("polyhedron_device", lambda: eng.exemplar_polys(*dev, tol=TOL)),), a.rounds, polys=a.polys,
           how={str(v): int(np.sum(how == v)) for v in np.unique(how)}, iters=int(out["iters"].sum()),
           kernel_class=eng.lp_kernel_class(2 * 24 + 1, 12 + 1))


if __name__ == "__main__":
    main()
