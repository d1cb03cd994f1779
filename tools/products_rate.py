"""Rates of combine's products on one GPU: combine_many with route="polyhedron" (every product stacked on the
host, tested against the point there and uploaded as a polyhedron of its own to qpn_exemplar_polys) against route="products" (every
candidate piece in a pool once, a product an index tuple, the closure and the emptiness test in qpn_exemplar_products), and the
bare qpn_exemplar_products calls over pools already in HBM.

  kinks      the combine_many calls of the solves of the golden simple_bilevel cases that reach it (tests/golden/
             simple_bilevel_cases.json), their nodes repeated to a level of `--nodes` nodes in all; a call keeps its own point
  bare       the qpn_exemplar_products calls route="products" made for that level, over device tensors

Three rounds, the routes alternating in each; a host clock around a synchronise.  Prints one JSON line per measurement and one with
the medians per workload and route.
usage: python tools/products_rate.py [--nodes 200] [--rounds 3]"""
import argparse

import numpy as np

from rate_common import emit, examples, on_device, qpn_amd, quiet_solve, report
from qpn_amd import qp_processing

import goldenio

TOL = 1e-4


def kink_calls(eng):
    """The (jobs, x) combine_many gets in the solves of the golden simple_bilevel cases, per call that has a job."""
    seen = []
    real = qp_processing.combine_many

    def capture(jobs, x, engine, **kw):
        if jobs:
            seen.append((list(jobs), np.array(x, dtype=np.float64)))
        return real(jobs, x, engine, **kw)

    c = goldenio.load("simple_bilevel_cases.json")
    qp_processing.combine_many = capture
    try:
        for w in c["w"]:
            quiet_solve(examples.setup("simple_bilevel", gen_solution_map=True), np.array(list(w) + c["x0"], float), engine=eng)
    finally:
        qp_processing.combine_many = real
    return seen


class Recorder:
    """The engine, with the arguments of its exemplar_products calls kept."""

    def __init__(self, eng):
        self._eng, self.seen = eng, []

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def exemplar_products(self, *args, **kw):
        self.seen.append((args, kw))
        return self._eng.exemplar_products(*args, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    eng = qpn_amd.default_engine(0)
    emit(what="library", path=qpn_amd._lib.LIB_PATH)

    calls = kink_calls(eng)
    reps = -(-a.nodes // sum(len(jobs) for jobs, _ in calls))
    level = [(jobs * reps, x) for jobs, x in calls]
    run = lambda engine, route: [qp_processing.combine_many(jobs, x, engine, tol=TOL, route=route) for jobs, x in level]
    routes = (("polyhedron", lambda: run(eng, "polyhedron")), ("products", lambda: run(eng, "products")))
    rec = Recorder(eng)
    answers = dict(polyhedron=run(eng, "polyhedron"), products=run(rec, "products"))       # one untimed pass each
    flat = {name: [P for call in got for pieces in call for P in pieces] for name, got in answers.items()}
    same = len(flat["polyhedron"]) == len(flat["products"]) and all(
        all(np.array_equal(s, t) for s, t in zip(P.vectorize() + (P.open_lo, P.open_hi), Q.vectorize() + (Q.open_lo, Q.open_hi)))
        for P, Q in zip(flat["polyhedron"], flat["products"]))
    asked = int(sum(args[6].shape[0] for args, _ in rec.seen))
    info = dict(nodes=int(sum(len(jobs) for jobs, _ in level)), combine_calls=len(level), products=asked, pieces_kept=len(flat["products"]),
                pieces_equal=bool(same), pool_rows=int(sum(args[0].shape[0] for args, _ in rec.seen)),
                shapes=sorted({(int(args[7]), int(args[0].shape[1])) for args, _ in rec.seen}))
    report("kinks_simple_bilevel", routes, a.rounds, **info)

    # the bare calls over pools already in HBM
    dev = []
    for args, kw in rec.seen:
        arrays = on_device(eng, args[:7] + (kw["point"], kw["point_of"]))
        rest = {k: v for k, v in kw.items() if k not in ("point", "point_of")}
        dev.append((arrays[:7] + (args[7],), dict(rest, point=arrays[7], point_of=arrays[8])))
    outs = [eng.exemplar_products(*args, **kw) for args, kw in dev]
    report("kinks_simple_bilevel_bare", (("products_device", lambda: [eng.exemplar_products(*args, **kw) for args, kw in dev]),), a.rounds,
           calls=len(dev), products=asked, near=int(sum(int(o["near"].sum()) for o in outs)), empty=int(sum(int(o["empty"].sum()) for o in outs)),
           iters=int(sum(int(o["iters"].sum()) for o in outs)))


if __name__ == "__main__":
    main()
