"""Rates of combine's intersection tree on one GPU: combine_many with route="products" (every tuple of
candidates an LP job of qpn_exemplar_products, the tuples enumerated on the host) against route="tree" (qpn_intersection_trees: the
lists go up, prefixes are pruned depth by depth on the device, no tuple is formed on the host), and the bare calls of either route
over pools already in HBM.

  kinks      section 5k's own workload: the combine_many calls of the solves of the golden simple_bilevel cases, their nodes repeated
             to a level of `--nodes` nodes in all (two unions a node: only depth 1 can prune)
  boxes      `--box-nodes` nodes of three unions of 12 boxes of tests/tree_cases.py's family around one point

Three rounds, the routes alternating in each; a host clock around a synchronise.  Prints one JSON line per measurement and one with
the medians per workload and route; the candidates the walk tested stand next to the tuples the products route sends.
usage: python tools/tree_rate.py [--nodes 200] [--box-nodes 50] [--rounds 3]"""
import argparse
import os

import numpy as np

from rate_common import ROOT, emit, on_device, qpn_amd, report
from products_rate import kink_calls
from qpn_amd import qp_processing
from qpn_amd.programs import Poly

TOL = 1e-4


class Recorder:
    """The engine, with the arguments and the counts of its exemplar_products and intersection_trees calls kept."""

    def __init__(self, eng):
        self._eng, self.products, self.trees, self.tested = eng, [], [], 0

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def exemplar_products(self, *args, **kw):
        self.products.append((args, kw))
        return self._eng.exemplar_products(*args, **kw)

    def intersection_trees(self, *args, **kw):
        self.trees.append((args, kw))
        out = self._eng.intersection_trees(*args, **kw)
        self.tested += int(np.asarray(out["tested"]).sum())
        return out


def box_level(nodes, per_list=12, d=2):
    """`nodes` jobs of combine_many: three unions of `per_list` boxes each, no region (no complement piece), all at one point."""
    g = np.random.default_rng(12)
    jobs = []
    for _ in range(nodes):
        sols = []
        for _ in range(3):
            boxes = []
            for _ in range(per_list):
                lo = 0.5 * g.integers(0, 3, d)
                boxes.append(Poly(np.eye(d), lo, lo + np.where(g.integers(0, 2, d) == 1, 0.9, 0.4)))
            sols.append(boxes)
        jobs.append(([[], [], []], sols))
    return [(jobs, np.full(d, 0.7))]


def same_pieces(a, b):
    fa = [P for call in a for pieces in call for P in pieces]; fb = [P for call in b for pieces in call for P in pieces]
    return len(fa) == len(fb) and all(all(np.array_equal(s, t) for s, t in zip(P.vectorize() + (P.open_lo, P.open_hi), Q.vectorize() + (Q.open_lo, Q.open_hi)))
                                      for P, Q in zip(fa, fb))


def replay(eng, seen, n_arrays):
    """Recorded calls whose first `n_arrays` arguments are arrays, over device tensors: -> [(args, kw)]."""
    dev = []
    for args, kw in seen:
        arrays = on_device(eng, list(args[:n_arrays]) + [kw["point"], kw["point_of"]])
        rest = {k: v for k, v in kw.items() if k not in ("point", "point_of")}
        dev.append((arrays[:n_arrays] + tuple(args[n_arrays:]), dict(rest, point=arrays[-2], point_of=arrays[-1])))
    return dev


def measure(eng, what, level, rounds):
    run = lambda engine, route: [qp_processing.combine_many(jobs, x, engine, tol=TOL, route=route) for jobs, x in level]
    rec = Recorder(eng)
    answers = dict(products=run(rec, "products"))                          # one untimed pass each
    sent = int(sum(args[6].shape[0] for args, _ in rec.products))
    by_products = list(rec.products)
    rec.products = []
    answers["tree"] = run(rec, "tree")
    info = dict(nodes=int(sum(len(jobs) for jobs, _ in level)), combine_calls=len(level), tuples_products_route=sent, tested_tree_route=rec.tested,
                tree_calls=len(rec.trees), tuples_fallen_back=int(sum(args[6].shape[0] for args, _ in rec.products)),
                pieces_kept=int(sum(len(p) for call in answers["tree"] for p in call)), pieces_equal=bool(same_pieces(answers["products"], answers["tree"])))
    report(what, (("products", lambda: run(eng, "products")), ("tree", lambda: run(eng, "tree"))), rounds, **info)
    # the bare calls over pools already in HBM (L, cap: the scalars between the arrays)
    dev_p = replay(eng, by_products, 7)
    dev_t = []
    for args, kw in rec.trees:
        A, l, u, ol, oh, pr, L, lp, lm, lr, cap = args
        arrays = on_device(eng, [A, l, u, ol, oh, pr, lp, lm, lr, kw["point"], kw["point_of"]])
        rest = {k: v for k, v in kw.items() if k not in ("point", "point_of")}
        dev_t.append((arrays[:6] + (L,) + arrays[6:9] + (cap,), dict(rest, point=arrays[9], point_of=arrays[10])))
    report(what + "_bare", (("products_device", lambda: [eng.exemplar_products(*args, **kw) for args, kw in dev_p]),
                            ("tree_device", lambda: [eng.intersection_trees(*args, **kw) for args, kw in dev_t])), rounds,
           products_calls=len(dev_p), tree_calls=len(dev_t), tuples_products_route=sent, tested_tree_route=rec.tested)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200)
    ap.add_argument("--box-nodes", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    eng = qpn_amd.default_engine(0)
    emit(what="library", path=os.path.relpath(qpn_amd._lib.LIB_PATH, ROOT))        # (relative: the record names no machine)
    calls = kink_calls(eng)
    reps = -(-a.nodes // sum(len(jobs) for jobs, _ in calls))
    measure(eng, "kinks_simple_bilevel", [(jobs * reps, x) for jobs, x in calls], a.rounds)
    measure(eng, "boxes_3x12", box_level(a.box_nodes), a.rounds)


if __name__ == "__main__":
    main()
