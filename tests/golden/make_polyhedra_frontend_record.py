#!/usr/bin/env python3
"""Writes tests/golden/polyhedra_frontend_record.json: what the batch front ends of polyhedra.py (exemplar_batch, issubset_batch,
issubset_batch_chunked, remove_subsets, remove_subsets_many, interior_members_batch, exemplar_slack_batch, isempty_slack_batch,
implicit_bounds_batch) answer on seeded batches of mixed shapes, on the oracle engine (the node-AVI routes) and on the twin engine
of tests/twin_engine.py (every route of the HIP engine, served by the numpy twins).  Per case: for every returned array the
dtype, the shape and the SHA-256 of its bytes; None or not per example; the text of an exception; and the twin engine's log of
(method, dtype and shape of every array argument) -- the calls, in their order.

The record pins the front ends ACROSS commits: it is written from the polyhedra.py of the commit BEFORE a change to the host
layer and tests/test_polyhedra_frontends_record.py recomputes it with the working tree's.  From that commit's file:

    git show <parent>:quadraticprogramnetworks.jl_amd/polyhedra.py > /tmp/parent_polyhedra.py
    python tests/golden/make_polyhedra_frontend_record.py --frontend /tmp/parent_polyhedra.py

(the file is loaded by path as a module of the working tree's package: its relative imports are the working tree's).  Without
--frontend it records the working tree's polyhedra.py.
"""
import argparse
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import qpn_amd  # noqa: E402,F401
from qpn_amd.programs import Poly  # noqa: E402

import exemplar_cases  # noqa: E402
import implicit_cases  # noqa: E402
import lp_cases  # noqa: E402
import subset_cases  # noqa: E402

RECORD = os.path.join(HERE, "polyhedra_frontend_record.json")
SHAPES = [(1, 1), (3, 2), (5, 2), (8, 4), (16, 8)]
INF = np.inf


def load_frontend(path=None):
    if path is None:
        from qpn_amd import polyhedra
        return polyhedra
    spec = importlib.util.spec_from_file_location("qpn_amd.polyhedra_under_record", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the inputs: seeded, small, at least two shapes mixed in every batch (item t has shape SHAPES[t % 5]) ----------------------
def triples(count, first=0, feasible=False):
    """Polyhedra of lp_cases' family, the shapes in turn; feasible: without the contradictory quarter of the seeds."""
    seeds = [s for s in range(first, first + 4 * count) if not (feasible and s % 4 == 1)][:count]
    return [lp_cases.family_case(s, shape=SHAPES[t % len(SHAPES)])[:3] for t, s in enumerate(seeds)]


def implicit_triples(count):
    return [implicit_cases.family_case(2 * t, SHAPES[1 + t % 4]) for t in range(count)] + [implicit_cases.PINNED]


def subset_pairs(count):
    """Pairs of subset_cases' family over three shapes in turn, every polyhedron one object that shows up in several pairs."""
    shapes = [(1, 1, 1), (3, 2, 2), (5, 4, 2), (16, 16, 8)]
    pairs = []
    for t in range(count):
        A1, l1, u1, A2, l2, u2 = subset_cases.family_pair(*shapes[t % len(shapes)], t)
        P1, P2 = (A1, l1, u1), (A2, l2, u2)
        pairs += [(P1, P2), (P1, P1), (P2, P1)]
    return pairs


def pieces(seed, k, d=3):
    """A list of Poly pieces in d variables for remove_subsets: boxes around seeded centres, every third one inside another, and
    rows of two shapes (a box has 2 or d rows)."""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(k):
        c = rng.standard_normal(d); w = 0.5 + rng.random(d)
        if t % 3 == 2:
            c, w = prev[0], 0.5 * prev[1]
        prev = (c, w)
        rows = d if t % 2 == 0 else 2
        out.append(Poly(np.eye(d)[:rows], (c - w)[:rows], (c + w)[:rows]))
    return out


def slack_polys():
    """exemplar_cases' planted family as Poly objects with open bounds, three shapes interleaved; then closed triples, a square
    equality system (the shortcut), a singular one, and an item without rows."""
    polys, _ = exemplar_cases.family_polys(shapes=((1, 1), (3, 2), (8, 4)), count=10)
    polys = [polys[10 * (t % 3) + t // 3] for t in range(30)]
    rng = np.random.default_rng(5)
    S = rng.standard_normal((3, 3)); b = rng.standard_normal(3)
    return polys + triples(10, first=200) + [(S, b, b.copy()), (np.ones((2, 2)), np.array([1.0, 2.0]), np.array([1.0, 2.0])),
                                             (np.zeros((0, 2)), np.zeros(0), np.zeros(0))]


def beyond_rows(rows, free):
    """A polyhedron in one variable with more rows than the kernels take: x in [0, 1] twice, the other rows x = 1/2 (explicit
    equalities) or, with `free`, no bound at all."""
    l = np.full(rows, -INF if free else 0.5); u = np.full(rows, INF if free else 0.5)
    l[:2] = 0.0; u[:2] = 1.0
    return np.ones((rows, 1)), l, u


# ---- digests ----------------------------------------------------------------------------------------------------------------------
def _arr(a):
    a = np.ascontiguousarray(a)
    return dict(dtype=str(a.dtype), shape=list(a.shape), sha256=hashlib.sha256(a.tobytes()).hexdigest())


def digest(value):
    """Arrays by dtype, shape and hash; lists and tuples item by item; None and Poly objects (by their rows) as they are."""
    if value is None:
        return None
    if isinstance(value, Poly):
        return [_arr(a) for a in value.vectorize()]
    if isinstance(value, (list, tuple)):
        return [digest(v) for v in value]
    return _arr(np.asarray(value))


def cases(fe):
    """The calls of the record -> [(name, call(engine), beyond, exact)].  beyond: the batch holds an item beyond the kernels' limits
    (it would pad the whole batch of an engine without the LP entries: the twin engine alone runs it).  exact: how the HIP
    engine's answer compares with the twin engine's -- True: every float goes through an LP entry (bit-equal); False: through the
    node solver; a list of polyhedra: exemplar_slack_batch's items without an open bound through solve_lps, the others through the
    node solver."""
    out = []
    add = lambda name, call, beyond=False, exact=False: out.append((name, call, beyond, exact))
    lp_r, ex_n = fe.LP_MAX_R + 1, fe.EX_MAX_N + 1
    add("exemplar_batch", lambda engine: fe.exemplar_batch(triples(30), engine))
    add("isempty_batch", lambda engine: fe.isempty_batch(triples(30, first=60), engine))
    pairs = subset_pairs(12)
    small = ((np.eye(1), np.array([0.25]), np.array([2.0])), beyond_rows(lp_r, free=True))     # (each has a bound the other lacks)
    add("issubset_batch", lambda engine: fe.issubset_batch(pairs, engine))
    add("issubset_batch beyond", lambda engine: fe.issubset_batch(pairs[:6] + [small, small[::-1]], engine), beyond=True)
    add("issubset_batch_chunked", lambda engine: fe.issubset_batch_chunked(pairs, engine, chunk_bytes=4000))
    add("remove_subsets", lambda engine: fe.remove_subsets(pieces(1, 6), engine))
    lists = [pieces(2, 5), None, pieces(3, 1), pieces(4, 7, d=2), []]
    for pre in (True, False):
        add(f"remove_subsets_many prefilter={pre}", lambda engine, pre=pre: fe.remove_subsets_many(lists, engine, prefilter=pre))
    add("interior_members_batch", lambda engine: fe.interior_members_batch(triples(30, first=120), engine))
    add("interior_members_batch chunk=4", lambda engine: fe.interior_members_batch(triples(30, first=120), engine, chunk=4))
    slack = slack_polys()
    tol = exemplar_cases.TOL
    for route in (None, "polyhedron"):
        exact = True if route else slack
        add(f"exemplar_slack_batch route={route}", lambda engine, route=route: fe.exemplar_slack_batch(slack, engine, tol=tol, route=route), exact=exact)
        add(f"exemplar_slack_batch not strict route={route}",
            lambda engine, route=route: fe.exemplar_slack_batch(slack, engine, tol=tol, strict=False, slack_cap=0.5, route=route), exact=exact)
        add(f"isempty_slack_batch route={route}", lambda engine, route=route: fe.isempty_slack_batch(slack, engine, x=np.zeros(8), route=route))
        add(f"exemplar_slack_batch beyond route={route}",
            lambda engine, route=route: fe.exemplar_slack_batch(slack[:8] + [beyond_rows(ex_n, free=False)], engine, tol=tol, route=route),
            beyond=True, exact=bool(route))
    feasible = implicit_triples(24)
    for route in ("jobs", "polyhedron"):
        add(f"implicit_bounds_batch route={route}", lambda engine, route=route: fe.implicit_bounds_batch(feasible, engine, route=route), exact=True)
        add(f"implicit_bounds_batch empty route={route}",
            lambda engine, route=route: fe.implicit_bounds_batch(feasible[:5] + triples(8, first=1) + feasible[5:9], engine, route=route), exact=True)
    add("implicit_bounds_batch beyond route=polyhedron",
        lambda engine: fe.implicit_bounds_batch(feasible[:6] + [beyond_rows(lp_r, free=False)], engine, route="polyhedron"), beyond=True, exact=True)
    return out


def answer(call, engine):
    """-> dict(result = what the call returned) or dict(raised = the text of its exception)."""
    try:
        return dict(result=call(engine))
    except Exception as e:                                       # (the text is part of the record)
        return dict(raised=f"{type(e).__name__}: {e}")


def record(fe):
    """The record of one front-end module: {case name [engine]: dict(result or raised, digested; on the twin engine its calls)}."""
    from oracle_engine import OracleEngine
    from twin_engine import TwinEngine
    rec = {}
    for name, call, beyond, _ in cases(fe):
        for tag, make in (("twin", TwinEngine),) if beyond else (("oracle", OracleEngine), ("twin", TwinEngine)):
            eng = make()
            got = answer(call, eng)
            if "result" in got:
                got["result"] = digest(got["result"])
            if tag == "twin":
                got["calls"] = eng.log
            rec[f"{name} [{tag}]"] = got
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frontend", default=None, help="the polyhedra.py to record (default: the working tree's)")
    ap.add_argument("--out", default=RECORD)
    a = ap.parse_args()
    cases = record(load_frontend(a.frontend))
    with open(a.out, "w") as f:                                  # a case per line
        f.write('{"source": "tests/golden/make_polyhedra_frontend_record.py", "cases": {\n')
        f.write(",\n".join(f" {json.dumps(k)}: {json.dumps(cases[k], sort_keys=True)}" for k in sorted(cases)))
        f.write("\n}}\n")
    print("wrote", a.out, len(cases), "cases")


if __name__ == "__main__":
    main()
