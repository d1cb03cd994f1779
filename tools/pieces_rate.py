"""Rates of the uncapped solution-graph route (QPNetOptions.max_pieces = None) on one GPU.

  finish     qpn_finish_pieces in device mode, pieces/s, on synthetic reduced pieces at (n, m) = (16, 16), (32, 32), (64, 64)
  level      level_batch.solution_pieces wall time on one level of followers with 1024 recipes each, three routes: the capped
             host body expanding all 1024 (max_pieces=1024), the uncapped route on the numpy twin (an engine without
             finish_pieces), the uncapped device route
  solve      algorithm.solve() wall time on 40 synthetic pairs at (32, 32), capped (default) and uncapped

Prints one JSON line per measurement.  usage: python tools/pieces_rate.py [--pieces 1024] [--reps 5] [--nodes 8]"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import qpn_amd  # noqa: E402
from qpn_amd import algorithm, examples, level_batch  # noqa: E402
from qpn_amd.avi_solutions import _probe_vector  # noqa: E402
from qpn_amd.programs import QPNet  # noqa: E402


def synth(n, m, P, seed=0):
    g = np.random.default_rng(seed)
    p = n
    oc, cap = n + p, n + 2 * m
    rec_of = (np.arange(P) % 4).astype(np.int32)
    ncols = np.full(4, oc, np.int32)
    take = np.tile(np.arange(oc, dtype=np.int32), (4, 1))
    xk = g.standard_normal((4, oc)); probe = np.tile(_probe_vector(oc), (4, 1))
    rows = g.integers(cap // 2, cap + 1, size=P).astype(np.int32)
    Ar = g.standard_normal((P, oc, cap))
    Ar *= np.arange(cap)[None, None, :] < rows[:, None, None]
    ax = np.einsum("tcr,tc->tr", Ar, xk[rec_of])
    lr = ax - np.abs(g.standard_normal((P, cap))); ur = ax + np.abs(g.standard_normal((P, cap)))
    pad = np.arange(cap)[None, :] >= rows[:, None]
    lr[pad] = -np.inf; ur[pad] = np.inf
    return Ar, lr, ur, rows, np.zeros(P, np.int32), rec_of, ncols, take, xk, probe, n, m


def many_recipe_net(nodes, d=10):
    """`nodes` copies of the counterexample pair of tests/test_complete_solution_graphs.py with d = 10: every follower has
    2^10 = 1024 recipes at the start."""
    nv = 2 * d * nodes
    net = QPNet(nv)
    leads, fols = [], []
    for k in range(nodes):
        xs = list(range(2 * d * k, 2 * d * k + d)); ys = list(range(2 * d * k + d, 2 * d * (k + 1)))
        A = np.zeros((d, nv)); A[np.arange(d), ys] = 1.0
        cid = net.add_constraint(A, np.zeros(d), np.full(d, np.inf))
        Qf = np.zeros((nv, nv)); Qf[np.ix_(xs + ys, xs + ys)] = np.block([[np.eye(d), -np.eye(d)], [-np.eye(d), np.eye(d)]])
        fols.append(net.add_qp(Qf, np.zeros(nv), [cid], ys))
        Ql = np.zeros((nv, nv)); Ql[np.ix_(xs, xs)] = np.eye(d)
        ql = np.zeros(nv); ql[ys[-1]] = -1.0
        leads.append(net.add_qp(Ql, ql, [], xs))
    net.add_edges(list(zip(leads, fols)))
    net.assign_constraint_groups()
    net.default_initialization = np.zeros(nv)
    return net, fols


class NoFinish:
    """The engine without finish_pieces: solution_pieces then runs the uncapped route on the numpy twin."""
    def __init__(self, eng):
        self._eng = eng
        self.device = -1

    def __getattr__(self, name):
        if name == "finish_pieces":
            raise AttributeError(name)
        return getattr(self._eng, name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pieces", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=8)
    ap.add_argument("--pairs", type=int, default=40)
    a = ap.parse_args()
    import torch
    eng = qpn_amd.default_engine(0)
    dv = "cuda:0"
    for n in (16, 32, 64):
        args = synth(n, n, a.pieces)
        d = [torch.as_tensor(np.ascontiguousarray(v), device=dv) for v in args[:10]] + list(args[10:])
        eng.finish_pieces(*d)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = eng.finish_pieces(*d)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        med = float(np.median(ts))
        print(json.dumps(dict(what="finish_pieces", n=n, m=n, p=n, pieces=a.pieces, stored=out["stored"], median_s=med,
                              pieces_per_s=a.pieces / med)), flush=True)

    net, fols = many_recipe_net(a.nodes)
    x = net.default_initialization
    recs, batches, rets = level_batch.verify_items(net, [(pid, []) for pid in fols], x, eng)
    want = [bool(r["solution"]) for r in rets]
    routes = (("capped_host_1024", eng, dict(max_pieces=1024)), ("uncapped_twin", NoFinish(eng), dict(max_pieces=None)),
              ("uncapped_device", eng, dict(max_pieces=None)))
    res = {}
    for name, e, kw in routes:
        ts = []
        for _ in range(max(1, a.reps // 2)):
            t0 = time.perf_counter()
            res[name] = level_batch.solution_pieces(net, recs, batches, rets, x, e, want, **kw)
            ts.append(time.perf_counter() - t0)
        print(json.dumps(dict(what="solution_pieces", route=name, nodes=len(fols), recipes_per_node=1024, median_s=float(np.median(ts)),
                              pieces_kept=[len(v) for v in res[name]][:4])), flush=True)
    same = all(len(p) == len(q) and all(np.array_equal(P.local()[1], Q.local()[1]) and np.array_equal(P.l, Q.l) and np.array_equal(P.u, Q.u)
                                        for P, Q in zip(p, q)) for p, q in zip(res["capped_host_1024"], res["uncapped_device"]))
    print(json.dumps(dict(what="solution_pieces_routes_agree", same=bool(same))), flush=True)

    for cap in (64, None):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            r = algorithm.solve(examples.setup("synthetic_pairs", pairs=a.pairs, n=32, m=32, max_pieces=cap), engine=eng)
            dt = time.perf_counter() - t0
        print(json.dumps(dict(what="solve", pairs=a.pairs, n=32, m=32, max_pieces=cap, solved=bool(r["solved"]), seconds=dt,
                              truncated=len(r.get("truncated") or []))), flush=True)


if __name__ == "__main__":
    main()
