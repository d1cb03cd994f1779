"""Rates of the subset tests P1 ⊆ P2 on one GPU: the emptiness queries (one node solve per finite bound of
P2 over a padded copy of P1: what an engine without issubset_pairs takes) against qpn_issubset_pairs, one job per pair, through
issubset_batch_chunked (host arrays) and as the bare call over device tensors.

  gauss      `--pairs` pairs of Gaussian pieces of 48 rows in 24 variables, in three parts timed apart: `copies` (P2 = P1 with
             every bound widened: true subsets, every bound one of P1's own rows), `scaled` (the same with P2's rows times two: true
             subsets whose every bound needs its LP; the first `--scaled` of them, the old route builds 96 queries for each) and
             `other` (P2 another Gaussian piece around the same point)
  level      the undecided pairs remove_subsets_many hands to issubset_batch_chunked during one solve() of `--net-pairs` synthetic
             pairs of (32, 32), and `level_all`: every pair of its lists, what it hands over with prefilter=False (the member
             prefilter settles all pairs of this net, so the first set is empty there)

Three rounds, the routes alternating in each; a host clock around a synchronise.  Prints one JSON line per measurement.
usage: python tools/subset_rate.py [--pairs 2000] [--scaled 200] [--net-pairs 250] [--rounds 3] [--skip-gauss] [--level-cap 2000]"""
import argparse
import time

import numpy as np

from rate_common import algorithm, emit, examples, on_device, polyhedra, qpn_amd, quiet_solve, report, without


def measure(what, pairs, eng, rounds):
    import torch
    old = without(eng, "issubset_pairs")                    # (issubset_batch builds its emptiness queries)
    calls, beyond = polyhedra.subset_packs(pairs)
    assert not beyond
    dev = [on_device(eng, args) for _, args in calls]

    def bare():
        outs = [eng.issubset_pairs(*args) for args in dev]
        torch.cuda.synchronize()
        return outs

    routes = (("queries", lambda: polyhedra.issubset_batch_chunked(pairs, old)),
              ("pairs_host", lambda: polyhedra.issubset_batch_chunked(pairs, eng)),
              ("pairs_device", bare))
    answers = {}
    for name, fn in routes:                                 # one untimed pass each
        answers[name] = fn()
    got = np.concatenate([o["sub"].cpu().numpy().astype(bool) for o in answers["pairs_device"]])
    order = np.concatenate([ks for ks, _ in calls])
    assert np.array_equal(answers["pairs_host"][order], got)
    info = dict(pairs=len(pairs), calls=len(calls), subsets=int(answers["pairs_host"].sum()),
                verdicts_differ=int(np.sum(answers["pairs_host"] != answers["queries"])),
                lps=int(sum(int(o["lps"].sum()) for o in answers["pairs_device"])),
                iters=int(sum(int(o["iters"].sum()) for o in answers["pairs_device"])))
    report(what, routes, rounds, medians=False, per=lambda s: dict(pairs_per_s=len(pairs) / s), **info)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2000)
    ap.add_argument("--scaled", type=int, default=200)
    ap.add_argument("--net-pairs", type=int, default=250)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-gauss", action="store_true")
    ap.add_argument("--level-cap", type=int, default=2000, help="at most this many pairs of a level set are timed")
    a = ap.parse_args()
    eng = qpn_amd.default_engine(0)
    emit(what="library", path=qpn_amd._lib.LIB_PATH)

    # (a) Gaussian pieces
    rng = np.random.default_rng(0)
    half = a.pairs // 2
    A = rng.standard_normal((a.pairs, 48, 24))
    x0 = rng.standard_normal((a.pairs, 24))
    s0 = np.einsum("brd,bd->br", A, x0)
    first = [(A[b], s0[b] - np.abs(rng.standard_normal(48)) - 0.05, s0[b] + np.abs(rng.standard_normal(48)) + 0.05) for b in range(a.pairs)]
    copies = [(first[b], (first[b][0], first[b][1] - 0.25, first[b][2] + 0.25)) for b in range(half)]
    scaled = [(P1, (2.0 * P2[0], 2.0 * P2[1], 2.0 * P2[2])) for P1, P2 in copies[:a.scaled]]
    other = []
    for b in range(half, a.pairs):
        A2 = rng.standard_normal((48, 24))
        c = A2 @ x0[b]
        other.append((first[b], (A2, c - np.abs(rng.standard_normal(48)) - 0.05, c + np.abs(rng.standard_normal(48)) + 0.05)))
    for what, pairs in (("gauss_48x24_copies", copies), ("gauss_48x24_scaled", scaled), ("gauss_48x24_other", other)):
        if pairs and not a.skip_gauss:
            measure(what, pairs, eng, a.rounds)

    # (b) the undecided pairs of a level
    seen, lists_seen = [], []
    real = polyhedra.issubset_batch_chunked
    real_many = algorithm.remove_subsets_many

    def recording(lists, engine, *args, **k):
        lists_seen.append([None if polys is None else list(polys) for polys in lists])
        return real_many(lists, engine, *args, **k)

    def capture(pairs, engine, **k):
        seen.extend(pairs)
        return real(pairs, engine, **k)

    polyhedra.issubset_batch_chunked = capture
    algorithm.remove_subsets_many = recording
    try:
        t0 = time.perf_counter()
        r = quiet_solve(examples.setup("synthetic_pairs", pairs=a.net_pairs, n=32, m=32), engine=eng)
        dt = time.perf_counter() - t0
    finally:
        algorithm.remove_subsets_many = real_many
    undecided = list(seen)
    del seen[:]
    try:
        for lists in lists_seen:
            polyhedra.remove_subsets_many(lists, eng, prefilter=False)
    finally:
        polyhedra.issubset_batch_chunked = real
    every = list(seen)[:a.level_cap]
    seen = undecided[:a.level_cap]
    emit(what="solve", pairs=a.net_pairs, n=32, m=32, solved=bool(r["solved"]), seconds=dt, undecided_pairs=len(undecided),
         timed_undecided=len(seen), timed_all_pairs=len(every))
    if seen:
        measure("level_undecided", seen, eng, a.rounds)
    if every:
        measure("level_all", every, eng, a.rounds)


if __name__ == "__main__":
    main()
