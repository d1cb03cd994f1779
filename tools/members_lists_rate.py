"""Both routes of remove_subsets_many's member prefilter (DESIGN.md sections 5e and 5e2) on the same pieces, on one GPU: from
"members on the device" to "refutation known on the host".

  pairs   polyhedra.REFUTE_ROUTE = "pairs": the pairs written out on the host, qpn_members_outside in slices of PAIR_CHUNK, one
          verdict byte per pair down, scattered into k x k matrices
  lists   polyhedra.REFUTE_ROUTE = "lists": a CSR of the lists up, qpn_members_outside_lists, `undecided` down, and the
          segments of `bits` of the pieces that left something undecided

What is timed is polyhedra._refuted_by_members itself, with the interior-member solve taken out (the members, their flags and
the pack are made once and handed to it where polyhedra._interior_member_groups would make them), so both routes do exactly
what they do inside remove_subsets_many.  Seeded pieces of (rows, columns) = (64, 64) around their own members, in lists of
`--k` pieces, `--lists` lists; `--dups` of the pieces are copies of their neighbour (their pairs stay undecided).  The routes
alternate, one warm-up round and `--rounds` measured ones; every time is a host clock around a call that ends in a
synchronise.  The bytes moved each way are computed from the shapes.  Prints one JSON line per measurement and the medians.
usage: python tools/members_lists_rate.py --k 64 --lists 256 | --k 1024 --lists 8 | --k 8192 --lists 1  [--rounds 3] [--dups 0.0]
       [--only pairs|lists]  (one route alone: for a kernel trace)"""
import argparse

import numpy as np

from rate_common import emit, on_device, polyhedra, qpn_amd, timed
from qpn_amd.engine import colmajor


def pieces(B, r, d, dups, seed=0):
    g = np.random.default_rng(seed)
    A = g.standard_normal((B, r, d))
    X = g.standard_normal((B, d))
    s = np.einsum("brd,bd->br", A, X)
    l = s - g.uniform(0.2, 1.0, (B, r)); u = s + g.uniform(0.2, 1.0, (B, r))
    for b in np.nonzero(g.random(B) < dups)[0]:
        if b % 2:                                              # a copy of the piece before it (same list for even list lengths)
            A[b], l[b], u[b], X[b] = A[b - 1], l[b - 1], u[b - 1], X[b - 1]
    return A, l, u, X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--lists", type=int, default=256)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--cols", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dups", type=float, default=0.0)
    ap.add_argument("--only", choices=("pairs", "lists"), default=None)
    a = ap.parse_args()
    import torch
    eng = qpn_amd.default_engine(0)
    k, L, r, d = a.k, a.lists, a.rows, a.cols
    B = k * L
    A, l, u, X = pieces(B, r, d, a.dups)
    Ad, ld, ud, Xd = on_device(eng, (colmajor(A), l, u, X))
    okd = torch.ones(B, dtype=torch.uint8, device=Xd.device)
    group = dict(idx=list(range(B)), x=Xd, ok=okd, Ac=Ad, l=ld, u=ud)
    comp = [[(A[b], l[b], u[b]) for b in range(a0, a0 + k)] for a0 in range(0, B, k)]      # (views: remove_subsets_many's triples)
    starts = {n: n * k for n in range(L)}
    flat = [t for trips in comp for t in trips]
    real = polyhedra._interior_member_groups
    polyhedra._interior_member_groups = lambda trips, engine, *aa, **kw: [group]
    pairs = L * k * (k - 1)
    words = -(-k // 32)
    emit(what="bytes", k=k, lists=L, pieces=B, ordered_pairs=pairs,
         pairs_up=8 * pairs, pairs_down=pairs,
         lists_up=4 * (B + L + 1) + 16 * B + 8, lists_down_always=4 * B, lists_down_per_undecided_piece=4 * words)
    state = {}

    def run(route):
        def fn():
            polyhedra.REFUTE_ROUTE = route
            state[route] = polyhedra._refuted_by_members(comp, flat, starts, eng, 1e-6)
        return fn

    def undecided(ref):
        n = 0
        for m in ref.values():
            if m is not None:
                n += int((~m).sum()) - m.shape[0]
        return n

    try:
        routes = [(name, run(name)) for name in ("pairs", "lists") if a.only in (None, name)]
        for name, fn in routes:                                # warm-up round: module loads, first launches, allocations
            s = timed(fn)
            emit(what="warmup", route=name, seconds=s, k=k, lists=L)
        if a.only is None:
            same = all((state["lists"][n] is None and not (~state["pairs"][n]).sum() - k) or
                       (state["lists"][n] is not None and np.array_equal(state["lists"][n] | np.eye(k, dtype=bool),
                                                                         state["pairs"][n] | np.eye(k, dtype=bool)))
                       for n in range(L))
            emit(what="routes_agree", same=bool(same), undecided_pairs=undecided(state["pairs"]),
                 lists_without_matrix=sum(1 for m in state["lists"].values() if m is None))
        times = {name: [] for name, _ in routes}
        for rnd in range(a.rounds):
            for name, fn in routes:
                eng.calls.clear(); eng.seconds.clear()
                s = timed(fn)
                times[name].append(s)
                emit(what="refute", route=name, round=rnd, seconds=s, k=k, lists=L, pairs_per_s=pairs / s,
                     abi_calls=sum(eng.calls.values()), abi_seconds=sum(eng.seconds.values()))
        emit(what="refute", medians={name: float(np.median(v)) for name, v in times.items()}, k=k, lists=L, rows=r, cols=d, dups=a.dups)
    finally:
        polyhedra.REFUTE_ROUTE = "pairs"
        polyhedra._interior_member_groups = real


if __name__ == "__main__":
    main()
