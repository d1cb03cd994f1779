"""Products of pieces for the tests of qpn_exemplar_products / polyhedra.exemplar_products_host, shared by the CPU and the GPU tests:
the planted polyhedra of tests/exemplar_cases.py cut into runs of rows, so that the answer for a product is the answer for the whole
polyhedron, which is known by construction; and points for the closure test whose verdict is known with a margin."""
from __future__ import annotations

import numpy as np

import exemplar_cases

KS = (1, 2, 3, 5)
SLOTS = 7
POINT_TOL = 1e-6
MARGIN = 1e-3                                    # no row value of a planted point lies nearer to a bound than this


def cut_batch(shape, count, first=0, ks=KS, slots=SLOTS):
    """`count` polyhedra of exemplar_cases.family_batch(shape, count, first), each cut at seeded random places into k runs of rows (k
    from `ks` in turn; a cut may repeat: an empty run; every third polyhedron with k >= 2 starts with one).  The pieces of all of them
    lie in ONE pool in a shuffled order, and product t names its k pieces in `slots` slots at seeded ascending places, -1 elsewhere.
    -> dict(pool = (A [rows, d], l, u, open_lo, open_hi [rows]), piece_row [pieces + 1] int32, factors [count, slots] int32, n,
    whole = (A [count, n, d], l, u, open_lo, open_hi), empty [count] bool, how [count])."""
    n, d = shape
    A, l, u, ol, oh, empty, how = exemplar_cases.family_batch(shape, count, first=first)
    g = np.random.default_rng([n, d, count, first, 77])
    runs = []                                                   # (polyhedron, first row, last row + 1) in product order
    of = []
    for t in range(count):
        k = ks[t % len(ks)]
        cuts = np.sort(g.integers(0, n + 1, k - 1))
        if k >= 2 and t % 3 == 0:
            cuts[0] = 0
        edges = np.concatenate([[0], cuts, [n]])
        of.append(list(range(len(runs), len(runs) + k)))
        runs += [(t, int(edges[i]), int(edges[i + 1])) for i in range(k)]
    order = g.permutation(len(runs))                            # pool piece p = run order[p]
    where = np.empty(len(runs), np.int64); where[order] = np.arange(len(runs))
    take = lambda M: np.concatenate([M[runs[r][0], runs[r][1]:runs[r][2]] for r in order])
    piece_row = np.concatenate([[0], np.cumsum([runs[r][2] - runs[r][1] for r in order])]).astype(np.int32)
    factors = np.full((count, slots), -1, np.int32)
    for t in range(count):
        places = np.sort(g.choice(slots, len(of[t]), replace=False))
        factors[t, places] = where[of[t]]
    return dict(pool=(take(A), take(l), take(u), take(ol), take(oh)), piece_row=piece_row, factors=factors, n=n, whole=(A, l, u, ol, oh),
                empty=empty, how=how)


def plant_x0(seed, n, d, kind):
    """The point exemplar_cases.planted(seed, n, d, kind) built its rows around (its generator's first draw)."""
    return np.random.default_rng([seed, n, d, exemplar_cases.KINDS.index(kind)]).standard_normal(d)


def closure_points(A, l, u, x0):
    """A point of the `fat` polyhedron (A, l, u) around x0 that lies 0.01 beyond ONE bound and inside every other row, every row value
    at least MARGIN away from its bounds: x0 moved along that row.  -> (point, 2 i + side), the first row and side that allows it."""
    s0 = A @ x0
    for i in range(A.shape[0]):
        for side, bound in ((0, l[i] - 0.01), (1, u[i] + 0.01)):
            if not np.isfinite(bound):
                continue
            p = x0 + A[i] * ((bound - s0[i]) / (A[i] @ A[i]))
            s = A @ p
            out = (s < l - MARGIN) | (s > u + MARGIN)
            clear = (np.abs(s - l) >= MARGIN) & (np.abs(s - u) >= MARGIN)
            if clear.all() and out[i] and out.sum() == 1:
                return p, 2 * i + side
    raise AssertionError("no row of this polyhedron can be left alone")
