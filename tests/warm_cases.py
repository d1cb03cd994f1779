"""Planted nodes and hints for the warm start of the n, m <= 32 node solve (QPN_AVI_FLAG_WARM_DUALS): shared by
tests/test_warm_nodes_host.py (the numpy twin) and tests/test_gpu_warm_nodes.py (the kernel).  The nodes are
solve_cases.make_node's, one parameter vector per shape (a batch shares it); a hint is a z whose multipliers carry the sides
(the primal part is noise: nobody reads it).

The weak family needs two inactive rows that are linearly independent of the active ones: like solve_cases.cell_families it is
left out where min(n, m) < 3.
"""
from __future__ import annotations

import numpy as np

import solve_cases as SC

SHAPES = [(32, 32), (5, 7), (1, 32), (32, 1), (17, 32)]
FAMILIES = ("k40", "k1e4", "axis", "skew", "nearsym", "weak", "k0", "kfull", "rowscale")
WRONG = ("dropped", "added", "swapped", "empty", "too_many", "infinite", "nan")
P = 3
PER = 2                                                  # nodes per family and shape

_CACHE = {}


def families(n, m):
    return tuple(f for f in FAMILIES if not (f == "weak" and min(n, m) < 3))


def shape_nodes(n, m, seed=23):
    """The planted nodes of one shape, every family PER times, one w for all (built once per process, left unchanged)."""
    if (n, m, seed) not in _CACHE:
        rng = np.random.default_rng([seed, n, m])
        w = rng.standard_normal(P)
        _CACHE[n, m, seed] = [SC.make_node(rng, n, m, f, P, w) for f in families(n, m) for _ in range(PER)]
    return _CACHE[n, m, seed]


def hint_from_side(node, side, rng):
    """z with noise in the primal part and multipliers of the given sides, |lambda| in [0.5, 1.5]."""
    n = node["rec"][0].shape[0]
    side = np.asarray(side, dtype=np.float64)
    return np.concatenate([rng.standard_normal(n), side * rng.uniform(0.5, 1.5, side.size)])


def true_hint(node, rng):
    return hint_from_side(node, node["side"], rng)


def wrong_hint(node, kind, rng):
    """A hint that is wrong in one way, or None where the node has no such hint."""
    Q, R, qd, A, B, l, u = node["rec"]
    n, m = Q.shape[0], A.shape[0]
    side = node["side"].astype(np.int64).copy()
    act = np.flatnonzero(side)
    free = np.flatnonzero((side == 0) & ~node["weak"])
    if kind == "dropped":
        if not act.size:
            return None
        side[rng.choice(act)] = 0
    elif kind == "added":
        cand = [(i, s) for i in free for s, bnd in ((1, l[i]), (-1, u[i])) if np.isfinite(bnd)]
        if not cand:
            return None
        i, s = cand[rng.integers(len(cand))]
        side[i] = s
    elif kind == "swapped":
        if not act.size:
            return None
        side[rng.choice(act)] *= -1
    elif kind == "empty":
        if not act.size:
            return None
        side[:] = 0
    elif kind == "too_many":                              # k > n: the true rows and inactive ones up to n + 1
        if act.size + free.size < n + 1:
            return None
        for i in free[:n + 1 - act.size]:
            side[i] = 1 if np.isfinite(l[i]) else -1
    elif kind == "infinite":
        cand = [(i, s) for i in free for s, bnd in ((1, l[i]), (-1, u[i])) if not np.isfinite(bnd)]
        if not cand:
            return None
        i, s = cand[rng.integers(len(cand))]
        side[i] = s
    z = hint_from_side(node, side, rng)
    if kind == "nan":
        z[n + rng.integers(m)] = np.nan
    return z


def random_hint(node, rng):
    """Each row's side drawn independently: its true side with probability 1/2, else one of the three at random (a hint with
    every side uniform would never be right beyond a few rows)."""
    side = node["side"].astype(np.int64)
    draw = rng.integers(-1, 2, side.size)
    return hint_from_side(node, np.where(rng.random(side.size) < 0.5, side, draw), rng)


def sides_of(z, n):
    return np.sign(np.asarray(z)[n:]).astype(np.int8)
