"""Intersection trees for the tests of qpn_intersection_trees / polyhedra.intersection_trees_host, shared by the CPU and the GPU tests.

The box family.  Pieces are axis boxes in d = 2 or 3: lower corners on a 0.5 grid, widths 0.4 or 0.9, rows of the identity, every
bound closed.  Along one axis the uppers are = 0.4 (mod 0.5) and the lowers = 0 (mod 0.5), so min(upper) - max(lower) of ANY set of
such intervals is one of ..., -0.6, -0.1, 0.4, 0.9: they overlap by 0.4 at least or leave a gap of 0.1 at least.  The slack LP's
optimum is eps = max over the axes of (max lower - min upper) / 2, so eps <= -0.2 or eps >= 0.05: with tol = 1e-2 every verdict of
every prefix is MEMBER or EMPTY_SLACK with a margin of 0.04 at least, whatever vertex the simplex ends in -- pruning a prefix can
never lose a tuple, and the tree's leaves ARE the non-empty tuples.  A box may drop one axis (d - 1 rows, unbounded there) or state
one bound row twice (d + 1 rows): the candidates of a depth then fall into several row counts n."""
from __future__ import annotations

import itertools

import numpy as np

TOL = 1e-2
MARGIN = 0.04
POINT_TOL = 1e-6
MEMBER, EMPTY_SLACK = 0, 2


def box_piece(g, d, grid):
    """One box: (A [r, d], l, u [r]) with r = d - 1 (one axis dropped), d, or d + 1 (one row twice)."""
    lo = 0.5 * g.integers(0, grid, d)
    hi = lo + np.where(g.integers(0, 2, d) == 1, 0.9, 0.4)
    rows = list(range(d))
    kind = int(g.integers(0, 3))
    if kind == 0 and d > 1:
        rows.pop(int(g.integers(0, d)))
    elif kind == 2:
        rows.append(int(g.integers(0, d)))
    A = np.eye(d)[rows]
    return A, lo[rows], hi[rows]


def box_trees(seed, d, L, widths, grid=3, red=None):
    """`len(widths)` trees of depth L over one pool of boxes: tree g's list t has widths[g][t] boxes of its own (every piece is
    named once), the pool's pieces shuffled.  red: per tree and list the trailing complement members (None: none).
    -> dict(pool = (A, l, u, open_lo, open_hi), piece_row, L, list_ptr, list_mem, list_red, trees)."""
    g = np.random.default_rng([seed, d, L, 20])
    total = int(sum(sum(w) for w in widths))
    boxes = [box_piece(g, d, grid) for _ in range(total)]
    order = g.permutation(total)                               # pool piece p = box order[p]
    where = np.empty(total, np.int64); where[order] = np.arange(total)
    A = np.vstack([boxes[b][0] for b in order]); l = np.concatenate([boxes[b][1] for b in order]); u = np.concatenate([boxes[b][2] for b in order])
    piece_row = np.concatenate([[0], np.cumsum([len(boxes[b][1]) for b in order])]).astype(np.int32)
    flat = [w for ws in widths for w in ws]
    list_ptr = np.concatenate([[0], np.cumsum(flat)]).astype(np.int32)
    list_mem = where[np.arange(total)].astype(np.int32)
    list_red = np.zeros(len(flat), np.int32) if red is None else np.asarray(red, np.int32).reshape(-1)
    zero = np.zeros(len(l), np.uint8)
    return dict(pool=(A, l, u, zero, zero.copy()), piece_row=piece_row, L=L, list_ptr=list_ptr, list_mem=list_mem, list_red=list_red,
                trees=len(widths))


def boxes_of(boxes, lists, red=None):
    """One tree over boxes given as (lower corner, upper corner) pairs: `lists` name them by number, every box is one pool piece
    of d rows.  -> the dict of box_trees."""
    d = len(boxes[0][0])
    A = np.vstack([np.eye(d) for _ in boxes])
    l = np.concatenate([np.asarray(b[0], float) for b in boxes]); u = np.concatenate([np.asarray(b[1], float) for b in boxes])
    zero = np.zeros(len(l), np.uint8)
    return dict(pool=(A, l, u, zero, zero.copy()), piece_row=(d * np.arange(len(boxes) + 1)).astype(np.int32), L=len(lists),
                list_ptr=np.concatenate([[0], np.cumsum([len(m) for m in lists])]).astype(np.int32),
                list_mem=np.array([b for mem in lists for b in mem], np.int32),
                list_red=np.zeros(len(lists), np.int32) if red is None else np.asarray(red, np.int32), trees=1)


def args_of(c):
    """The positional arguments of intersection_trees_host / Engine.intersection_trees up to list_red."""
    return (*c["pool"], c["piece_row"], c["L"], c["list_ptr"], c["list_mem"], c["list_red"])


def tree_lists(c, g):
    """Tree g's lists: [[(pool piece, is a complement piece)]]."""
    L = c["L"]
    out = []
    for t in range(L):
        p0, p1 = int(c["list_ptr"][g * L + t]), int(c["list_ptr"][g * L + t + 1])
        out.append([(int(c["list_mem"][j]), j >= p1 - int(c["list_red"][g * L + t])) for j in range(p0, p1)])
    return out


def all_tuples(c, g):
    """Every tuple of tree g that is not made of complement pieces alone, in lexicographic order of list positions."""
    return [tuple(f for f, _ in ch) for ch in itertools.product(*tree_lists(c, g)) if not all(comp for _, comp in ch)]


def rows_of(c, tup):
    return int(sum(c["piece_row"][f + 1] - c["piece_row"][f] for f in tup))


def overlapping_boxes(count, d=2):
    """`count` boxes of the family that all contain the cube [0.5, 0.9]^d: per axis [0, 0.9] or [0.5, 0.9] or [0.5, 1.4]."""
    sides = ((0.0, 0.9), (0.5, 0.9), (0.5, 1.4))
    out = []
    for i in range(count):
        pick = [sides[(i // 3 ** k) % 3] for k in range(d)]
        out.append((tuple(p[0] for p in pick), tuple(p[1] for p in pick)))
    return out
