"""Shared inputs of tests/test_parent_records_host.py and tests/test_gpu_parent_records.py: seeded small nets
whose parents' records cover the shapes qpn_assemble_parent_nodes can go wrong at, the engine double the twin serves, the edits
that make an item bad, and a two-level net caught at a kink (two pieces for one child)."""
import collections
import functools

import numpy as np

import qpn_amd  # noqa: F401
from qpn_amd import algorithm, examples, level_batch
from qpn_amd.programs import Poly, QPNet

from oracle_engine import OracleEngine

INF = np.inf


class TwinEngine(OracleEngine):
    """The oracle engine plus assemble_parent_nodes served by the numpy twin; `n` counts the calls, `args` keeps them."""

    def __init__(self):
        super().__init__()
        self.n = collections.Counter()
        self.args = []

    def assemble_parent_nodes(self, *a):
        self.n["assemble_parent_nodes"] += 1
        self.args.append(a)
        return level_batch.assemble_parent_records_host(*a)


# a family: (n0, base rows, children, parameters the parent reads, [choice, ...]); a choice: one piece spec per child;
# a piece spec: (rows, "eq" | "ineq" | "mix", "local" | "dense")
CASES = [
    ("n2_base0_one_child", [(2, 0, 1, 2, [[(1, "ineq", "local")], [(5, "mix", "local")], [(0, "ineq", "local")], [(5, "eq", "local")],
                                          [(1, "eq", "dense")], [(16, "ineq", "local")], [(17, "mix", "local")]])]),
    ("n4_base3_two_children", [(4, 3, 2, 2, [[(5, "mix", "local"), (8, "ineq", "local")], [(5, "mix", "local"), (9, "ineq", "local")],
                                             [(1, "eq", "local"), (1, "ineq", "local")], [(5, "mix", "dense"), (8, "ineq", "local")],
                                             [(0, "eq", "local"), (5, "eq", "dense")]])]),
    ("three_parents_p_and_base_padded", [(4, 3, 1, 2, [[(5, "mix", "local")], [(1, "ineq", "local")]]),
                                         (4, 3, 1, 1, [[(5, "mix", "local")], [(1, "ineq", "dense")]]),
                                         (4, 0, 1, 2, [[(5, "mix", "local")], [(13, "ineq", "local")], [(14, "mix", "local")]])]),
]


def _bounds(g, rows, kind):
    l = np.round(g.standard_normal(rows), 3); u = l.copy()
    for i in range(rows):
        if kind == "ineq" or (kind == "mix" and i % 2 == 1):
            u[i] = l[i] + 1.0 + i
            if i % 3 == 0:
                l[i] = -INF
            elif i % 3 == 1:
                u[i] = INF
    if kind == "ineq" and rows >= 5:
        l[4], u[4] = -INF, INF
    return l, u


def _piece(g, nv, reads, spec):
    rows, kind, form = spec
    cols = np.sort(g.choice(reads, size=max(2, min(len(reads), 1 + int(g.integers(len(reads))))), replace=False)).astype(np.int64)
    A = g.standard_normal((rows, cols.size))
    if rows:
        A[0, -1] = -0.0
        A[-1, 0] = 0.0 if cols.size > 1 else A[-1, 0]
    l, u = _bounds(g, rows, kind)
    if form == "dense":
        Ad = np.zeros((rows, nv)); Ad[:, cols] = A
        return Poly(Ad, l, u)
    return Poly.from_sorted(nv, cols, A, l, u, normalise=False)


def build(case):
    """The net of a case and its items [(pid, [child Poly, ...])], one per choice of every family."""
    name, families = case
    g = np.random.default_rng(sum(map(ord, name)))
    nv = sum(n0 + 3 for n0, *_ in families) + 1                   # the last variable is read by nobody
    net = QPNet(nv)
    o, edges, plans = 0, [], []
    for n0, nbase, nchild, npar, choices in families:
        dec = list(range(o, o + n0)); par = list(range(o + n0, o + n0 + npar))
        own = dec[:n0 - nchild * (n0 // 2 // nchild)]
        kids = np.array_split(np.array(dec[len(own):]), nchild)
        idx = dec + par
        G = g.standard_normal((len(idx), len(idx)))
        Q = G.T @ G + np.eye(len(idx))
        cons = []
        if nbase:
            A = g.standard_normal((nbase, len(idx))); l = np.array([-INF, 0.5, -1.0])[:nbase]; u = np.array([1.0, 0.5, INF])[:nbase]
            cons.append(net.add_constraint(A, l, u, cols=idx))
        pid = net.add_qp(Q, g.standard_normal(len(idx)), cons, own, idx=idx)
        for kv in kids:
            cid = net.add_qp(np.eye(len(idx)), np.zeros(len(idx)), [], [int(v) for v in kv], idx=idx)
            edges.append((pid, cid))
        plans.append((pid, np.array(idx), choices))
        o += n0 + 3
    net.add_edges(edges)
    net.assign_constraint_groups()
    items = []
    for pid, reads, choices in plans:
        assert np.array_equal(level_batch._static(net, pid)["reads"], reads)
        for choice in choices:
            items.append((pid, [_piece(g, nv, reads, spec) for spec in choice]))
    return net, items


def bad_edits(base):
    """[(name, edit, err)]: edit(args) makes item 0 of a form-1 call bad in one way and leaves every other item as it is.  Item 0
    has two pieces, the second without equalities and of more rows than the padding leaves free."""
    pieces, maps = len(base[12]), len(base[16]) - 1
    q0, m0 = int(base[19][0, 0]), int(base[20][0, 0])
    c = int(base[12][q0][2]); r = int(base[12][q0][1])
    mo = int(base[16][m0])
    old = np.array(base[17][mo:mo + c])
    A0 = np.asarray(base[13])[int(base[12][q0][3]):][:r * c].reshape(r, c)
    assert c >= 2 and r >= 1

    def with_map(new):
        def edit(a):
            a[16] = np.append(a[16], a[16][-1] + len(new)).astype(np.int32)
            a[17] = np.append(a[17], new).astype(np.int32)
            a[20][0, 0] = maps
            return a
        return edit

    def setter(k, at, v):
        def edit(a):
            a[k][at] = v
            return a
        return edit

    def more_rows(a):
        a[19][0, 2], a[20][0, 2] = a[19][0, 1], a[20][0, 1]
        return a
    n0, p = base[6].shape[1], base[3]
    hit = int(np.nonzero((A0 != 0).any(axis=0))[0][0])
    out_of_range = old.copy(); out_of_range[0] = n0 + p
    below = old.copy(); below[0] = -2
    twice = old.copy(); twice[1] = twice[0]
    unread = old.copy(); unread[hit] = -1
    return [("parent index", setter(18, 0, len(base[6])), level_batch.PR_BAD_INDEX),
            ("parent index negative", setter(18, 0, -1), level_batch.PR_BAD_INDEX),
            ("piece index", setter(19, (0, 0), pieces), level_batch.PR_BAD_INDEX),
            ("piece index negative", setter(19, (0, 1), -2), level_batch.PR_BAD_INDEX),
            ("map index", setter(20, (0, 1), maps), level_batch.PR_BAD_INDEX),
            ("piece range", setter(12, (q0, 1), len(base[14]) + 1), level_batch.PR_BAD_INDEX),
            ("map entry above", with_map(out_of_range), level_batch.PR_BAD_MAP),
            ("map entry below", with_map(below), level_batch.PR_BAD_MAP),
            ("map names a column twice", with_map(twice), level_batch.PR_BAD_MAP),
            ("map length", with_map(np.append(old, -1)), level_batch.PR_BAD_MAP),
            ("unread column", with_map(unread), level_batch.PR_BAD_COLUMN),
            ("rows", more_rows, level_batch.PR_BAD_ROWS),
            ("equality count", setter(19, (0, 0), -1), level_batch.PR_BAD_EQ)]


def biggest_call(eng):
    return max(eng.args, key=lambda a: len(a[18]))


@functools.lru_cache(maxsize=None)
def _kink():
    """A sweep of solve() on a small net of leader-follower pairs at which some follower's solution graph has two pieces."""
    real = level_batch.verify_items
    for pairs, n, m in ((6, 3, 3), (5, 4, 6), (8, 3, 2), (12, 3, 3)):
        net = examples.setup("synthetic_pairs", pairs=pairs, n=n, m=m)
        found = []

        def spy(qpn, items, x, *a, **k):
            if not found and len({pid for pid, _ in items}) < len(items) and all(ch for _, ch in items):
                found.append((np.array(x, dtype=np.float64), [(pid, list(ch)) for pid, ch in items]))
            return real(qpn, items, x, *a, **k)
        level_batch.verify_items = spy
        try:
            algorithm.solve(net, engine=OracleEngine())
        finally:
            level_batch.verify_items = real
        if found:
            return (pairs, n, m), found[0]
    raise AssertionError("no kink met")


def kinked_pairs():
    """(net, x, S): a fresh net of leader-follower pairs, the point of a sweep and the followers' solution graphs there, one of
    them with two pieces."""
    (pairs, n, m), (x, items) = _kink()
    net = examples.setup("synthetic_pairs", pairs=pairs, n=n, m=m)
    S = {}
    for pid, ch in items:
        (j,) = sorted(net.network_edges[pid])
        if not any(P is ch[0] for P in S.setdefault(j, [])):
            S[j].append(ch[0])
    return net, x.copy(), S


def random_call(seed, form, items, parents, n0, mb, ps, p, pieces, rows, eqs, c, slots, base_eq=True):
    """The arguments of one assemble_parent_nodes call made directly (no net): `parents` parents with 1 .. mb base rows (all mb
    when parents == 1), the first of them an equality (base_eq); `pieces` pieces of `rows` rows, the first `eqs` of them (after a
    shuffle) equalities, over c columns; a map per (parent, piece) with a -1 entry under a zero column now and then; every item
    takes `slots` pieces.  Every item has base_eq + slots * eqs equality rows; m is padded to 16 for the tallest item."""
    g = np.random.default_rng(seed)
    sQc = g.standard_normal((parents, n0, n0)); sRc = g.standard_normal((parents, ps, n0)); sqd = g.standard_normal((parents, n0))
    mbt = np.array([mb if parents == 1 else 1 + (k * 5) % mb for k in range(parents)], np.int32)
    sAc = g.standard_normal((parents, n0, mb)); sBc = g.standard_normal((parents, ps, mb))
    sl = np.round(g.standard_normal((parents, mb)), 2); su = sl + 1.0
    sl[:, 1::3] = -INF; su[:, 2::3] = INF
    if base_eq:
        su[:, 0] = sl[:, 0]                                       # the first base row: an equality
    for k in range(parents):                                      # beyond a parent's own rows: padding nobody may read as data
        sAc[k, :, mbt[k]:] = np.nan; sBc[k, :, mbt[k]:] = np.nan; sl[k, mbt[k]:] = np.nan; su[k, mbt[k]:] = np.nan
    desc = np.zeros((pieces, 4), np.int32); pA, pl, pu = [], [], []
    for q in range(pieces):
        A = g.standard_normal((rows, c)); A[g.uniform(size=A.shape) < 0.2] = 0.0; A[0, 0] = -0.0
        if q % 2:
            A[:, c - 1] = 0.0
        l = np.round(g.standard_normal(rows), 2); u = l + 0.5
        l[1::4] = -INF; u[3::4] = INF
        E = g.permutation(rows)[:eqs]
        l[E] = np.where(np.isfinite(l[E]), l[E], 0.25); u[E] = l[E]
        desc[q] = (q * rows, rows, c, q * rows * c)
        pA.append(A.ravel()); pl.append(l); pu.append(u)
    moff = [0]; mdat = []
    for k in range(parents * pieces):
        mv = g.permutation(n0 + p)[:c].astype(np.int32)
        if (k % pieces) % 2 and k % 3 == 0:
            mv[c - 1] = -1                                        # (that piece's last column is all zeros)
        mdat.append(mv); moff.append(moff[-1] + c)
    parent_of = g.integers(parents, size=items).astype(np.int32)
    piece_of = np.full((items, 8), -1, np.int32); map_of = np.zeros((items, 8), np.int32)
    for b in range(items):
        at = np.sort(g.permutation(8)[:slots])
        qs = g.integers(pieces, size=slots)
        piece_of[b, at] = qs; map_of[b, at] = parent_of[b] * pieces + qs
    ne = int(base_eq) + slots * eqs if form else 0
    tall = int(mbt.max()) + slots * rows - ne
    m = max(16, -(-tall // 16) * 16) if tall else 0
    return (form, ne, m, p, sQc, sRc, sqd, sAc, sBc, sl, su, mbt, desc, np.concatenate(pA), np.concatenate(pl), np.concatenate(pu),
            np.array(moff, np.int32), np.concatenate(mdat).astype(np.int32), parent_of, piece_of, map_of)
