"""polyhedra_host.intersection_trees_host, the numpy twin of qpn_intersection_trees, and the host functions
that use the entry, without a GPU: the breadth-first twin against a depth-first recursion written here after get_next!
(src/intersection.jl:66-105) on the box family of tests/tree_cases.py; the subset law against exemplar_products_host over all tuples
and, on the box family, equality with them; a planted prunable tree with hand-counted tests; the redzone; the limits in both modes;
intersection_trees and combine_at with route="tree" on a spy engine served by the twins."""
from __future__ import annotations

import os

import numpy as np
import pytest

import goldenio as G
import qpn_amd  # noqa: F401
import tree_cases as TC
from qpn_amd import algorithm, examples, polyhedra, qp_processing
from qpn_amd.programs import Poly
from test_exemplar_products_host import Spy as ProductsSpy, _kink, _same_pieces
from tree_cases import TOL

INF = np.inf
BOX_CASES = [(2, 2, 0), (3, 2, 1), (2, 3, 2), (3, 3, 0), (2, 5, 3), (3, 5, 4)]       # (d, L, seed): both verdicts at every depth >= 2


class Spy(ProductsSpy):
    """The spy of the products tests plus intersection_trees, served by its twin and logged like the others."""

    def intersection_trees(self, A, l, u, open_lo, open_hi, piece_row, L, list_ptr, list_mem, list_red, cap, point=None, point_of=None,
                           point_tol=1e-6, tol=1e-2, slack_cap=1.0, opts=None):
        assert all(a.dtype == np.int32 for a in (piece_row, list_ptr, list_mem, list_red)) and (point_of is None or point_of.dtype == np.int32)
        self._note("intersection_trees", A, l, u, open_lo, open_hi, piece_row, list_ptr, list_mem, list_red, point, point_of)
        out = polyhedra.intersection_trees_host(A, l, u, open_lo, open_hi, piece_row, L, list_ptr, list_mem, list_red, cap, point=point,
                                                point_of=point_of, point_tol=point_tol, tol=tol, slack_cap=slack_cap, opts=opts)
        self.tested = getattr(self, "tested", 0) + int(out["tested"].sum())
        return {k: (np.array([v]) if np.isscalar(v) or isinstance(v, int) else v) for k, v in out.items()}


def box_case(d, L, seed, trees=6):
    g = np.random.default_rng([seed, L])
    widths = [[int(g.integers(1, 5)) for _ in range(L)] for _ in range(trees)]
    return TC.box_trees(seed, d, L, widths)


def one_verdict(c, tup, **kw):
    """exemplar_products_host on ONE tuple -> (empty, how, eps)."""
    L = c["L"]
    fac = np.full((1, L), -1, np.int64); fac[0, :len(tup)] = tup
    got = polyhedra.exemplar_products_host(*c["pool"], c["piece_row"], fac, TC.rows_of(c, tup), tol=TOL, **kw)
    return bool(got["empty"][0]), int(got["how"][0]), float(got["eps"][0])


def depth_first(c, near=None):
    """get_next! (src/intersection.jl:66-105) as a recursion: per tree, a member is appended, the prefix tested, and the subtree
    under an empty prefix never entered.  near: per tree and list the members that stay (None: all).
    -> (leaves [(tree, tuple)], tested [L], alive [L])."""
    L = c["L"]
    tested, alive, leaves = [0] * L, [0] * L, []

    def walk(g, lists, t, tup, allc):
        for f, comp in lists[t]:
            if t == L - 1 and allc and comp:
                continue
            tested[t] += 1
            if one_verdict(c, tup + (f,))[0]:
                continue
            alive[t] += 1
            if t == L - 1:
                leaves.append((g, tup + (f,)))
            else:
                walk(g, lists, t + 1, tup + (f,), allc and comp)

    for g in range(c["trees"]):
        lists = TC.tree_lists(c, g)
        if near is not None:
            lists = [[m for m in mem if m[0] in near[g][t]] for t, mem in enumerate(lists)]
        walk(g, lists, 0, (), True)
    return leaves, tested, alive


def leaves_of(out):
    return [(int(g), tuple(int(f) for f in row)) for g, row in zip(out["leaf_tree"], out["leaves"])]


# ---- the twin ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,L,seed", BOX_CASES)
def test_the_twin_equals_the_depth_first_walk_and_all_tuples_on_boxes(d, L, seed):
    c = box_case(d, L, seed)
    out = polyhedra.intersection_trees_host(*TC.args_of(c), 4096, tol=TOL)
    leaves, tested, alive = depth_first(c)
    assert leaves_of(out) == leaves and out["tested"].tolist() == tested and out["alive"].tolist() == alive
    assert out["n_leaves"] == len(leaves) and out["overflow"] == 0 and not out["unanswered"].any()
    assert out["tree_leaves"].tolist() == [sum(1 for g, _ in leaves if g == k) for k in range(c["trees"])]
    assert out["leaves"].dtype == np.int32 and out["tested"].dtype == np.int64 and out["leaf_how"].dtype == np.int32
    # both verdicts at every depth a box can be empty at (one box alone never is)
    assert out["alive"][0] == out["tested"][0] and all(0 < a < t for a, t in zip(out["alive"][1:], out["tested"][1:]))
    # the subset law, and on this family equality: the margin makes it a condition
    survivors, margin = [], INF
    for g in range(c["trees"]):
        for tup in TC.all_tuples(c, g):
            empty, how, eps = one_verdict(c, tup)
            assert how in (TC.MEMBER, TC.EMPTY_SLACK)
            margin = min(margin, abs(eps - TOL), abs(eps + TOL))
            if not empty:
                survivors.append((g, tup))
    assert margin >= TC.MARGIN - 1e-9
    assert set(leaves) <= set(survivors) and leaves == survivors
    # every leaf's verdict is the job of the same rows in the same order
    assert out["leaf_how"].tolist() == [one_verdict(c, tup)[1] for _, tup in leaves]
    # a depth holds several row counts
    ns = {TC.rows_of(c, (int(a), int(b))) for g in range(c["trees"]) for a, _ in TC.tree_lists(c, g)[0] for b, _ in TC.tree_lists(c, g)[1]}
    assert len(ns) >= 3


def planted():
    """List 1: two disjoint boxes; list 2: three boxes that meet the first of them only; list 3: four boxes, all over the first."""
    boxes = [((0.0, 0.0), (0.4, 0.4)), ((1.0, 1.0), (1.4, 1.4)),
             ((0.0, 0.0), (0.9, 0.9)), ((0.0, 0.0), (0.4, 0.9)), ((0.0, 0.0), (0.9, 0.4)),
             ((0.0, 0.0), (0.4, 0.4)), ((0.0, 0.0), (0.9, 0.4)), ((0.0, 0.0), (0.4, 0.9)), ((0.0, 0.0), (0.9, 0.9))]
    return TC.boxes_of(boxes, [[0, 1], [2, 3, 4], [5, 6, 7, 8]])


def test_a_planted_prunable_tree_tests_fewer_prefixes_than_it_has_tuples():
    c = planted()
    out = polyhedra.intersection_trees_host(*TC.args_of(c), 64, tol=TOL)
    # depth 1: 2 boxes, both kept; depth 2: 2 x 3, the three under box 0 kept; depth 3: 3 x 4, all kept
    assert out["tested"].tolist() == [2, 6, 12] and out["alive"].tolist() == [2, 3, 12]
    assert int(out["tested"].sum()) == 20 < 2 * 3 * 4
    assert leaves_of(out) == [(0, (0, b, e)) for b in (2, 3, 4) for e in (5, 6, 7, 8)]
    assert leaves_of(out) == [(0, t) for t in TC.all_tuples(c, 0) if not one_verdict(c, t)[0]]


def redzone_case():
    """Tree 0: S0 | C1 and S2 | C3 with only C1, C3 meeting: its one non-empty tuple is made of complement pieces.  Tree 1: C4 alone
    then S5, which meet: a prefix of complement pieces with a solution piece in the last slot."""
    boxes = [((0.0, 0.0), (0.4, 0.4)), ((1.0, 1.0), (1.9, 1.9)), ((2.0, 2.0), (2.4, 2.4)), ((1.5, 1.5), (2.4, 1.9)),
             ((0.0, 0.0), (0.9, 0.9)), ((0.5, 0.5), (0.9, 0.9))]
    a = TC.boxes_of(boxes, [[0, 1], [2, 3]], red=[1, 1])
    a["list_ptr"] = np.array([0, 2, 4, 5, 6], np.int32); a["list_mem"] = np.array([0, 1, 2, 3, 4, 5], np.int32)
    a["list_red"] = np.array([1, 1, 1, 0], np.int32); a["trees"] = 2
    return a


def test_the_redzone_and_the_near_test():
    c = redzone_case()
    out = polyhedra.intersection_trees_host(*TC.args_of(c), 64, tol=TOL)
    assert [one_verdict(c, t)[0] for t in ((0, 2), (0, 3), (1, 2), (1, 3))] == [True, True, True, False]
    assert out["tree_leaves"].tolist() == [0, 1] and leaves_of(out) == [(1, (4, 5))]
    # depth 2 forms (0, 2), (0, 3), (1, 2) but not (1, 3); tree 1 forms (4, 5)
    assert out["tested"].tolist() == [3, 4] and out["alive"].tolist() == [3, 1]
    assert leaves_of(out) == depth_first(c)[0]
    # with tree 0's redzone taken away its tuple of the two last pieces is a leaf: the redzone alone kept it out
    free = dict(c, list_red=np.array([0, 0, 1, 0], np.int32))
    assert leaves_of(polyhedra.intersection_trees_host(*TC.args_of(free), 64, tol=TOL)) == [(0, (1, 3)), (1, (4, 5))]
    # a member that is not near leaves its list, the rest keeps its order: the point (0.7, 0.7) lies in boxes 1 and 2 of list 1
    boxes = [((0.0, 0.0), (0.4, 0.9)), ((0.0, 0.0), (0.9, 0.9)), ((0.5, 0.5), (0.9, 0.9)), ((0.5, 0.5), (1.4, 1.4)), ((0.0, 0.5), (0.4, 0.9))]
    c = TC.boxes_of(boxes, [[0, 1, 2], [3, 4]])
    kw = dict(point=np.array([[9.0, 9.0], [0.7, 0.7]]), point_of=np.array([1]), point_tol=TC.POINT_TOL, tol=TOL)
    out = polyhedra.intersection_trees_host(*TC.args_of(c), 64, **kw)
    assert out["tested"].tolist() == [2, 2] and leaves_of(out) == [(0, (1, 3)), (0, (2, 3))]
    assert leaves_of(out) == depth_first(c, near=[[{1, 2}, {3}]])[0]
    # ... which is the per-product closure test: the tuples exemplar_products_host calls near and not empty
    fac = np.array(TC.all_tuples(c, 0))
    per = polyhedra.exemplar_products_host(*c["pool"], c["piece_row"], fac, 4, point=kw["point"], point_of=np.ones(len(fac), np.int64),
                                           point_tol=TC.POINT_TOL, tol=TOL)
    assert [tuple(f) for f, nr, em in zip(fac.tolist(), per["near"], per["empty"]) if nr and not em] == [(1, 3), (2, 3)]
    # without a point every member is near: box 0 meets box 4
    assert leaves_of(polyhedra.intersection_trees_host(*TC.args_of(c), 64, tol=TOL)) == [(0, (0, 4)), (0, (1, 3)), (0, (1, 4)), (0, (2, 3))]


def long_case(second):
    """Two lists of one piece each: 255 rows and `second` rows, all copies of the rows of the box [0, 0.9]^2."""
    rows = 255 + second
    A = np.eye(2)[np.arange(rows) % 2]
    zero = np.zeros(rows, np.uint8)
    return dict(pool=(A, np.zeros(rows), np.full(rows, 0.9), zero, zero.copy()), piece_row=np.array([0, 255, rows], np.int32), L=2,
                list_ptr=np.array([0, 1, 2], np.int32), list_mem=np.array([0, 1], np.int32), list_red=np.zeros(2, np.int32), trees=1)


def test_the_limits_in_both_modes():
    twin = polyhedra.intersection_trees_host
    # cap: the planted tree forms 6 candidates at depth 2 of 3
    c = planted()
    out = twin(*TC.args_of(c), 5, tol=TOL)
    assert out["overflow"] == 2 and out["n_leaves"] == 0 and out["tested"].tolist() == [2, 6, 0] and out["alive"].tolist() == [2, 0, 0]
    assert out["tree_leaves"].tolist() == [0] and out["leaves"].shape == (0, 3)
    assert twin(*TC.args_of(c), 12, tol=TOL)["overflow"] == 0 and twin(*TC.args_of(c), 11, tol=TOL)["overflow"] == 3
    # bad members, a piece without rows, a bad list_red, a bad point_of: host arrays raise, device arrays answer -1 for that tree alone
    good = box_case(2, 3, 2)
    want = twin(*TC.args_of(good), 4096, tol=TOL)
    pieces = len(good["piece_row"]) - 1
    first = lambda g: int(good["list_ptr"][g * 3])
    bads = []
    for value in (pieces, -1):
        c = dict(good, list_mem=good["list_mem"].copy()); c["list_mem"][first(2)] = value
        bads.append((c, {}))
    f = int(good["list_mem"][first(2)])
    c = dict(good, piece_row=good["piece_row"].copy())
    shift = c["piece_row"][f + 1] - c["piece_row"][f]
    c["pool"] = tuple(np.delete(v, np.s_[c["piece_row"][f]:c["piece_row"][f + 1]], axis=0) for v in good["pool"])
    c["piece_row"][f + 1:] -= shift                                                  # piece f has no rows now
    zero_rows = c
    c = dict(good, list_red=good["list_red"].copy()); c["list_red"][6] = 5
    bads.append((c, {}))
    bads.append((good, dict(point=np.zeros((2, 2)), point_of=np.array([0, 1, 2, 0, 1, 0]), point_tol=1e3)))
    for c, kw in bads:
        with pytest.raises(ValueError, match="tree 2"):
            twin(*TC.args_of(c), 4096, tol=TOL, **kw)
        got = twin(*TC.args_of(c), 4096, tol=TOL, device=True, **kw)
        assert got["tree_leaves"].tolist() == [v if g != 2 else -1 for g, v in enumerate(want["tree_leaves"])]
        assert leaves_of(got) == [lf for lf in leaves_of(want) if lf[0] != 2]
    with pytest.raises(ValueError, match="tree 2"):
        twin(*TC.args_of(zero_rows), 4096, tol=TOL)
    # lists must not overlap in list_mem: a list_ptr that does not ascend as a whole is refused, and on device arrays no tree is walked
    p = good["list_ptr"].copy(); p[7] = p[6] - 1
    with pytest.raises(ValueError, match="list_ptr"):
        twin(*TC.args_of(dict(good, list_ptr=p)), 4096, tol=TOL)
    got = twin(*TC.args_of(dict(good, list_ptr=p)), 4096, tol=TOL, device=True)
    assert got["tree_leaves"].tolist() == [-1] * 6 and got["n_leaves"] == 0 and not got["tested"].any()
    got = twin(*TC.args_of(zero_rows), 4096, tol=TOL, device=True)
    assert got["tree_leaves"][2] == -1 and (np.delete(got["tree_leaves"], 2) >= 0).all() and got["n_leaves"] == got["tree_leaves"].sum() + 1
    # the longest pieces add up to 511: taken; to 512: refused
    out = twin(*TC.args_of(long_case(256)), 4, tol=TOL)
    assert out["tested"].tolist() == [1, 1] and leaves_of(out) == [(0, (0, 1))]
    with pytest.raises(ValueError, match="511"):
        twin(*TC.args_of(long_case(257)), 4, tol=TOL)
    assert twin(*TC.args_of(long_case(257)), 4, tol=TOL, device=True)["tree_leaves"].tolist() == [-1]
    for L, cap in ((1, 4), (33, 4), (2, 0), (2, (1 << 22) + 1)):
        with pytest.raises(ValueError):
            twin(*good["pool"], good["piece_row"], L, np.zeros(L + 1, np.int32), np.zeros(0, np.int32), np.zeros(L, np.int32), cap)
    # no tree
    out = twin(*good["pool"], good["piece_row"], 3, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), 4)
    assert out["n_leaves"] == 0 and out["tree_leaves"].shape == (0,) and not out["tested"].any()


# ---- the front ends ---------------------------------------------------------------------------------------------------------------
def as_pieces(c):
    A, l, u, ol, oh = c["pool"]
    pr = c["piece_row"]
    return [(A[a:b], l[a:b], u[a:b], ol[a:b] != 0, oh[a:b] != 0) for a, b in zip(pr[:-1], pr[1:])]


def as_trees(c):
    return [([[f for f, _ in mem] for mem in TC.tree_lists(c, g)], [sum(comp for _, comp in mem) for mem in TC.tree_lists(c, g)])
            for g in range(c["trees"])]


def test_intersection_trees_groups_by_shape_and_falls_back_by_the_rules():
    two, three = box_case(2, 3, 2), box_case(3, 5, 4)
    pieces = as_pieces(two)
    trees = as_trees(two)
    base = len(pieces)
    pieces += as_pieces(three)
    trees += [([[base + f for f in mem] for mem in lists], reds) for lists, reds in as_trees(three)]
    want = [[t for g, t in leaves_of(polyhedra.intersection_trees_host(*TC.args_of(c), 4096, tol=TOL)) if g == k] for c in (two, three)
            for k in range(6)]
    want = want[:6] + [[tuple(base + f for f in t) for t in ts] for ts in want[6:]]
    # pool positions are positions in `pieces` here: the pools hold every piece once, in order
    spy = Spy()
    leaves, stats = polyhedra.intersection_trees(pieces, trees, spy, tol=TOL)
    assert leaves == want and stats["fallback"] == [] and stats["calls"] == 2
    assert spy.count("intersection_trees") == 2 and spy.count("exemplar_products", "exemplar_polys", "solve_lps", "solve_nodes") == 0
    assert stats["tested"] == spy.tested < stats["products"]
    # the rules: one list alone, a piece that is closed with l == u, a piece without rows, an engine without the method
    flat = (np.eye(2), np.array([0.5, 0.5]), np.array([0.5, 0.5]), np.zeros(2, bool), np.zeros(2, bool))
    none = (np.zeros((0, 2)), np.zeros(0), np.zeros(0), np.zeros(0, bool), np.zeros(0, bool))
    k = len(pieces)
    more = pieces + [flat, none]
    lists0 = trees[0][0]
    odd = [([lists0[0]], [0]), ([lists0[0], [k]], [0, 0]), ([lists0[0], lists0[1] + [k + 1]], [0, 0]), trees[0]]
    spy = Spy()
    leaves, stats = polyhedra.intersection_trees(more, odd, spy, tol=TOL)
    assert stats["fallback"] == [0, 1, 2] and spy.count("intersection_trees") == 1 and spy.count("exemplar_products") >= 1
    assert leaves[3] == want[0] and leaves[0] == [(f,) for f in lists0[0]]
    assert leaves[2] == [(a, b) for a in lists0[0] for b in lists0[1] + [k + 1] if b == k + 1 or not one_verdict(two, (a, b))[0]]
    old = ProductsSpy()
    leaves, stats = polyhedra.intersection_trees(pieces, trees[:6], old, tol=TOL)
    assert leaves == want[:6] and stats["fallback"] == list(range(6)) and old.count("exemplar_products") >= 1
    # an overflow is retried once with the true products
    spy = Spy()
    wide = TC.boxes_of(TC.overlapping_boxes(9), [[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    low = polyhedra.TREE_ALIVE_GUESS
    try:
        polyhedra.TREE_ALIVE_GUESS = 1
        leaves, stats = polyhedra.intersection_trees(as_pieces(wide), as_trees(wide), spy, tol=TOL)
    finally:
        polyhedra.TREE_ALIVE_GUESS = low
    assert stats["calls"] == 2 and stats["fallback"] == [] and len(leaves[0]) == 27


def test_combine_at_by_the_tree_equals_the_products_route():
    regions, solutions, x = _kink()
    want = qp_processing.combine_at(regions, solutions, x, Spy(), route="products")
    spy = Spy()
    _same_pieces(qp_processing.combine_at(regions, solutions, x, spy, route="tree"), want)
    # the kink's S2 is closed with l == u: the shortcut rule sends the tree to isempty_products
    assert spy.count("intersection_trees") == 0 and spy.count("exemplar_products") >= 1
    for pt in ((-1.0, 0.0), (0.5, 0.5)):
        a = qp_processing.combine_at(regions, solutions, np.array(pt), Spy(), route="products")
        _same_pieces(qp_processing.combine_at(regions, solutions, np.array(pt), Spy(), route="tree"), a)
    # the kink with a solution piece that has an interior: the walk is the entry's, and no tuple goes to exemplar_products
    S2 = Poly(np.array([[1.0, 0.0], [0.0, 1.0]]), [0.0, 0.0], [1.0, 1.0])
    S3 = Poly(np.array([[1.0, 0.0], [0.0, 1.0]]), [-1.0, -1.0], [0.0, 0.0])
    R3 = Poly(np.array([[1.0, 1.0]]), [-INF], [0.0])
    regions, solutions = regions + [[R3]], [solutions[0], [S2], [S3]]
    want = qp_processing.combine_at(regions, solutions, x, Spy(), route="products")
    spy = Spy()
    _same_pieces(qp_processing.combine_at(regions, solutions, x, spy, route="tree"), want)
    assert len(want) >= 2 and spy.count("intersection_trees") == 1 and spy.count("exemplar_products", "exemplar_polys", "solve_lps") == 0
    # an engine without the method goes the way of the products route; the size guard comes back as it did
    _same_pieces(qp_processing.combine_at(regions, solutions, x, ProductsSpy(), route="tree"), want)
    many = ([[regions[0][0]]] * 4, [[solutions[0][0]] * 6] * 4)
    with pytest.raises(RuntimeError, match="Too many solutions"):
        qp_processing.combine_at(*many, x, Spy(), route="tree")
    assert qp_processing.EMPTINESS_ROUTE == "nodes"


def test_golden_cases_by_the_tree_equal_the_products_route(monkeypatch):
    """solve() on the reference's end-to-end cases: every combine_many it makes is asked again by "products" and by "tree", piece for
    piece equal; on the tree route no exemplar_products call carries more tuples than the walk tested."""
    c = G.load("simple_bilevel_cases.json")
    inner = qp_processing.combine_many
    seen = []

    def both(jobs, x, eng, **kw):
        kw.pop("route", None)
        want = inner(jobs, x, Spy(), route="products", **kw)
        spy = Spy()
        got = inner(jobs, x, spy, route="tree", **kw)
        for a, b in zip(got, want):
            _same_pieces(a, b)
        sent = [int(s[6].split("[")[1].split(",")[0]) for m, s in spy.log if m == "exemplar_products"]      # tuples per call
        tested = getattr(spy, "tested", 0)
        assert all(n <= tested for n in sent), (sent, tested)              # no call carries more tuples than the walk tested
        seen.append((spy.count("intersection_trees"), sum(sent), tested, sum(len(a) for a in got)))
        return inner(jobs, x, eng, **kw)

    monkeypatch.setattr(qp_processing, "combine_many", both)
    import qpn_amd.level_batch as lb
    if hasattr(lb, "combine_many"):
        monkeypatch.setattr(lb, "combine_many", both)
    for w in c["w"]:
        ret = algorithm.solve(examples.setup("simple_bilevel", gen_solution_map=True), np.array(list(w) + c["x0"], float), engine=Spy())
        assert ret["solved"]
    assert seen and any(n for _, _, _, n in seen)
    print("combine_many calls (tree calls, tuples sent to exemplar_products, candidates the walk tested, pieces):", seen)
    # none of these jobs falls under a fallback rule: each is walked, and not one tuple goes to exemplar_products
    assert len(seen) == 4 and all(trees >= 1 and tuples == 0 and tested > 0 for trees, tuples, tested, _ in seen)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_symbol_and_its_signature():
    import ctypes
    from qpn_amd import _lib
    assert "qpn_intersection_trees" in _lib.ABI_SYMBOLS and _lib.TREE_MAX_L == 32 and _lib.TREE_MAX_CAP == 1 << 22
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "qpn_hip.h")).read()
    assert "int qpn_intersection_trees(qpn_ctx *ctx" in header and "#define QPN_ABI_VERSION 1" in header
    assert "qpn_tree" in open(os.path.join(root, "quadraticprogramnetworks.jl_amd", "csrc", "build.sh")).read()
    if os.path.exists(_lib.LIB_PATH):
        vp, i32, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
        lib = _lib.load_library()
        assert list(lib.qpn_intersection_trees.argtypes) == [vp, i32, i32, vp, vp, vp, vp, vp, i32, vp, i32, i32, i32, vp, vp, vp, i32, vp, vp,
                                                              f64, f64, f64, ctypes.POINTER(_lib.LpOpts), i32] + [vp] * 9 + [ctypes.c_int]
