"""qpn_intersection_trees (csrc/qpn_tree.hip) against its numpy twin polyhedra.intersection_trees_host: every
output equal, in host and in device mode, on the box family and the planted trees of tests/test_intersection_trees_host.py, a
frontier over several scan chunks with cap met exactly and missed by one, many trees in one call, the redzone, null flags and
points, no tree, the argument errors and bad device members; and the host functions that use it -- combine_at with route="tree"
against route="products", solve() end to end with qp_processing.EMPTINESS_ROUTE switched."""
from __future__ import annotations

import numpy as np
import pytest

import goldenio as G
import tree_cases as TC
from test_intersection_trees_host import BOX_CASES, box_case, leaves_of, long_case, planted, redzone_case
from tree_cases import TOL

pytestmark = pytest.mark.gpu

INF = np.inf
COUNTS = ("tree_leaves", "tested", "alive", "unanswered")


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _same(got, want, what):
    k = int(_host(got["n_leaves"])[0])
    assert k == want["n_leaves"] and int(_host(got["overflow"])[0]) == want["overflow"], (what, k, want["n_leaves"], _host(got["overflow"]))
    for key in COUNTS:
        g = _host(got[key])
        assert g.dtype == want[key].dtype and np.array_equal(g, want[key]), (what, key, g, want[key])
    for key in ("leaves", "leaf_tree", "leaf_how"):
        g = _host(got[key])[:k]
        assert g.dtype == np.int32 and np.array_equal(g, want[key]), (what, key, g, want[key])


def _dev(engine, a, dtype):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=f"cuda:{engine.device}")


def _both_modes(engine, c, cap, want=None, device_twin=False, point=None, point_of=None, **kw):
    """The entry in host and in device mode against the twin (`want`: a twin answer the caller has).  -> the twin's answer."""
    from qpn_amd import polyhedra
    A, l, u, ol, oh = c["pool"]
    rest = (c["piece_row"], c["L"], c["list_ptr"], c["list_mem"], c["list_red"])
    if want is None:
        want = polyhedra.intersection_trees_host(A, l, u, ol, oh, *rest, cap, point=point, point_of=point_of, device=device_twin, **kw)
    if not device_twin:
        got = engine.intersection_trees(A, l, u, ol, oh, *rest, cap, point=point, point_of=point_of, **kw)
        assert got["leaves"].shape == (want["n_leaves"], c["L"])
        _same(got, want, "host mode")
    f, b, i = (lambda a: _dev(engine, a, np.float64)), (lambda a: _dev(engine, a, np.uint8)), (lambda a: _dev(engine, a, np.int32))
    got = engine.intersection_trees(f(A), f(l), f(u), b(ol), b(oh), i(rest[0]), rest[1], i(rest[2]), i(rest[3]), i(rest[4]), cap,
                                    point=f(point), point_of=i(point_of), **kw)
    assert all(hasattr(v, "cpu") for v in got.values()) and got["leaves"].shape == (cap, c["L"])
    _same(got, want, "device mode")
    return want


@pytest.mark.parametrize("d,L,seed", BOX_CASES)
def test_the_box_family_equals_the_twin(engine, d, L, seed):
    c = box_case(d, L, seed)
    n0 = engine.calls["qpn_intersection_trees"]
    want = _both_modes(engine, c, 4096, tol=TOL)
    assert engine.calls["qpn_intersection_trees"] == n0 + 2
    assert want["n_leaves"] > 0 and all(0 < a < t for a, t in zip(want["alive"][1:], want["tested"][1:]))
    # depth 2 alone holds at least three row counts: three launches of the LP kernels for one depth
    ns = {TC.rows_of(c, (a, b)) for g in range(c["trees"]) for a, _ in TC.tree_lists(c, g)[0] for b, _ in TC.tree_lists(c, g)[1]}
    assert len(ns) >= 3


def test_the_planted_trees_and_the_redzone(engine):
    want = _both_modes(engine, planted(), 64, tol=TOL)
    assert want["tested"].tolist() == [2, 6, 12] and want["alive"].tolist() == [2, 3, 12]
    want = _both_modes(engine, redzone_case(), 64, tol=TOL)
    assert want["tree_leaves"].tolist() == [0, 1]                       # a tree that ends with no leaf, next to one with a leaf
    dead = dict(redzone_case(), list_red=np.array([1, 1, 1, 1], np.int32))
    want = _both_modes(engine, dead, 64, tol=TOL)
    assert want["n_leaves"] == 0 and want["tested"].tolist() == [3, 3]


def test_a_frontier_over_several_scan_chunks_with_cap_met_and_missed_by_one(engine):
    """One tree of three lists of 12 mutually overlapping boxes: 12, 144, 1 728 candidates, all kept."""
    boxes = TC.overlapping_boxes(36, d=3)
    c = TC.boxes_of(boxes, [list(range(12)), list(range(12, 24)), list(range(24, 36))])
    want = _both_modes(engine, c, 1728, tol=TOL)
    assert want["n_leaves"] == 1728 and want["tested"].tolist() == [12, 144, 1728] and want["overflow"] == 0
    assert leaves_of(want) == [(0, t) for t in TC.all_tuples(c, 0)]
    over = _both_modes(engine, c, 1727, tol=TOL)
    assert over["overflow"] == 3 and over["n_leaves"] == 0 and over["tested"].tolist() == [12, 144, 1728] and over["alive"].tolist() == [12, 144, 0]


def test_forty_trees_in_one_call_some_dead_at_depth_one(engine):
    g = np.random.default_rng(40)
    widths = [[int(g.integers(1, 5)) for _ in range(3)] for _ in range(40)]
    c = TC.box_trees(7, 2, 3, widths, grid=2)
    point = np.array([[0.7, 0.7], [9.0, 9.0], [0.2, 0.7]])
    point_of = np.array([1 if k % 7 == 3 else 2 if k % 5 == 1 else 0 for k in range(40)], np.int32)
    want = _both_modes(engine, c, 4096, point=point, point_of=point_of, point_tol=TC.POINT_TOL, tol=TOL)
    dead = [k for k in range(40) if k % 7 == 3]
    assert not want["tree_leaves"][dead].any() and want["n_leaves"] > 0 and want["tested"][0] < sum(w[0] for w in widths)
    assert len(set(want["leaf_tree"].tolist())) >= 5
    # null flags and null points
    A, l, u, _, _ = c["pool"]
    _both_modes(engine, dict(c, pool=(A, l, u, None, None)), 4096, tol=TOL)


def test_argument_errors_no_tree_and_bad_device_members(engine):
    from qpn_amd import polyhedra
    from qpn_amd.engine import QpnError
    good = box_case(2, 3, 2)
    A, l, u, ol, oh = good["pool"]
    pr, L, lp, lm, lr = good["piece_row"], 3, good["list_ptr"], good["list_mem"], good["list_red"]
    call = lambda c, cap=4096, **kw: engine.intersection_trees(*TC.args_of(c), cap, tol=TOL, **kw)
    # sizes beyond the limits
    for args in ((A, l, u, ol, oh, pr, 1, np.zeros(2, np.int32), lm[:0], np.zeros(1, np.int32), 4),
                 (A, l, u, ol, oh, pr, 33, np.zeros(34, np.int32), lm[:0], np.zeros(33, np.int32), 4),
                 (A, l, u, ol, oh, pr, L, lp, lm, lr, (1 << 22) + 1),
                 (np.zeros((1, 256)), np.zeros(1), np.ones(1), None, None, np.array([0, 1], np.int32), 2, np.array([0, 1, 2], np.int32),
                  np.zeros(2, np.int32), np.zeros(2, np.int32), 4)):
        with pytest.raises(QpnError, match="size"):
            engine.intersection_trees(*args)
    with pytest.raises(QpnError, match="size"):
        call(long_case(257), 4)
    with pytest.raises(QpnError, match="bad argument"):
        call(good, 0)
    # inconsistent shapes
    for bad in ((A, l[:3], u, ol, oh, pr, L, lp, lm, lr, 4), (A, l, u, ol, oh, pr, L, lp[:-1], lm, lr, 4), (A, l, u, ol, oh, pr, 4, lp, lm, lr, 4)):
        with pytest.raises(QpnError, match="inconsistent shapes"):
            engine.intersection_trees(*bad)
    with pytest.raises(QpnError, match="inconsistent shapes"):
        call(good, point=np.zeros((1, 2)))
    # host indices out of range, a CSR that is not ascending, a piece without rows, a redzone longer than its list: an argument error
    pieces = len(pr) - 1
    first = int(lp[6])
    bads = []
    for value in (pieces, -1):
        m = lm.copy(); m[first] = value
        bads.append(dict(good, list_mem=m))
    p = lp.copy(); p[7] = p[6] - 1
    bads.append(dict(good, list_ptr=p))
    r = lr.copy(); r[6] = 5
    bads.append(dict(good, list_red=r))
    f = int(lm[first])
    prz = pr.copy(); cut = prz[f + 1] - prz[f]
    zero_rows = dict(good, pool=tuple(np.delete(v, np.s_[pr[f]:pr[f + 1]], axis=0) for v in good["pool"]), piece_row=prz)
    prz[f + 1:] -= cut
    bads.append(zero_rows)
    for c in bads:
        with pytest.raises(QpnError, match="bad argument"):
            call(c)
    with pytest.raises(QpnError, match="bad argument"):
        call(good, point=np.zeros((2, 2)), point_of=np.array([0, 1, 2, 0, 1, 0], np.int32))
    # no tree
    got = engine.intersection_trees(A, l, u, ol, oh, pr, 3, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), 4)
    assert int(got["n_leaves"][0]) == 0 and int(got["overflow"][0]) == 0 and not got["tested"].any() and got["leaves"].shape == (0, 3)
    import torch
    dv = f"cuda:{engine.device}"
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dv)
    got = engine.intersection_trees(t(A, np.float64), t(l, np.float64), t(u, np.float64), None, None, t(pr, np.int32), 3, t(np.zeros(1), np.int32),
                                    t(np.zeros(0), np.int32), t(np.zeros(0), np.int32), 4)
    assert int(got["n_leaves"].cpu()[0]) == 0 and int(got["overflow"].cpu()[0]) == 0 and not got["alive"].cpu().numpy().any()
    # the longest pieces add up to 511: the largest job the entry takes
    want = _both_modes(engine, long_case(256), 4, tol=TOL)
    assert leaves_of(want) == [(0, (0, 1))]
    # device arrays: the bad tree answers -1 and its neighbours are what they were
    whole = polyhedra.intersection_trees_host(*TC.args_of(good), 4096, tol=TOL)
    for c in bads[:2] + bads[3:]:
        got = _both_modes(engine, c, 4096, device_twin=True, tol=TOL)
        assert got["tree_leaves"][2] == -1 and np.array_equal(np.delete(got["tree_leaves"], 2), np.delete(whole["tree_leaves"], 2))
    # a list_ptr that does not ascend could make lists overlap: no tree of such a call is walked
    got = _both_modes(engine, bads[2], 4096, device_twin=True, tol=TOL)
    assert got["tree_leaves"].tolist() == [-1] * 6 and got["n_leaves"] == 0 and not got["tested"].any()
    p = lp.copy(); p[3] = 0                                                     # tree 1's first list would lie over tree 0's
    assert p[2] > 0
    got = _both_modes(engine, dict(good, list_ptr=p), 4096, device_twin=True, tol=TOL)
    assert got["tree_leaves"].tolist() == [-1] * 6
    got = _both_modes(engine, good, 4096, device_twin=True, point=np.zeros((2, 2)), point_of=np.array([0, 1, 2, 0, 1, -1], np.int32),
                      point_tol=1e3, tol=TOL)
    assert got["tree_leaves"][[2, 5]].tolist() == [-1, -1] and np.array_equal(got["tree_leaves"][[0, 1, 3, 4]], whole["tree_leaves"][[0, 1, 3, 4]])
    got = _both_modes(engine, long_case(257), 4, device_twin=True, tol=TOL)
    assert got["tree_leaves"].tolist() == [-1] and got["n_leaves"] == 0


# ---- the host functions on the tree route against the products route ---------------------------------------------------------------
def _counts(engine):
    return engine.calls["qpn_intersection_trees"], engine.calls["qpn_exemplar_products"], engine.calls["qpn_exemplar_polys"], engine.calls["qpn_solve_lps"]


def _same_pieces(got, want):
    assert len(got) == len(want)
    for P, Q in zip(got, want):
        for a, b in zip(P.vectorize() + (P.open_lo, P.open_hi), Q.vectorize() + (Q.open_lo, Q.open_hi)):
            assert a.dtype == b.dtype and np.array_equal(a, b)


def test_combine_at_on_the_kink_by_the_tree_equals_the_products_route(engine):
    from qpn_amd.programs import Poly
    from qpn_amd.qp_processing import combine_at
    R1 = Poly(np.array([[0.0, 1.0], [1.0, 0.0]]), [0.0, -INF], [0.0, 0.0])
    R2 = Poly(np.array([[1.0, -1.0], [0.0, 1.0]]), [0.0, 0.0], [0.0, INF])
    S1 = Poly(np.array([[0.0, 1.0], [1.0, 0.0]]), [0.0, -INF], [0.0, 0.0])
    S2 = Poly(np.array([[1.0, 0.0], [0.0, 1.0]]), [0.0, 0.0], [0.0, 0.0])
    x = np.zeros(2)
    # the hand-worked kink: S2 is closed with l == u, the shortcut rule sends it the way of the products route
    want = combine_at([[R1], [R2]], [[S1], [S2]], x, engine, route="products")
    before = _counts(engine)
    _same_pieces(combine_at([[R1], [R2]], [[S1], [S2]], x, engine, route="tree"), want)
    after = _counts(engine)
    assert len(want) >= 2 and after[0] == before[0] and after[1] > before[1]
    # with solution pieces that have an interior, and a third union, the walk is the device's
    S2 = Poly(np.array([[1.0, 0.0], [0.0, 1.0]]), [0.0, 0.0], [1.0, 1.0])
    S3 = Poly(np.array([[1.0, 0.0], [0.0, 1.0]]), [-1.0, -1.0], [0.0, 0.0])
    R3 = Poly(np.array([[1.0, 1.0]]), [-INF], [0.0])
    regions, solutions = [[R1], [R2], [R3]], [[S1], [S2], [S3]]
    want = combine_at(regions, solutions, x, engine, route="products")
    before = _counts(engine)
    _same_pieces(combine_at(regions, solutions, x, engine, route="tree"), want)
    after = _counts(engine)
    assert len(want) >= 2 and after[0] == before[0] + 1 and after[1:] == before[1:]


def test_reference_end_to_end_cases_on_the_tree_route(engine, monkeypatch):
    """tests/test_gpu_host_logic.py's end-to-end cases with qp_processing.EMPTINESS_ROUTE = "tree": the equilibria of the default
    route, the reference's assertions, and every combine_many walks its trees on qpn_intersection_trees."""
    from qpn_amd import algorithm, examples, qp_processing
    assert qp_processing.EMPTINESS_ROUTE == "nodes"
    c = G.load("simple_bilevel_cases.json")
    assert len(c["w"]) == 8
    solve = lambda w: algorithm.solve(examples.setup("simple_bilevel", gen_solution_map=True), np.array(list(w) + c["x0"], float), engine=engine)
    default = [solve(w) for w in c["w"]]
    monkeypatch.setattr(qp_processing, "EMPTINESS_ROUTE", "tree")
    before = _counts(engine)
    for w, xs, min_pieces, old in zip(c["w"], c["accepted_xy"], c["min_pieces_root_graph"], default):
        ret = solve(w)
        assert ret["solved"] and old["solved"], ret
        assert np.array_equal(ret["x_opt"], old["x_opt"]), (w, ret["x_opt"], old["x_opt"])
        assert any(np.allclose(ret["x_opt"], list(w) + list(xy), atol=c["atol"]) for xy in xs), (w, ret["x_opt"])
        assert len(ret["Sol"][2]) >= min_pieces and len(ret["Sol"][2]) == len(old["Sol"][2]), (w, len(ret["Sol"][2]))
    after = _counts(engine)
    assert after[0] > before[0]
