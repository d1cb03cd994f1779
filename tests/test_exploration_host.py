"""QPNetOptions.exploration_vertices on CPU, arithmetic served by the oracle test double; the `-m gpu` twin is
tests/test_gpu_exploration.py.

What is pinned here:
* a three-variable counterexample where the verified multiplier is not unique: without exploration the follower's graph is the
  thin piece {y = x = 0}, the leader is pinned by it and solve() ends at x = 0; with exploration_vertices = 3 the two further
  pieces appear and solve() ends at the equilibrium (-1, 1, 1), for either order of the follower's two rows;
* the numpy twin of qpn_multiplier_vertices finds exactly the vertices of an enumeration over column subsets, and a breadth-first
  prefix with VERTEX_BUDGET when the budget is smaller; the EMPTY and NO_VERTEX statuses;
* a graph with exploration contains every piece of the graph without it;
* exploration_vertices 0 and 1 launch nothing new and change no result;
* max_pieces counts the distinct recipes of an item over its products."""
import warnings

import numpy as np
import pytest

from exploration_cases import X0, brute_vertices, counterexample_net, degenerate_case
from qpn_amd import algorithm, examples
from qpn_amd import level_batch as lb


@pytest.fixture()
def eng():
    from oracle_engine import OracleEngine
    return OracleEngine()


@pytest.mark.parametrize("swap", [False, True])
def test_counterexample_default_stops_on_the_thin_piece(eng, swap):
    net, lead, fol = counterexample_net(swap)
    r = algorithm.solve(net, X0, engine=eng)
    assert r["solved"]
    assert np.max(np.abs(r["x_opt"] - X0)) <= 1e-9


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("max_pieces", [64, None])
def test_counterexample_with_exploration_reaches_the_equilibrium(eng, swap, max_pieces):
    net, lead, fol = counterexample_net(swap, exploration_vertices=3, max_pieces=max_pieces)
    r = algorithm.solve(net, X0, engine=eng)
    assert r["solved"]
    assert np.max(np.abs(r["x_opt"] - np.array([-1.0, 1.0, 1.0]))) <= 1e-6


def _follower_pieces(eng, E, swap=False, max_pieces=64):
    net, lead, fol = counterexample_net(swap)
    items = [(fol, [])]
    recs, batches, rets = lb.verify_items(net, items, X0, eng)
    assert rets[0]["solution"]
    return lb.solution_pieces(net, recs, batches, rets, X0, eng, [True], max_pieces=max_pieces, exploration_vertices=E)[0]


def _keys(pieces):
    return {lb._poly_key(P) for P in pieces}


def test_counterexample_follower_graph_has_three_pieces(eng):
    assert len(_follower_pieces(eng, 0)) < 3
    got = _follower_pieces(eng, 3)
    assert len(got) == 3
    assert _keys(_follower_pieces(eng, 0)) <= _keys(got)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("kind", ["lp", "mixed", "dependent"])
def test_twin_equals_brute_force(seed, kind):
    rng = np.random.default_rng(100 + seed)
    n, m = [(2, 5), (3, 6), (3, 8), (4, 10), (2, 9), (5, 10)][seed]
    E, g, cls, lam = degenerate_case(rng, n, m, kind)
    want = brute_vertices(E, g, cls)
    verts, count, status = lb.multiplier_vertices_host(E[None], g[None], cls[None], lam[None], 400, max_bases=100000)
    got = {tuple(np.round(v, 5) + 0.0) for v in verts[0, :count[0]]}
    if status[0] == lb.MV_NO_VERTEX:
        assert count[0] == 0
        return
    assert status[0] == lb.MV_COMPLETE
    assert got == want and count[0] == len(want)
    if len(want) >= 3:
        V = len(want) - 1
        v2, c2, s2 = lb.multiplier_vertices_host(E[None], g[None], cls[None], lam[None], V, max_bases=100000)
        assert s2[0] == lb.MV_VERTEX_BUDGET and c2[0] == V
        assert np.array_equal(v2[0, :V], verts[0, :V])          # the breadth-first prefix


def test_twin_statuses():
    E = np.array([[1.0, 1.0], [0.0, 0.0]])
    v, c, s = lb.multiplier_vertices_host(E[None], np.array([[1.0, 1.0]]), np.zeros((1, 2), np.uint8), np.array([[0.5, 0.5]]), 4)
    assert s[0] == lb.MV_EMPTY and c[0] == 0
    E = np.array([[1.0, 1.0, 1.0]])
    cls = np.array([[lb.MV_FREE, lb.MV_FREE, lb.MV_GE]], np.uint8)
    v, c, s = lb.multiplier_vertices_host(E[None], np.array([[1.0]]), cls, np.array([[0.5, 0.5, 0.0]]), 4)
    assert s[0] == lb.MV_NO_VERTEX and c[0] == 0
    # the simplex {lambda >= 0 : sum = 1} in R^6: six vertices, one basis budget too small
    E = np.ones((1, 6))
    v, c, s = lb.multiplier_vertices_host(E[None], np.array([[1.0]]), np.zeros((1, 6), np.uint8), np.full((1, 6), 1 / 6), 10)
    assert s[0] == lb.MV_COMPLETE and c[0] == 6
    v, c, s = lb.multiplier_vertices_host(E[None], np.array([[1.0]]), np.zeros((1, 6), np.uint8), np.full((1, 6), 1 / 6), 10,
                                          max_bases=3)
    assert s[0] == lb.MV_BASIS_BUDGET and c[0] == 3


def test_recipe_filter_twin():
    masks = np.array([[0x10, 0x30], [0x30, 0x10], [0x30, 0x30]], np.uint8)
    first = np.array([0, 0, 0], np.int32)
    K = np.array([[5, 5], [5, 6], [6, 5], [6, 6]], np.uint8)
    keep = lb.recipe_filter_host(masks, np.concatenate([K, K]), np.array([1] * 4 + [2] * 4), first)
    assert keep.tolist() == [0, 0, 1, 1] + [0, 0, 0, 1]
    assert lb.distinct_recipes(list(masks)) == 4.0


@pytest.mark.parametrize("n,m,pairs", [(3, 5, 3), (4, 4, 2)])
def test_exploration_graph_contains_the_default_graph(eng, n, m, pairs):
    net = examples.setup("synthetic_pairs", pairs=pairs, n=n, m=m)
    r = algorithm.solve(net, engine=eng)
    assert r["solved"]
    players = sorted(net.network_depth_map[2])
    for x in (r["x_opt"], np.zeros(net.num_vars)):
        items = [(pid, []) for pid in players]
        recs, batches, rets = lb.verify_items(net, items, x, eng)
        want = [bool(t["solution"]) for t in rets]
        if not any(want):
            continue
        base = lb.solution_pieces(net, recs, batches, rets, x, eng, want)
        for E in (2, 10):
            got = lb.solution_pieces(net, recs, batches, rets, x, eng, want, exploration_vertices=E)
            for a, b in zip(base, got):
                if a is not None:
                    assert _keys(a) <= _keys(b)


def test_counterexample_follower_graph_contains_the_default_graph_on_config2(eng):
    net = examples.setup("robust_avoid_simple", seed=1)
    r = algorithm.solve(net, engine=eng)
    assert r["solved"]
    for level in (2, 3):
        players = sorted(net.network_depth_map[level])
        items = [(pid, []) for pid in players if not net.network_edges[pid]]
        if not items:
            continue
        recs, batches, rets = lb.verify_items(net, items, r["x_opt"], eng)
        want = [bool(t["solution"]) for t in rets]
        base = lb.solution_pieces(net, recs, batches, rets, r["x_opt"], eng, want)
        got = lb.solution_pieces(net, recs, batches, rets, r["x_opt"], eng, want, exploration_vertices=10)
        for a, b in zip(base, got):
            if a is not None:
                assert _keys(a) <= _keys(b)


class _NoVertices:
    """The oracle engine with a multiplier_vertices that must not be called."""

    def __init__(self):
        from oracle_engine import OracleEngine
        self._e = OracleEngine()
        self.device = -1

    def __getattr__(self, name):
        return getattr(self._e, name)

    def multiplier_vertices(self, *a, **k):
        raise AssertionError("multiplier_vertices called with exploration off")

    def recipe_filter(self, *a, **k):
        raise AssertionError("recipe_filter called with exploration off")


@pytest.mark.parametrize("E", [0, 1])
def test_default_off_launches_nothing_and_changes_nothing(eng, E):
    net, lead, fol = counterexample_net(exploration_vertices=E)
    r = algorithm.solve(net, X0, engine=_NoVertices())
    ref = algorithm.solve(counterexample_net()[0], X0, engine=eng)
    assert r["solved"] and np.array_equal(r["x_opt"], ref["x_opt"])
    net = examples.setup("robust_avoid_simple", seed=2, exploration_vertices=E)
    r = algorithm.solve(net, engine=_NoVertices())
    ref = algorithm.solve(examples.setup("robust_avoid_simple", seed=2), engine=eng)
    assert r["solved"] == ref["solved"] and np.array_equal(r["x_opt"], ref["x_opt"])


def test_cap_counts_distinct_recipes_over_products(eng):
    """The follower's products overlap and hold 3 distinct recipes: a cap of 2 keeps the first two in product order and warns;
    a cap of 3 keeps all three pieces, as the uncapped route does."""
    with pytest.warns(UserWarning, match="3 local recipes, only the first 2"):
        two = _follower_pieces(eng, 3, max_pieces=2)
    assert len(two) == 2
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*local recipes.*")
        three = _follower_pieces(eng, 3, max_pieces=3)
    assert len(three) == 3 and _keys(two) <= _keys(three)
    assert _keys(three) == _keys(_follower_pieces(eng, 3, max_pieces=None))


def test_uncapped_refuses_more_than_2_24_distinct_recipes(eng, monkeypatch):
    monkeypatch.setattr(lb, "MAX_RECIPES", 2)
    with pytest.raises(RuntimeError, match="3 local recipes"):
        _follower_pieces(eng, 3, max_pieces=None)


def test_local_recipe_count_counts_the_union(eng):
    from qpn_amd.qp_processing import local_recipe_count
    net, lead, fol = counterexample_net()
    x = np.array([-1.0, 0.0, 0.0])
    base = local_recipe_count(net, fol, x, {}, engine=eng)
    assert local_recipe_count(net, fol, x, {}, engine=eng, exploration_vertices=1) == base
    assert local_recipe_count(net, fol, x, {}, engine=eng, exploration_vertices=3) == 3 > base
