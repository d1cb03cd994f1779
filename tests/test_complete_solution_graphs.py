"""Uncapped solution graphs (QPNetOptions.max_pieces = None) on CPU, arithmetic served by the oracle test double; the `-m gpu`
twin is tests/test_gpu_complete_solution_graphs.py.

What is pinned here:
* a two-node net whose answer the cap changes: the first 64 recipes of the follower all hold y_7 at its bound, under which x = 0
  is optimal for the leader; recipe 64 on frees y_7, and the true equilibrium is x = y = e_7.  The capped default warns, reports
  the follower in `truncated` and stops at 0; max_pieces=None reaches e_7 with `truncated == []`;
* the uncapped route (chunked enumeration, the numpy twin of qpn_finish_pieces) builds the same pieces, Poly by Poly and bit for
  bit, as the capped body given a cap no node reaches -- with chunks small enough that nodes span several;
* a node with more than 2^24 recipes is refused by name before anything is enumerated."""
import warnings

import numpy as np
import pytest

import qpn_amd  # noqa: F401
from qpn_amd import algorithm, examples, level_batch
from qpn_amd.programs import QPNet, QPNetOptions

INF = np.inf


@pytest.fixture()
def eng():
    from oracle_engine import OracleEngine
    return OracleEngine()


def counterexample_net(d=7, **opts):
    """Follower y in R^d: min 1/2 |y - x|^2 s.t. y >= 0 (row y_d last: the slowest digit of the recipe product); leader x in R^d:
    min 1/2 |x|^2 - y_d; edge leader -> follower; start at 0."""
    net = QPNet(2 * d)
    A = np.zeros((d, 2 * d)); A[np.arange(d), d + np.arange(d)] = 1.0
    cid = net.add_constraint(A, np.zeros(d), np.full(d, INF))
    Qf = np.block([[np.eye(d), -np.eye(d)], [-np.eye(d), np.eye(d)]])
    fol = net.add_qp(Qf, np.zeros(2 * d), [cid], list(range(d, 2 * d)))
    Ql = np.zeros((2 * d, 2 * d)); Ql[:d, :d] = np.eye(d)
    ql = np.zeros(2 * d); ql[2 * d - 1] = -1.0
    lead = net.add_qp(Ql, ql, [], list(range(d)))
    net.add_edges([(lead, fol)])
    net.assign_constraint_groups()
    net.set_options(**opts)
    net.default_initialization = np.zeros(2 * d)
    return net, lead, fol


def _level(net, players, x, eng):
    items = [(pid, []) for pid in players]
    recs, batches, rets = level_batch.verify_items(net, items, x, eng)
    want = [bool(r["solution"]) for r in rets]
    return recs, batches, rets, want


def test_default_cap_is_64():
    assert QPNetOptions().max_pieces == 64
    net, _, _ = counterexample_net()
    with warnings.catch_warnings():
        warnings.simplefilter("error")                    # a known option: no "Invalid option name" warning
        net.set_options(max_pieces=None)
    assert net.options.max_pieces is None


def test_counterexample_recipe_order(eng):
    """All 7 rows of the follower are weakly active at 0 and keep both codes 5 and 6: 128 recipes, of which number 64 is the first
    with the last row (y_7) at code 6 (free)."""
    net, lead, fol = counterexample_net()
    x = np.zeros(14)
    recs, batches, rets, want = _level(net, [fol], x, eng)
    assert want == [True]
    b = batches[0]
    masks, total = level_batch._piece_masks(b, [0], rets, want, 1e-2, eng)
    assert int(total[0]) == 128
    K, _ = eng.recipes_batch(masks, np.array([0, 128], np.int64))
    K = np.asarray(K)
    last = K[:, -1 - (b.m - b.m_true[0])]                 # the row of y_7 (constraint rows are padded after the true ones)
    assert np.all(last[:64] == 5) and np.all(last[64:] == 6)
    assert int(np.argmax(last == 6)) == 64


def test_counterexample_default_is_truncated(eng):
    net, lead, fol = counterexample_net()
    with pytest.warns(UserWarning, match="only the first 64"):
        r = algorithm.solve(net, engine=eng)
    assert r["solved"] and r["truncated"] == [fol]
    assert np.max(np.abs(r["x_opt"])) <= 1e-9


def test_counterexample_uncapped_reaches_the_equilibrium(eng):
    net, lead, fol = counterexample_net(max_pieces=None)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*local recipes.*")
        r = algorithm.solve(net, engine=eng)
    assert r["solved"] and r["truncated"] == []
    e7 = np.zeros(7); e7[6] = 1.0
    assert np.max(np.abs(r["x_opt"][:7] - e7)) <= 1e-6 and np.max(np.abs(r["x_opt"][7:] - e7)) <= 1e-6


def _same_pieces(a, b):
    assert len(a) == len(b)
    for Pa, Pb in zip(a, b):
        if Pa is None or Pb is None:
            assert Pa is None and Pb is None
            continue
        assert len(Pa) == len(Pb)
        for p, q in zip(Pa, Pb):
            (ca, Aa), (cb, Ab) = p.local(), q.local()
            assert np.array_equal(ca, cb) and np.array_equal(Aa, Ab)
            assert np.array_equal(p.l, q.l) and np.array_equal(p.u, q.u)


def follower_net(rows, lo):
    """counterexample_net with the follower's rows given: y in R^d minimises 1/2 |y - x|^2 s.t. rows y >= lo."""
    rows = np.asarray(rows, dtype=np.float64)
    d = rows.shape[1]
    net = QPNet(2 * d)
    cid = net.add_constraint(np.hstack([np.zeros_like(rows), rows]), np.asarray(lo, dtype=np.float64), np.full(len(rows), INF))
    fol = net.add_qp(np.block([[np.eye(d), -np.eye(d)], [-np.eye(d), np.eye(d)]]), np.zeros(2 * d), [cid], list(range(d, 2 * d)))
    Ql = np.zeros((2 * d, 2 * d)); Ql[:d, :d] = np.eye(d)
    ql = np.zeros(2 * d); ql[2 * d - 1] = -1.0
    lead = net.add_qp(Ql, ql, [], list(range(d)))
    net.add_edges([(lead, fol)])
    net.assign_constraint_groups()
    return net, fol


def hand_built_levels():
    """Follower levels on which the capped and the uncapped reader have something to differ in -- name -> (net, players, x):
    offpoint      rows y >= 0 in R^3 at x = y = (5e-5, 0, 0): 8 pieces, 4 of them non-members (a code kept by CODE_TOL whose piece
                  misses the point by more than MEMBER_TOL)
    nomember      y_1 >= 0 at x = 0, y = 5e-5: both pieces are non-members, the node keeps its fallback
    parallel      y_1 >= 0, 2 y_1 >= -1, y_2 >= 0 at 0: every piece is a merge candidate (_dedupe)
    twice         y_1 >= 0 twice, y_2 >= 0 at 0: 8 recipes, 6 merge candidates and 2 flagged (_flagged_piece); 6 pieces are kept,
                  2 are duplicates found by _poly_key
    twice_scaled  the same with the second row 2 y_1 >= 0."""
    e = np.eye(3)
    out = {}
    net, fol = follower_net(e, np.zeros(3))
    out["offpoint"] = (net, [fol], np.array([5e-5, 0, 0, 5e-5, 0, 0]))
    net, fol = follower_net([[1.0]], [0.0])
    out["nomember"] = (net, [fol], np.array([0.0, 5e-5]))
    net, fol = follower_net([e[0], 2 * e[0], e[1]], [0.0, -1.0, 0.0])
    out["parallel"] = (net, [fol], np.zeros(6))
    for name, s in (("twice", 1.0), ("twice_scaled", 2.0)):
        net, fol = follower_net([e[0], s * e[0], e[1]], np.zeros(3))
        out[name] = (net, [fol], np.zeros(6))
    return out


def parity_levels(eng):
    """Follower levels of three record shapes: the counterexample at its start (128 recipes) and two pair nets at a point
    off their equilibria (the solve's first iterate); then hand_built_levels."""
    out = []
    net, lead, fol = counterexample_net()
    out.append((net, [fol], np.zeros(14)))
    for n, m, pairs in ((3, 5, 4), (5, 3, 3)):
        net = examples.setup("synthetic_pairs", pairs=pairs, n=n, m=m)
        r = algorithm.solve(net, engine=eng)
        assert r["solved"]
        out.append((net, sorted(net.network_depth_map[2]), r["x_opt"]))
    return out + list(hand_built_levels().values())


@pytest.mark.parametrize("chunk", [None, 5])
def test_uncapped_route_matches_capped_body(eng, chunk):
    for net, players, x in parity_levels(eng):
        recs, batches, rets, want = _level(net, players, x, eng)
        assert any(want)
        ref = level_batch.solution_pieces(net, recs, batches, rets, x, eng, want, max_pieces=10 ** 9)
        cut = set()
        got = level_batch.solution_pieces(net, recs, batches, rets, x, eng, want, max_pieces=None, truncated=cut, _chunk=chunk)
        assert not cut
        _same_pieces(ref, got)


def test_recipes_range_twin_equals_slices(eng):
    g = np.random.default_rng(4)
    masks = g.integers(1, 256, size=(3, 5)).astype(np.uint8)
    masks[:, :2] &= 0x0F
    tot = [int(np.prod([bin(int(v)).count("1") for v in row])) for row in masks]
    K, node_of = eng.recipes_batch(masks, np.concatenate([[0], np.cumsum(tot)]).astype(np.int64))
    K = np.asarray(K)
    first = np.array([1, 0, tot[2] - 3]); cnt = np.array([min(4, tot[0] - 1), 0, 3])
    K2, no2 = level_batch._recipes_range_host(masks, first, cnt)
    base = np.concatenate([[0], np.cumsum(tot)])
    want = np.concatenate([K[base[b] + first[b]: base[b] + first[b] + cnt[b]] for b in range(3)])
    assert np.array_equal(K2, want) and np.array_equal(no2, np.repeat(np.arange(3), cnt))


def test_more_than_2_24_recipes_is_refused(eng):
    """25 weakly active rows with two codes each: 2^25 recipes.  solve() ends unsolved and names the node; nothing is enumerated."""
    net, lead, fol = counterexample_net(d=25, max_pieces=None)
    r = algorithm.solve(net, engine=eng)
    assert not r["solved"]
    assert f"node {fol}: 33554432 local recipes" in r["error"] and "2^24" in r["error"]
    assert eng.calls["recipes_batch"] == 0 and eng.calls["reduced_pieces"] == 0
