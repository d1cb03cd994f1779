"""The one solution-pieces pipeline on the MI355X: the capped route (host arrays, _finish_host) against the uncapped route
(device arrays, qpn_finish_pieces) on the hand-built levels where the two readers have something to differ in, and the C-ABI
calls of the default path."""
import collections

import pytest

import qpn_amd  # noqa: F401
from qpn_amd import algorithm, examples, level_batch

from test_complete_solution_graphs import _level, _same_pieces, hand_built_levels

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["offpoint", "nomember", "parallel", "twice", "twice_scaled"])
def test_capped_and_uncapped_routes_agree_on_hip(engine, name):
    """Non-members and the fallback, merge candidates, flagged pieces and duplicates: max_pieces=64 (no level reaches it)
    against max_pieces=None in one round and in rounds of 3, Poly by Poly and bit for bit."""
    net, players, x = hand_built_levels()[name]
    recs, batches, rets, want = _level(net, players, x, engine)
    assert any(want)
    ref = level_batch.solution_pieces(net, recs, batches, rets, x, engine, want, max_pieces=64)
    for chunk in (None, 3):
        _same_pieces(ref, level_batch.solution_pieces(net, recs, batches, rets, x, engine, want, max_pieces=None, _chunk=chunk))


# what one solution_pieces call of the default path cost at the commit before the three bodies became one pipeline
DEFAULT_PATH_CALLS = {"qpn_comp_indices": 2, "qpn_recipes_batch": 1, "qpn_reduced_pieces": 1}


def test_default_path_abi_calls(engine):
    """Four synthetic pairs (n = 3, m = 5), default options, the followers' level at the solve's answer: the C-ABI calls of one
    solution_pieces call, by name and by count."""
    net = examples.setup("synthetic_pairs", pairs=4, n=3, m=5)
    r = algorithm.solve(net, engine=engine)
    assert r["solved"]
    players = sorted(net.network_depth_map[2])
    recs, batches, rets, want = _level(net, players, r["x_opt"], engine)
    assert any(want)
    before = collections.Counter(engine.calls)
    level_batch.solution_pieces(net, recs, batches, rets, r["x_opt"], engine, want)
    after = collections.Counter(engine.calls)
    assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == DEFAULT_PATH_CALLS
