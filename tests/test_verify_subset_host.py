"""The host side of the subset verify: the route switch of process_level.

A stand-in engine, the CPU oracle behind a resident handle that has verify and verify_subset; both verify the rows they are asked
for and count them.  With level_batch.SUBSET_VERIFY_ROUTE on, a process_level sweep over an all-leaf level whose memo holds some
players' results verifies exactly the other players through one verify_subset call, makes the full call when the memo holds none
and no call when it holds all, and returns what it returns with the route off, value for value."""
import numpy as np

from oracle_engine import OracleEngine


class _CountingHandle:
    """Nodes.verify and Nodes.verify_subset on host arrays, served by the oracle's verify_nodes over the rows asked for."""

    def __init__(self, eng, records):
        self.eng, self.records = eng, [np.array(a) for a in records]
        self.batch, self.n = self.records[2].shape
        self.m = self.records[5].shape[1]

    def _rows(self, rows, xd, w, tol):
        self.eng.verified.extend(int(r) for r in rows)
        return OracleEngine.verify_nodes(self.eng, *[a[rows] for a in self.records], xd, w, tol=tol)

    def verify(self, xd, w, tol=1e-4):
        assert np.shape(xd) == (self.batch, self.n)
        self.eng.full_calls += 1
        return self._rows(np.arange(self.batch), xd, w, tol)

    def verify_subset(self, idx, xd, w, tol=1e-4):
        idx = np.asarray(idx)
        assert idx.dtype == np.int32 and idx.ndim == 1 and np.shape(xd) == (idx.size, self.n) and np.shape(w)[0] == idx.size
        assert idx.min() >= 0 and idx.max() < self.batch
        self.eng.subset_calls.append(idx.copy())
        return self._rows(idx, xd, w, tol)


class _CountingEngine(OracleEngine):
    def __init__(self):
        super().__init__()
        self.verified, self.full_calls, self.subset_calls = [], 0, []

    def upload_nodes(self, *records):
        return _CountingHandle(self, records)


def _net():
    from qpn_amd import examples, level_batch
    net = examples.setup("synthetic_pairs", pairs=6, n=3, m=4)
    followers = sorted(i for i in net.qps if not net.network_edges[i])
    x0 = 0.1 * np.random.default_rng(5).standard_normal(net.num_vars)
    # the followers' own solutions at x0: process_level accepts them and builds their solution graphs
    x = level_batch.solve_level(net, followers, x0, engine=OracleEngine())
    return net, followers, x


def _moved(net, followers, x, which, seed=9):
    """x with the variables of the pairs of followers[which] moved (their own and their leaders')."""
    from qpn_amd import level_batch
    x2 = x.copy()
    rng = np.random.default_rng(seed)
    for k in which:
        cols = level_batch._subtree_cols(net, followers[k])
        x2[cols] += 0.05 * rng.standard_normal(cols.size)
    return x2


def _two_sweeps(route, which):
    """process_level at x, then at x with the pairs `which` moved; the second sweep's results and what it verified."""
    from qpn_amd import level_batch
    net, followers, x = _net()
    eng = _CountingEngine()
    assert level_batch.SUBSET_VERIFY_ROUTE is False
    level_batch.SUBSET_VERIFY_ROUTE = route
    try:
        r1 = level_batch.process_level(net, followers, x, {}, engine=eng)
        assert eng.full_calls == 1 and not eng.subset_calls and sorted(eng.verified) == list(range(len(followers)))
        assert all(r["solution"] for r in r1)
        eng.verified, eng.full_calls = [], 0
        r2 = level_batch.process_level(net, followers, _moved(net, followers, x, which), {}, engine=eng)
    finally:
        level_batch.SUBSET_VERIFY_ROUTE = False
    return r1, r2, eng, followers


def _same(a, b):
    """Two process_level lists, value for value (a solution graph: its pieces' arrays and open-bound flags)."""
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        assert set(ra) == set(rb)
        for key in ra:
            if key != "S" or ra["S"] is None:
                assert ra[key] == rb[key], key
                continue
            assert len(ra["S"]) == len(rb["S"])
            for Pa, Pb in zip(ra["S"], rb["S"]):
                assert all(np.array_equal(u, v) for u, v in zip(Pa.vectorize(), Pb.vectorize()))
                assert all(np.array_equal(u, v) for u, v in zip(Pa.open_bounds(), Pb.open_bounds()))


def test_route_verifies_exactly_the_moved_followers():
    which = [1, 4]
    _, off, e0, followers = _two_sweeps(False, which)
    first, on, e1, _ = _two_sweeps(True, which)
    # off: the code as it was -- every node of the level, one full call
    assert e0.full_calls == 1 and not e0.subset_calls and sorted(e0.verified) == list(range(len(followers)))
    # on: the two moved followers and nothing else, in one subset call
    assert e1.full_calls == 0 and len(e1.subset_calls) == 1 and e1.verified == which
    assert e1.subset_calls[0].tolist() == which
    _same(on, off)
    # (the sweep says something: the moved followers' results are new, the others are the memo's objects)
    for k in range(len(followers)):
        assert (on[k] is first[k]) == (k not in which)


def test_route_makes_the_full_call_without_a_hit():
    which = list(range(6))
    _, off, e0, _ = _two_sweeps(False, which)
    _, on, e1, followers = _two_sweeps(True, which)
    assert e1.full_calls == 1 and not e1.subset_calls and sorted(e1.verified) == list(range(len(followers)))
    _same(on, off)


def test_route_makes_no_call_when_every_player_is_a_hit():
    first0, off, e0, followers = _two_sweeps(False, [])
    first, on, e1, _ = _two_sweeps(True, [])
    assert e0.full_calls == 1 and len(e0.verified) == len(followers)          # off: all verified again
    assert e1.full_calls == 0 and not e1.subset_calls and not e1.verified
    _same(on, off)
    assert all(a is b for a, b in zip(on, first))
