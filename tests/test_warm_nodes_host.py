"""The numpy twin of the warm-start kernel (level_batch.warm_nodes_host) and the opt-in route of solve_level.

On solve_cases.make_node nodes (tests/warm_cases.py: nine families, five shapes) the twin, given the planted sides, accepts every
node; given a hint that is wrong in one of seven ways it declines.  An accepted point is held to the truth: the active set its
multipliers claim is the planted one, solve_ref.solve_reference on that set ends with its certificate (the proof that the set is
THE solution's), and the point is within solve_ref.accuracy_bar of that certified solution -- the bar of the cold routes, from
the CPU oracle's own error on the same nodes.  (The certificate itself asks a stationarity residual of 2^-52 relative, which no
fp64 point has: it is applied where tests/solve_cases.py applies it, to the longdouble solve on the claimed set.)

Wiring: through a spy engine whose handle is served by the twin, WARM_DUALS_ROUTE = True passes the previous z and the flag for
the resident leaf batches only, and False makes no call that today's code does not make.
"""
import numpy as np
import pytest

import solve_cases as SC
import solve_ref as SR
import warm_cases as WC

import qpn_amd  # noqa: F401
from qpn_amd import _lib, algorithm, examples, level_batch
from qpn_amd.engine import colmajor
from oracle_engine import OracleEngine


def _abi(nodes):
    Q, R, qd, A, B, l, u = SC.stack(nodes)
    return [colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u]


@pytest.mark.parametrize("n,m", WC.SHAPES)
def test_planted_sides_are_accepted_and_certified(oracle, n, m):
    nodes = WC.shape_nodes(n, m)
    rng = np.random.default_rng([1, n, m])
    hints = np.stack([WC.true_hint(c, rng) for c in nodes])
    res = level_batch.warm_nodes_host(_abi(nodes), nodes[0]["w"], hints)
    assert res["accepted"].all(), [c["family"] for c, a in zip(nodes, res["accepted"]) if not a]
    assert np.all(res["status"] == 1) and np.all(res["pivots"] == 0)
    truths = [SC.truth(c) for c in nodes]
    ref = SC.oracle_solve(oracle, nodes, nodes[0]["w"])
    e_ref = {}
    for c, (zt, info), zo in zip(nodes, truths, ref["z"]):
        e_ref[c["family"]] = max(e_ref.get(c["family"], 0.0), SR.node_error(zo, zt, n, SC.row_norm(c)))
    for c, (zt, info), z in zip(nodes, truths, res["z"]):
        assert np.array_equal(WC.sides_of(z, n), c["side"]), c["family"]
        assert info["ok"], (c["family"], info["why"])                # the certificate on the set the point claims
    fails = SC.check_against_truth(nodes, truths, res, f"twin ({n},{m})", {}, e_ref)
    assert not fails, "\n".join(fails)
    # the residual the twin reports is the post-check's, below its tolerance
    assert np.all(res["resid"] <= 1e-6)


@pytest.mark.parametrize("kind", WC.WRONG)
def test_wrong_hints_are_declined(kind):
    seen = 0
    for n, m in WC.SHAPES:
        nodes = WC.shape_nodes(n, m)
        rng = np.random.default_rng([2, n, m, WC.WRONG.index(kind)])
        pairs = [(c, WC.wrong_hint(c, kind, rng)) for c in nodes]
        pairs = [(c, z) for c, z in pairs if z is not None]
        if not pairs:
            continue
        sub = [c for c, _ in pairs]
        hints = np.stack([z for _, z in pairs])
        res = level_batch.warm_nodes_host(_abi(sub), sub[0]["w"], hints)
        assert not res["accepted"].any(), (kind, n, m, [c["family"] for c, a in zip(sub, res["accepted"]) if a])
        # a declined node keeps what came in
        assert np.array_equal(res["z"], hints, equal_nan=True) and np.all(res["status"] == 0) and np.all(res["pivots"] == -1)
        seen += len(sub)
    assert seen >= 10, (kind, seen)                       # every kind of wrong hint exists on some shapes


def test_mixed_batch_node_by_node():
    n, m = 17, 32
    nodes = WC.shape_nodes(n, m)
    rng = np.random.default_rng(3)
    wrong = [i % 2 == 1 for i in range(len(nodes))]
    hints = np.stack([WC.wrong_hint(c, "nan", rng) if bad else WC.true_hint(c, rng) for c, bad in zip(nodes, wrong)])
    res = level_batch.warm_nodes_host(_abi(nodes), nodes[0]["w"], hints)
    assert np.array_equal(res["accepted"], ~np.array(wrong))


# ---- the route switch of solve_level ---------------------------------------------------------------------------------------------
class _SpyHandle:
    """A resident handle served by the oracle (cold) and the twin (warm): Nodes.solve's interface, with a log."""

    def __init__(self, eng, records):
        self.eng, self.records = eng, [np.array(a) for a in records]
        self.batch, self.n = self.records[2].shape
        self.m = self.records[5].shape[1]

    def verify(self, xd, w, tol=1e-4):
        return OracleEngine.verify_nodes(self.eng, *self.records, xd, w, tol=tol)

    def solve(self, w, opts=None, want=("z", "resid", "pivots", "active"), out=None, x_out=None, warm=None):
        flags = opts.flags if opts is not None else 0
        if warm is not None:
            flags |= _lib.AVI_FLAG_WARM_DUALS
        self.eng.sweeps.append(dict(n=self.n, m=self.m, batch=self.batch, flags=flags,
                                    warm=None if warm is None else np.array(warm), in_place=warm is not None and out is not None
                                    and warm is out["z"]))
        cold = OracleEngine.solve_nodes(self.eng, *self.records, w)
        res = {k: np.array(cold[k]) for k in ("z", "status", "resid", "pivots")}
        if warm is not None:
            got = level_batch.warm_nodes_host(self.records, w, warm)
            acc = got["accepted"]
            for k in res:
                res[k][acc] = got[k][acc]
            self.eng.accepted.append(int(acc.sum()))
        self.eng.sweeps[-1]["z_out"] = res["z"].copy()
        if out is None:
            out = {}
        out.update(res)
        return out


class _SpyEngine(OracleEngine):
    def __init__(self):
        super().__init__()
        self.sweeps, self.accepted, self.uploads, self.plain = [], [], 0, 0

    def upload_nodes(self, *records):
        self.uploads += 1
        return _SpyHandle(self, records)

    def solve_nodes(self, *a, **k):
        self.plain += 1
        assert "opts" not in k or k["opts"] is None                  # inner nodes stay cold
        return OracleEngine.solve_nodes(self, *a, **k)


def _sweeps(route):
    """Three sweeps of the followers (childless, resident) of a two-level net, the leaders' variables moved a little in between
    as the outer loop moves them, then one sweep of the leaders under their children's first pieces."""
    import parent_cases as PC
    net, x, S = PC.kinked_pairs()
    followers, leaders = sorted(net.network_depth_map[2]), sorted(net.network_depth_map[1])
    rng = np.random.default_rng(4)
    level_batch.WARM_DUALS_ROUTE = route
    try:
        e = _SpyEngine()
        xs = []
        for t in range(3):
            x = level_batch.solve_level(net, followers, x + (1e-4 * rng.standard_normal(x.size) if t else 0.0), engine=e)
            xs.append(x)
        xs.append(level_batch.solve_level(net, leaders, x, {j: S[j][0] for j in S}, engine=e))
    finally:
        level_batch.WARM_DUALS_ROUTE = False
    return xs, e


def test_route_passes_the_previous_z_for_resident_leaf_batches_only():
    assert level_batch.WARM_DUALS_ROUTE is False
    off, e0 = _sweeps(False)
    on, e1 = _sweeps(True)
    # off: no sweep carries a hint or the flag -- the calls of the code as it was
    assert len(e0.sweeps) >= 3 and all(s["warm"] is None and s["flags"] == 0 for s in e0.sweeps)
    # on: the same calls; the first sweep of a handle is cold, every later one carries the z of the sweep before it, in place,
    # with the flag
    assert e1.uploads == e0.uploads and len(e1.sweeps) == len(e0.sweeps)
    last = {}
    for s in e1.sweeps:
        key = (s["n"], s["m"], s["batch"])
        if key not in last:
            assert s["warm"] is None and s["flags"] == 0
        else:
            assert s["warm"] is not None and s["in_place"] and s["flags"] & _lib.AVI_FLAG_WARM_DUALS
            assert np.array_equal(s["warm"], last[key]["z_out"])
        last[key] = s
    # the nodes with children (the leaders) went through solve_nodes, without options, as often as with the route off
    assert e1.plain == e0.plain > 0
    # the small moves leave most followers' active sets alone (the net has a follower at a kink, whose multiplier is a rounding
    # error of either sign): hints held in every warm sweep, and the sweeps end where the cold ones end
    assert len(e1.accepted) == len(e1.sweeps) - 1 and all(0 < a <= s["batch"] for a, s in zip(e1.accepted, e1.sweeps[1:]))
    for a, b in zip(on, off):
        assert np.max(np.abs(a - b)) <= 1e-9
