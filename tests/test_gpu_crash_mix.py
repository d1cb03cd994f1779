"""Mixed reuse sweeps (crash cache valid, launches beyond one resident round): every wavefront picks one of the two Stage A
bodies of the fused symmetric n = m = 32 kernel -- reuse the cache, or compute and keep nothing -- by its position in the launch
(crash_mix_rule.py restates the rule).  Both give the same bits, so every output of every sweep is IDENTICAL -- array_equal --
to the same sweep of a handle with QPN_OPT_CRASH_CACHE = 0 and to the first sweep of a fresh handle, with the longest-first
schedule on (its re-sorts move nodes between the two kinds of position) and in natural order, for shared and per-node
parameters, host and device callers; nodes that decline do so from either kind of position and come back from the general
kernel; an update of Qd refills the cache and the sweeps after it are identical again."""
import numpy as np
import pytest

import crash_mix_rule as rule
import problems as P

pytestmark = pytest.mark.gpu

KEYS = ("z", "status", "resid", "pivots", "active", "x_out")
SIZES = (4500, 10000, 12289)
_cache = {}


def _base(cnt):
    """Plain records (no declining node), made once per size."""
    if cnt not in _cache:
        Q, R, qd, A, B, l, u = P.synth_nodes(300 + cnt, cnt, 32, 32, 8)
        B = np.random.default_rng(cnt).standard_normal((cnt, 32, 8)) * 0.1
        _cache[cnt] = (Q, R, qd, A, B, l, u)
    return _cache[cnt]


def _records(cnt, bad_pivot, equality):
    """Column-major records as the ABI takes them: node `bad_pivot` fails the pivot test (its first pivot is 1e-6 against the
    1e-4 max |M| threshold; Qd stays symmetric and positive definite), node `equality` has an equality row (l == u)."""
    from qpn_amd.engine import colmajor
    Q, R, qd, A, B, l, u = _base(cnt)
    Q, l, u = Q.copy(), l.copy(), u.copy()
    Q[bad_pivot, 0, :] = 0.0; Q[bad_pivot, :, 0] = 0.0; Q[bad_pivot, 0, 0] = 1e-6
    u[equality, 2] = l[equality, 2]
    return [colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u]


def _np(res):
    return {k: np.array(v.cpu() if hasattr(v, "cpu") else v) for k, v in res.items() if v is not None}


def _solve(nodes, w, device):
    if device:
        import torch
        wd = torch.tensor(np.ascontiguousarray(w), dtype=torch.float64, device="cuda:0")
        x = torch.zeros((nodes.batch, 35), dtype=torch.float64, device="cuda:0")
        out = _np(nodes.solve(wd, x_out=x))
        torch.cuda.synchronize()
        out["x_out"] = x.cpu().numpy()
    else:
        x = np.zeros((nodes.batch, 35))
        out = _np(nodes.solve(w, x_out=x))
        out["x_out"] = x
    return out


def _same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k} differs"


class _uncached:
    def __init__(self, engine):
        self.engine = engine

    def __enter__(self):
        from qpn_amd import _lib
        self.engine.set_option(_lib.OPT_CRASH_CACHE, 0)

    def __exit__(self, *exc):
        from qpn_amd import _lib
        self.engine.set_option(_lib.OPT_CRASH_CACHE, 1)


def _fresh(engine, abi, w, device, period):
    nodes = engine.upload_nodes(*abi)
    nodes.set_schedule(period)
    out = _solve(nodes, w, device)
    nodes.close()
    return out


def _positions(cnt):
    """One computing and one reusing launch position of a natural-order sweep, twice (for the two declining nodes)."""
    from_ = rule.reuse_from(cnt)
    comp = [p for p in range(16, from_) if rule.recomputes(p, rule.SHARE, from_)]
    reus = [p for p in range(16, from_) if not rule.recomputes(p, rule.SHARE, from_)]
    return comp, reus


def test_the_build_mixes():
    """These tests need a build whose share is above 0 -- else every launch is a plain reuse sweep and they show nothing."""
    assert rule.SHARE > 0
    for cnt in SIZES:
        assert rule.mixed(cnt)
        comp, reus = _positions(cnt)
        assert len(comp) >= 2 and len(reus) >= 2


def _sweeps(engine, cnt, device, per_node_w, period, count, bad_pivot, equality, seed):
    abi = _records(cnt, bad_pivot, equality)
    nodes = engine.upload_nodes(*abi)
    off = engine.upload_nodes(*abi)
    nodes.set_schedule(period); off.set_schedule(period)
    rng = np.random.default_rng(seed)
    for sweep in range(count):
        w = rng.standard_normal((cnt, 8)) if per_node_w else rng.standard_normal(8)
        a = _solve(nodes, w, device)
        info = nodes.info()
        assert info["crash_cached"] and not info["crash_refused"]
        with _uncached(engine):
            b = _solve(off, w, device)
            io = off.info()
            assert not io["crash_cached"] and io["crash_refused"]
        _same(a, b, f"sweep {sweep} against QPN_OPT_CRASH_CACHE = 0")
        _same(a, _fresh(engine, abi, w, device, period), f"sweep {sweep} against a fresh handle's first sweep")
        # both declining nodes went to the general kernel and came back from it, never as -1
        assert a["status"][bad_pivot] != -1 and a["status"][equality] != -1
        assert int(np.sum(a["status"] == 1)) >= cnt - 2
    engine.synchronize()
    info = nodes.info()
    assert info["decline_state"] == 3 and info["declined"] == 2 and info["crash_cached"]
    return nodes, off, abi, rng


@pytest.mark.parametrize("cnt", SIZES)
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("per_node_w", [False, True])
def test_scheduled_sweeps_are_identical(engine, cnt, device, per_node_w):
    nodes, off, _, _ = _sweeps(engine, cnt, device, per_node_w, 16, 40, 3, 5, 11 + cnt)
    assert nodes.info()["scheduled"]
    nodes.close(); off.close()


@pytest.mark.parametrize("cnt", SIZES)
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("per_node_w", [False, True])
@pytest.mark.parametrize("bad_on", ["computing", "reusing"])
def test_natural_order_sweeps_and_declines_from_both_kinds_of_position(engine, cnt, device, per_node_w, bad_on):
    # natural order: launch position = node index
    comp, reus = _positions(cnt)
    bad_pivot, equality = (comp[0], reus[1]) if bad_on == "computing" else (reus[0], comp[1])
    from_ = rule.reuse_from(cnt)
    assert rule.recomputes(bad_pivot, rule.SHARE, from_) == (bad_on == "computing")
    assert rule.recomputes(equality, rule.SHARE, from_) == (bad_on != "computing")
    nodes, off, _, _ = _sweeps(engine, cnt, device, per_node_w, 0, 4, bad_pivot, equality, 23 + cnt)
    assert not nodes.info()["scheduled"]
    nodes.close(); off.close()


@pytest.mark.parametrize("cnt", [10000])
@pytest.mark.parametrize("period", [0, 16])
def test_update_of_qd_refills_the_cache_and_the_sweeps_stay_identical(engine, cnt, period):
    from qpn_amd.engine import colmajor
    comp, reus = _positions(cnt)
    nodes, off, abi, rng = _sweeps(engine, cnt, False, False, period, 3, comp[0], reus[1], 5)
    # another Qd for one node on a computing and one on a reusing position (symmetric, positive definite)
    Qc = abi[0].copy()
    for node in (comp[2], reus[2]):
        Qc[node] = Qc[node] * 1.25
    new = list(abi); new[0] = Qc
    nodes.update("Qd", Qc); off.update("Qd", Qc)
    assert not nodes.info()["crash_cached"]
    for sweep in range(4):
        w = rng.standard_normal(8)
        a = _solve(nodes, w, False)
        assert nodes.info()["crash_cached"]                        # refilled by the first sweep after the update
        with _uncached(engine):
            b = _solve(off, w, False)
        _same(a, b, f"after the update, sweep {sweep} against QPN_OPT_CRASH_CACHE = 0")
        _same(a, _fresh(engine, new, w, False, period), f"after the update, sweep {sweep} against a fresh handle")
    nodes.close(); off.close()
