"""Crash cache of resident symmetric n = m = 32 records (QPN_OPT_CRASH_CACHE): the first sweep over a handle stores what Stage A
of the fused kernel makes of Qd and Ad alone, the later sweeps reuse it.  The cached sweeps run the parameter-dependent
operations in the same order on the same numbers, so every output is IDENTICAL -- array_equal, not close -- to

  * the first sweep of a fresh handle given the same w (that sweep cannot have used a cache), and
  * a handle swept with QPN_OPT_CRASH_CACHE = 0,

for shared and per-node parameters, host and device callers, batches below and above one resident round (4 096), nodes that
decline for either reason (they keep being re-solved by the general kernel), and across qpn_nodes_update: Qd / Ad drop the
cache, R / qd / B / l / u keep it.  Other shapes and asymmetric records are not cached and give what they gave."""
import numpy as np
import pytest

import problems as P

pytestmark = pytest.mark.gpu

KEYS = ("z", "status", "resid", "pivots", "active")


def _records(seed, cnt, n=32, m=32, p=8, declines=True):
    """Column-major records as the ABI takes them.  With `declines`, node 3 fails the pivot test (its first pivot is 1e-6 against
    the 1e-4 max |M| threshold; Qd stays symmetric and positive definite) and node 5 has an equality row (l == u)."""
    from qpn_amd.engine import colmajor
    Q, R, qd, A, B, l, u = P.synth_nodes(seed, cnt, n, m, p)
    B = np.random.default_rng(seed).standard_normal((cnt, m, p)) * 0.1
    Q, l, u = Q.copy(), l.copy(), u.copy()
    if declines:
        Q[3, 0, :] = 0.0; Q[3, :, 0] = 0.0; Q[3, 0, 0] = 1e-6
        u[5, 2] = l[5, 2]
    return [colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u]


def _np(res):
    return {k: np.array(v.cpu() if hasattr(v, "cpu") else v) for k, v in res.items() if v is not None}


def _solve(nodes, w, n=32, device=False):
    """One sweep with every output, the primal blocks into an iterate of their own as well; host arrays or device tensors."""
    if device:
        import torch
        wd = torch.tensor(np.ascontiguousarray(w), dtype=torch.float64, device="cuda:0")
        x = torch.zeros((nodes.batch, n + 3), dtype=torch.float64, device="cuda:0")
        out = _np(nodes.solve(wd, x_out=x))
        torch.cuda.synchronize()
        out["x_out"] = x.cpu().numpy()
    else:
        x = np.zeros((nodes.batch, n + 3))
        out = _np(nodes.solve(w, x_out=x))
        out["x_out"] = x
    return out


def _assert_identical(a, b, what):
    for k in KEYS + ("x_out",):
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k} differs"


class _option:
    def __init__(self, engine, opt, value, back):
        self.engine, self.opt, self.value, self.back = engine, opt, value, back

    def __enter__(self):
        self.engine.set_option(self.opt, self.value)

    def __exit__(self, *exc):
        self.engine.set_option(self.opt, self.back)


def _uncached(engine):
    from qpn_amd import _lib
    return _option(engine, _lib.OPT_CRASH_CACHE, 0, 1)


def _fresh_first_sweep(engine, abi, w, device=False):
    nodes = engine.upload_nodes(*abi)
    assert not nodes.info()["crash_cached"]
    out = _solve(nodes, w, abi[2].shape[1], device)
    declined = None
    engine.synchronize()
    info = nodes.info()
    if info["decline_state"] >= 2:
        declined = info["declined"]
    nodes.close()
    return out, declined


@pytest.mark.parametrize("cnt", [96, 4500])
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("per_node_w", [False, True])
def test_cached_sweeps_are_identical_to_uncached_ones(engine, cnt, device, per_node_w):
    abi = _records(101 + cnt, cnt)
    nodes = engine.upload_nodes(*abi)
    off = engine.upload_nodes(*abi)
    info = nodes.info()
    assert info["symmetric"] and not info["crash_cached"] and not info["crash_refused"]
    rng = np.random.default_rng(7)
    for sweep in range(6):
        w = rng.standard_normal((cnt, 8)) if per_node_w else rng.standard_normal(8)
        a = _solve(nodes, w, device=device)
        info = nodes.info()
        assert info["crash_cached"] and not info["crash_refused"]      # from the first sweep on
        ref, ref_declined = _fresh_first_sweep(engine, abi, w, device)
        _assert_identical(a, ref, f"sweep {sweep} against a fresh handle's first sweep")
        with _uncached(engine):
            b = _solve(off, w, device=device)
            io = off.info()
            assert not io["crash_cached"] and io["crash_refused"]
        _assert_identical(a, b, f"sweep {sweep} against QPN_OPT_CRASH_CACHE = 0")
        # both declining nodes went to the general kernel and came back solved or flagged by it, never as -1
        assert a["status"][3] != -1 and a["status"][5] != -1
        assert int(np.sum(a["status"] == 1)) >= cnt - 2
    engine.synchronize()
    info, io = nodes.info(), off.info()
    assert info["decline_state"] == 3 and info["declined"] == 2
    assert io["decline_state"] == 3 and io["declined"] == 2
    assert ref_declined in (None, 2)
    nodes.close(); off.close()


def test_no_declines_means_one_launch_with_and_without_the_cache(engine):
    cnt = 300
    abi = _records(55, cnt, declines=False)
    nodes = engine.upload_nodes(*abi)
    rng = np.random.default_rng(3)
    for sweep in range(5):
        w = rng.standard_normal(8)
        a = _solve(nodes, w)
        ref, _ = _fresh_first_sweep(engine, abi, w)
        _assert_identical(a, ref, f"sweep {sweep}")
        assert np.all(a["status"] == 1)
    engine.synchronize()
    info = nodes.info()
    assert info["decline_state"] == 2 and info["declined"] == 0 and info["crash_cached"]
    nodes.close()


@pytest.mark.parametrize("field", ["Qd", "Ad", "l", "u", "R", "qd", "B"])
def test_update_drops_the_cache_exactly_when_qd_or_ad_change(engine, field):
    cnt = 200
    abi = _records(61, cnt)
    abi2 = _records(62, cnt)                      # another set of records: the source of the replaced field
    idx = dict(Qd=0, R=1, qd=2, Ad=3, B=4, l=5, u=6)[field]
    new = list(abi)
    new[idx] = abi2[idx]
    if field == "l":                              # keep l <= u
        new[5] = np.minimum(abi2[5], abi[6])
    if field == "u":
        new[6] = np.maximum(abi2[6], abi[5])
    nodes = engine.upload_nodes(*abi)
    rng = np.random.default_rng(9)
    w = rng.standard_normal(8)
    _solve(nodes, w); _solve(nodes, w)
    assert nodes.info()["crash_cached"]
    nodes.update(field, new[idx])
    info = nodes.info()
    assert info["crash_cached"] == (field not in ("Qd", "Ad")), info
    assert not info["crash_refused"]
    for sweep in range(3):
        w = rng.standard_normal(8)
        a = _solve(nodes, w)
        ref, _ = _fresh_first_sweep(engine, new, w)
        _assert_identical(a, ref, f"after update({field}), sweep {sweep}")
        assert nodes.info()["crash_cached"]
    nodes.close()


def test_sym_route_change_drops_the_cache_and_results_stay(engine):
    from qpn_amd import _lib
    cnt = 128
    abi = _records(71, cnt)
    nodes = engine.upload_nodes(*abi)
    w = np.random.default_rng(1).standard_normal(8)
    a0 = _solve(nodes, w); a1 = _solve(nodes, w)
    _assert_identical(a0, a1, "second sweep")
    with _option(engine, _lib.OPT_SYM_ROUTE, 0, 1):
        g = _solve(nodes, w)
        info = nodes.info()
        assert not info["crash_cached"] and info["crash_refused"]
        per_call = _np(engine.solve_nodes(*abi, w))
        for k in KEYS:
            assert np.array_equal(g[k], per_call[k]), k                # the general variants, as ever
    assert not nodes.info()["crash_cached"]                            # dropped: filled again by the next sweep
    a2 = _solve(nodes, w)
    assert nodes.info()["crash_cached"]
    a3 = _solve(nodes, w)
    _assert_identical(a0, a2, "refilled"); _assert_identical(a0, a3, "reused after the refill")
    nodes.close()


def test_asymmetric_records_are_not_cached_and_equal_the_per_call_route(engine):
    from qpn_amd.engine import colmajor
    cnt = 150
    abi = _records(81, cnt, declines=False)
    K = np.random.default_rng(77).standard_normal((cnt, 32, 32)) * 0.05
    abi[0] = np.ascontiguousarray(abi[0] + colmajor(K - K.transpose(0, 2, 1)))
    nodes = engine.upload_nodes(*abi)
    assert not nodes.info()["symmetric"]
    rng = np.random.default_rng(5)
    for sweep in range(3):
        w = rng.standard_normal(8)
        a = _np(nodes.solve(w))
        b = _np(engine.solve_nodes(*abi, w))
        for k in KEYS:
            assert np.array_equal(a[k], b[k]), k
        info = nodes.info()
        assert not info["crash_cached"] and info["crash_refused"]
    nodes.close()


@pytest.mark.parametrize("n,m", [(16, 16), (32, 24)])
def test_other_shapes_are_not_cached_and_unchanged(engine, n, m):
    cnt = 120
    abi = _records(91, cnt, n, m, declines=False)
    nodes = engine.upload_nodes(*abi)
    rng = np.random.default_rng(6)
    for sweep in range(3):
        w = rng.standard_normal(8)
        a = _solve(nodes, w, n)
        ref, _ = _fresh_first_sweep(engine, abi, w)
        _assert_identical(a, ref, f"sweep {sweep}")
        with _uncached(engine):
            b = _solve(nodes, w, n)
        _assert_identical(a, b, f"sweep {sweep}, option off")
        info = nodes.info()
        assert not info["crash_cached"] and info["crash_refused"]
    nodes.close()


def test_option_off_then_on_and_bad_values(engine):
    from qpn_amd import _lib
    from qpn_amd.engine import QpnError
    abi = _records(95, 64)
    nodes = engine.upload_nodes(*abi)
    w = np.random.default_rng(2).standard_normal(8)
    with _uncached(engine):
        a = _solve(nodes, w); _solve(nodes, w)
        assert not nodes.info()["crash_cached"] and nodes.info()["crash_refused"]
    b = _solve(nodes, w)
    assert nodes.info()["crash_cached"] and not nodes.info()["crash_refused"]
    c = _solve(nodes, w)
    _assert_identical(a, b, "fill sweep"); _assert_identical(a, c, "reuse sweep")
    with pytest.raises(QpnError):
        engine.set_option(_lib.OPT_CRASH_CACHE, 2)
    nodes.close()
