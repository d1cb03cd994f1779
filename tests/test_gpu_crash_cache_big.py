"""Crash cache of resident LARGE records (QPN_OPT_CRASH_CACHE_BIG; 64 < n <= 256, m <= 256: the blocked crash of
csrc/qpn_avi_schur_big2.hip).  The first sweep over a handle keeps what the elimination makes of Qd and Ad alone (the
multipliers of every rank-64 pass, W, S, the smallest pivot, max |M| over H and C); later sweeps replay the one column that
moves with w (csrc/qpn_crash_big.hip).  Every output of every sweep is IDENTICAL -- array_equal, not close -- to

  * a second handle swept with the option at 0, and
  * the first sweep of a fresh handle given the same w,

for shared and per-node w, host and device callers, symmetric records (block principal pivoting) and asymmetric ones or a
caller-set pivot budget (the Lemke kernel alone, which works on a private copy of S), nodes that decline for either reason, a
pivot threshold that moves with qd, and across qpn_nodes_update.  Shapes outside the class, and records passed per call, are
not cached and give what they gave.

Shapes (n, m, p): (144, 16, 4) records route, three passes, a last block one tile wide, one constraint tile; (129, 40, 3) the
conversion route, padding on both sides; (80, 144, 4) a 4-tile then a 1-tile block, m > 128; (192, 192, 8) three full passes;
(256, 256, 8) four."""
import numpy as np
import pytest

import problems as P

pytestmark = pytest.mark.gpu

KEYS = ("z", "status", "resid", "pivots", "active")
SHAPES = [(144, 16, 4), (129, 40, 3), (80, 144, 4), (192, 192, 8), (256, 256, 8)]
SWEEPS = 6


def _records(seed, cnt, n, m, p, asym=False, declines=False, big_q=()):
    """Column-major records as the ABI takes them.  asym: a skew part on every Qd (the handle is not symmetric: Stage B is the
    Lemke kernel alone).  declines: node 1 has a singular leading Qd block (a pivot of 0 in the first pass; the bounds keep the
    node well-posed) and node 2 an equality row.  big_q: nodes whose Qd is 1e4 times the usual."""
    from qpn_amd.engine import colmajor
    Q, R, qd, A, B, l, u = P.synth_nodes(seed, cnt, n, m, p)
    B = np.random.default_rng(seed).standard_normal((cnt, m, p)) * 0.1
    Q, A, l, u = Q.copy(), A.copy(), l.copy(), u.copy()
    if asym:
        K = np.random.default_rng(seed + 1).standard_normal((cnt, n, n)) * 0.02
        Q = Q + (K - K.transpose(0, 2, 1))
    if declines:
        Q[1, :3, :] = 0.0; Q[1, :, :3] = 0.0
        A[1, :3, :] = 0.0; A[1, 0, 0] = 1.0; A[1, 1, 1] = 1.0; A[1, 2, 2] = 1.0
        l[1, :3] = -0.5; u[1, :3] = 0.5
        u[2, 5] = l[2, 5]
    for k in big_q:
        Q[k] *= 1e4
    return [colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u]


def _np(res):
    return {k: np.array(v.cpu() if hasattr(v, "cpu") else v) for k, v in res.items() if v is not None}


def _solve(nodes, w, device=False, opts=None):
    """One sweep with every output, the primal blocks into an iterate of their own as well; host arrays or device tensors."""
    n = nodes.n
    if device:
        import torch
        wd = torch.tensor(np.ascontiguousarray(w), dtype=torch.float64, device="cuda:0")
        x = torch.zeros((nodes.batch, n + 3), dtype=torch.float64, device="cuda:0")
        out = _np(nodes.solve(wd, opts=opts, x_out=x))
        torch.cuda.synchronize()
        out["x_out"] = x.cpu().numpy()
    else:
        x = np.zeros((nodes.batch, n + 3))
        out = _np(nodes.solve(w, opts=opts, x_out=x))
        out["x_out"] = x
    return out


def _assert_identical(a, b, what):
    for k in KEYS + ("x_out",):
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{what}: {k} differs"


class _uncached:
    def __init__(self, engine):
        self.engine = engine

    def __enter__(self):
        from qpn_amd import _lib
        self.engine.set_option(_lib.OPT_CRASH_CACHE_BIG, 0)

    def __exit__(self, *exc):
        from qpn_amd import _lib
        self.engine.set_option(_lib.OPT_CRASH_CACHE_BIG, 1)


@pytest.fixture
def big(engine):
    """Every case sets the option first (and leaves the default behind)."""
    from qpn_amd import _lib
    engine.set_option(_lib.OPT_CRASH_CACHE_BIG, 1)
    try:
        yield engine
    finally:
        engine.set_option(_lib.OPT_CRASH_CACHE_BIG, 0)


def _fresh_first_sweep(engine, abi, w, device=False, opts=None):
    nodes = engine.upload_nodes(*abi)
    assert not nodes.info()["big_cached"]
    out = _solve(nodes, w, device, opts)
    nodes.close()
    return out


def _check_sweep(engine, nodes, off, abi, w, what, device=False, opts=None, cached=True):
    """One sweep of the cached handle against the option-0 handle and a fresh handle's first sweep."""
    a = _solve(nodes, w, device, opts)
    info = nodes.info()
    assert info["big_cached"] == cached and not info["big_refused"], (what, info)
    with _uncached(engine):
        b = _solve(off, w, device, opts)
        io = off.info()
        assert not io["big_cached"] and io["big_refused"], (what, io)
    _assert_identical(a, b, f"{what} against QPN_OPT_CRASH_CACHE_BIG = 0")
    _assert_identical(a, _fresh_first_sweep(engine, abi, w, device, opts), f"{what} against a fresh handle's first sweep")
    return a


def _w(rng, cnt, p, per_node):
    return rng.standard_normal((cnt, p)) if per_node else rng.standard_normal(p)


CASES = [(s, d) for s in SHAPES for d in ([False, True] if s in (SHAPES[0], SHAPES[-1]) else [False])]


@pytest.mark.parametrize("shape,device", CASES)
@pytest.mark.parametrize("per_node_w", [False, True])
def test_cached_sweeps_are_identical_to_uncached_ones(big, shape, device, per_node_w):
    n, m, p = shape
    cnt = 6
    abi = _records(300 + n + m, cnt, n, m, p)
    nodes, off = big.upload_nodes(*abi), big.upload_nodes(*abi)
    info = nodes.info()
    assert info["symmetric"] and not info["big_cached"] and not info["big_refused"]
    rng = np.random.default_rng(7)
    for sweep in range(SWEEPS):
        a = _check_sweep(big, nodes, off, abi, _w(rng, cnt, p, per_node_w), f"sweep {sweep}", device)
        assert np.all(a["status"] == 1) and np.max(a["resid"]) <= 1e-8          # (two failures cannot agree)
    nodes.close(); off.close()


@pytest.mark.parametrize("shape", [(144, 16, 4), (192, 192, 8)])
def test_lemke_sweeps_leave_the_cached_s_alone(big, shape):
    """Symmetric records: sweeps under a caller-set pivot budget send every node through the Lemke kernel, which folds its
    pivots into the dictionary in place; the sweeps between them are block principal pivoting on the cached S."""
    n, m, p = shape
    cnt = 6
    abi = _records(400 + n, cnt, n, m, p)
    nodes, off = big.upload_nodes(*abi), big.upload_nodes(*abi)
    lemke = big.default_opts()
    lemke.max_pivots = 1000000
    rng = np.random.default_rng(11)
    for sweep in range(SWEEPS):
        opts = lemke if sweep % 2 == 0 else None
        a = _check_sweep(big, nodes, off, abi, _w(rng, cnt, p, sweep >= 3), f"sweep {sweep}", opts=opts)
        assert np.all(a["status"] == 1) and np.max(a["resid"]) <= 1e-8
    nodes.close(); off.close()


@pytest.mark.parametrize("shape", [(129, 40, 3), (256, 256, 8)])
def test_asymmetric_records_take_the_lemke_kernel_on_a_copy(big, shape):
    n, m, p = shape
    cnt = 6
    abi = _records(500 + n, cnt, n, m, p, asym=True)
    nodes, off = big.upload_nodes(*abi), big.upload_nodes(*abi)
    assert not nodes.info()["symmetric"]
    rng = np.random.default_rng(13)
    for sweep in range(SWEEPS):
        a = _check_sweep(big, nodes, off, abi, _w(rng, cnt, p, sweep % 2 == 1), f"sweep {sweep}")
        assert np.all(a["status"] == 1) and np.max(a["resid"]) <= 1e-8
    nodes.close(); off.close()


@pytest.mark.parametrize("shape", [(144, 16, 4), (80, 144, 4)])
def test_planted_decliners_stay_with_the_uncached_route(big, shape):
    n, m, p = shape
    cnt = 8
    abi = _records(600 + n, cnt, n, m, p, declines=True)
    nodes, off = big.upload_nodes(*abi), big.upload_nodes(*abi)
    rng = np.random.default_rng(17)
    for sweep in range(SWEEPS):
        a = _check_sweep(big, nodes, off, abi, _w(rng, cnt, p, sweep % 2 == 1), f"sweep {sweep}")
        assert a["status"][1] != -1 and a["status"][2] != -1      # the general kernel took both
        rest = np.delete(np.arange(cnt), [1, 2])
        assert np.all(a["status"][rest] == 1) and np.max(a["resid"][rest]) <= 1e-8
    nodes.close(); off.close()


def _lu_pivots_min(Q):
    """Smallest |pivot| of the elimination of Q without pivoting (the block pivots' diagonal tiles are eliminated this way)."""
    U = np.array(Q, dtype=np.float64)
    piv = np.inf
    for k in range(U.shape[0]):
        piv = min(piv, abs(U[k, k]))
        U[k + 1:, k:] -= np.outer(U[k + 1:, k] / U[k, k], U[k, k:])
    return piv


def test_the_threshold_moves_with_qd(big):
    """1e-4 max(1, max |M|) takes in g = qd + R w.  Nodes 1, 3, 5 carry 1e4 x the usual Qd.  With qd at 1e5 times itself the
    threshold passes the pivots of the ordinary nodes (they decline) and stays below those of the scaled ones; the cache stays
    installed, and every sweep equals the uncached one -- the general kernel's answers for the decliners included."""
    from qpn_amd.engine import colmajor
    n, m, p = 192, 192, 8
    cnt = 6
    abi = _records(700, cnt, n, m, p, big_q=(1, 3, 5))
    nodes, off = big.upload_nodes(*abi), big.upload_nodes(*abi)
    rng = np.random.default_rng(19)
    ws = [rng.standard_normal(p) for _ in range(6)]
    # the numpy maxima: which nodes the blocked crash declines, before and after the update
    Q, R = colmajor(abi[0]), colmajor(abi[1])               # (back to the math layout)
    mhc = np.maximum(np.abs(abi[0]).reshape(cnt, -1).max(axis=1), np.abs(abi[3]).reshape(cnt, -1).max(axis=1))
    pmin = np.array([_lu_pivots_min(Q[k]) for k in range(cnt)])

    def declined(qd, w):
        g = qd + R @ w
        thr = 1e-4 * np.maximum(1.0, np.maximum(mhc, np.abs(g).max(axis=1)))
        assert np.all(np.abs(pmin / thr - 1.0) > 0.5)          # (no node anywhere near its threshold: rounding decides nothing)
        return pmin < thr

    qd0, qd1 = abi[2], 1e5 * abi[2]
    # (the natural-map residual is an absolute figure, linear in the scale of M: 1e-8 for the usual records, 1e4 x that for
    # the nodes whose Qd is 1e4 x the usual)
    rtol = 1e-8 * np.array([1.0, 1e4] * 3)
    for w in ws[:2]:
        assert not declined(qd0, w).any()
    for w in ws[2:4]:
        d = declined(qd1, w)
        assert d.any() and not d.all() and np.array_equal(d, np.array([True, False] * 3))
    for sweep in range(2):
        a = _check_sweep(big, nodes, off, abi, ws[sweep], f"sweep {sweep}")
        assert np.all(a["status"] == 1) and np.all(a["resid"] <= rtol)
    abi1 = list(abi); abi1[2] = qd1
    nodes.update("qd", qd1); off.update("qd", qd1)
    assert nodes.info()["big_cached"]
    for sweep in range(2, 4):
        a = _check_sweep(big, nodes, off, abi1, ws[sweep], f"sweep {sweep}, qd x 1e5")
        assert np.all(a["status"] != -1)
    nodes.update("qd", qd0); off.update("qd", qd0)
    assert nodes.info()["big_cached"]
    for sweep in range(4, 6):
        a = _check_sweep(big, nodes, off, abi, ws[sweep], f"sweep {sweep}, qd back")
        assert np.all(a["status"] == 1) and np.all(a["resid"] <= rtol)
    nodes.close(); off.close()


@pytest.mark.parametrize("field", ["Qd", "Ad", "l", "u", "R", "qd", "B"])
def test_update_drops_the_cache_exactly_when_qd_or_ad_change(big, field):
    n, m, p = 144, 16, 4
    cnt = 6
    abi = _records(800, cnt, n, m, p)
    abi2 = _records(801, cnt, n, m, p)
    idx = dict(Qd=0, R=1, qd=2, Ad=3, B=4, l=5, u=6)[field]
    new = list(abi)
    new[idx] = abi2[idx]
    if field == "l":
        new[5] = np.minimum(abi2[5], abi[6])
    if field == "u":
        new[6] = np.maximum(abi2[6], abi[5])
    nodes, off = big.upload_nodes(*abi), big.upload_nodes(*abi)
    rng = np.random.default_rng(23)
    for sweep in range(2):
        _check_sweep(big, nodes, off, abi, rng.standard_normal(p), f"sweep {sweep}")
    nodes.update(field, new[idx]); off.update(field, new[idx])
    info = nodes.info()
    assert info["big_cached"] == (field not in ("Qd", "Ad")) and not info["big_refused"], info
    for sweep in range(3):
        a = _check_sweep(big, nodes, off, new, rng.standard_normal(p), f"after update({field}), sweep {sweep}")
        assert np.all(a["status"] == 1) and np.max(a["resid"]) <= 1e-8
    nodes.close(); off.close()


def test_an_update_that_makes_an_equality_row_declines_on_reuse_sweeps(big):
    n, m, p = 144, 16, 4
    cnt = 6
    abi = _records(810, cnt, n, m, p)
    nodes, off = big.upload_nodes(*abi), big.upload_nodes(*abi)
    rng = np.random.default_rng(29)
    for sweep in range(2):
        _check_sweep(big, nodes, off, abi, rng.standard_normal(p), f"sweep {sweep}")
    u2 = abi[6].copy()
    u2[4, 7] = abi[5][4, 7]
    new = list(abi); new[6] = u2
    nodes.update("u", u2); off.update("u", u2)
    assert nodes.info()["big_cached"]
    for sweep in range(3):
        a = _check_sweep(big, nodes, off, new, rng.standard_normal(p), f"equality row, sweep {sweep}")
        assert np.all(a["status"] != -1)
    nodes.update("u", abi[6]); off.update("u", abi[6])
    a = _check_sweep(big, nodes, off, abi, rng.standard_normal(p), "bounds back")
    assert np.all(a["status"] == 1)
    nodes.close(); off.close()


def test_a_caller_made_order_with_holes_fills_nothing(big):
    n, m, p = 144, 16, 4
    cnt = 6
    abi = _records(820, cnt, n, m, p)
    nodes, off = big.upload_nodes(*abi), big.upload_nodes(*abi)
    rng = np.random.default_rng(31)
    order = np.array([4, -1, 0, 99, 2, 1], dtype=np.int32)
    big.set_node_order(order)
    try:
        for sweep in range(2):
            w = rng.standard_normal(p)
            a = _solve(nodes, w)
            assert not nodes.info()["big_cached"]
            with _uncached(big):
                b = _solve(off, w)
            _assert_identical(a, b, f"ordered sweep {sweep}")
    finally:
        big.set_node_order(None)
    for sweep in range(2):
        _check_sweep(big, nodes, off, abi, rng.standard_normal(p), f"sweep {sweep}")
    big.set_node_order(order)
    try:
        w = rng.standard_normal(p)
        a = _solve(nodes, w)                      # reuses the valid cache
        assert nodes.info()["big_cached"]
        with _uncached(big):
            b = _solve(off, w)
        _assert_identical(a, b, "ordered sweep over a valid cache")
    finally:
        big.set_node_order(None)
    nodes.close(); off.close()


@pytest.mark.parametrize("n,m", [(32, 32), (96, 64)])
def test_other_shapes_are_refused_and_unchanged(big, n, m):
    cnt, p = 8, 4
    abi = _records(830, cnt, n, m, p)
    nodes = big.upload_nodes(*abi)
    rng = np.random.default_rng(37)
    for sweep in range(3):
        w = rng.standard_normal(p)
        a = _solve(nodes, w)
        info = nodes.info()
        assert not info["big_cached"] and info["big_refused"], info
        with _uncached(big):
            b = _solve(nodes, w)
        _assert_identical(a, b, f"sweep {sweep}")
    nodes.close()


def test_records_passed_per_call_are_never_cached(big):
    n, m, p = 256, 256, 8
    abi = _records(840, 4, n, m, p)
    rng = np.random.default_rng(41)
    for sweep in range(2):
        w = rng.standard_normal(p)
        a = _np(big.solve_nodes(*abi, w))
        with _uncached(big):
            b = _np(big.solve_nodes(*abi, w))
        for k in KEYS:
            assert np.array_equal(a[k], b[k]), k
        assert np.all(a["status"] == 1)


def test_option_off_on_off_and_bad_values(big):
    from qpn_amd import _lib
    from qpn_amd.engine import QpnError
    n, m, p = 144, 16, 4
    abi = _records(850, 6, n, m, p)
    nodes = big.upload_nodes(*abi)
    w = np.random.default_rng(2).standard_normal(p)
    with _uncached(big):
        a = _solve(nodes, w); _solve(nodes, w)
        assert not nodes.info()["big_cached"] and nodes.info()["big_refused"]
    b = _solve(nodes, w)
    assert nodes.info()["big_cached"] and not nodes.info()["big_refused"]
    c = _solve(nodes, w)
    with _uncached(big):
        d = _solve(nodes, w)
        assert not nodes.info()["big_cached"] and nodes.info()["big_refused"]
    e = _solve(nodes, w)
    for x, what in ((b, "fill sweep"), (c, "reuse sweep"), (d, "off again"), (e, "on again")):
        _assert_identical(a, x, what)
    with pytest.raises(QpnError):
        big.set_option(_lib.OPT_CRASH_CACHE_BIG, 2)
    nodes.close()
