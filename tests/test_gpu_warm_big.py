"""QPN_OPT_WARM_BIG on the GPU: block principal pivoting of large resident symmetric nodes seeded from the multipliers of the
incoming z (csrc/qpn_avi_schur_big.hip: schur_big_bpp<true>).  Four nodes per shape, the cases of
tests/warm_big_cases.py, numpy and torch.cuda callers, shared and per-node w.  The bars are tests/test_gpu_bpp.py's:
|z - z_oracle| <= 1e-9 max(1, max |z_oracle|), resid <= 1e-8, status and active masks equal to the CPU oracle's.

Taken:    1. true hints -- every node comes back with pivots == n (no pair switched) and meets the bars; the cold sweep switched
             pairs in at least one node; the in-place form warm = out["z"] gives the same arrays;
          2. w moved by a relative 1e-3 / 1e-1 -- the bars at the new w, fewer pairs switched over the batch than un-hinted.
Survived: 3. wrong hints (10 % of the rows redrawn, every finite-lower row at lower, all signs flipped) -- the bars; a seed above the
             rank of S (its first factorisation fails: the workgroup restarts cold) on loose records, where the cold start
             finishes by block pivoting -- the bars and the un-hinted call's pivots (no node left to the Lemke kernel that the
             un-hinted call keeps from it); the same seed at (70, 255) plain, where the cold start fails too -- the bars;
          4. dropped hints (more than 112 rows, zeros, NaNs, infinite sides only) -- every output bit for bit that of the same
             call without the flag.
Ignored:  5. option 0, QPN_OPT_SYM_ROUTE = 0, a pivot budget, asymmetric Qd, records per call, shape (96, 96) -- bit for bit.
Beside:   6. nodes that block principal pivoting cannot finish (rank-deficient S, more than 112 active rows, equality rows);
          7. QPN_OPT_CRASH_CACHE_BIG = 1: hinted reuse sweeps, and a hinted sweep that fills the cache."""
import ctypes

import numpy as np
import pytest

import problems as P
import warm_big_cases as C

pytestmark = pytest.mark.gpu

KEYS = ("z", "status", "resid", "pivots", "active")
_REF = {}


@pytest.fixture
def warm(engine):
    """Every case sets the option first and leaves the default behind."""
    from qpn_amd import _lib
    engine.set_option(_lib.OPT_WARM_BIG, 1)
    try:
        yield engine
    finally:
        engine.set_option(_lib.OPT_WARM_BIG, 0)
        engine.set_option(_lib.OPT_SYM_ROUTE, 1)
        engine.set_option(_lib.OPT_CRASH_CACHE_BIG, 0)


def _oracle(oracle, key, rec, w):
    """The CPU oracle's answer for a batch at w: computed once per key, read only."""
    if key not in _REF:
        M, q, lo, hi, kd = P.reduced_blocks(*rec, w)
        _REF[key] = oracle.solve_avi_batch(M, q, lo, hi, kind=kd)
        assert np.all(_REF[key]["status"] == 1)
    return _REF[key]


def _host(a):
    return a.cpu().numpy().copy() if hasattr(a, "cpu") else np.array(a)


def _up(dev):
    import torch
    return (lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()) if dev else (lambda a: np.array(a))


def _run(engine, src, w, z_in, flag, dev=False, max_pivots=0):
    """One sweep with z_in going in through z.  src: a Nodes handle, or the seven record arrays (per-call route).  flag = False
    is the SAME call without QPN_AVI_FLAG_WARM_DUALS: Nodes.solve would make a call that brings no hint a cold start, so that
    one is made at the ABI."""
    from qpn_amd import _lib
    from qpn_amd.engine import _ptr
    up = _up(dev)
    batch, N = z_in.shape
    o = engine.default_opts()
    o.max_pivots = max_pivots
    if flag:
        o.flags |= _lib.AVI_FLAG_WARM_DUALS
    wd = up(w)
    if isinstance(src, (list, tuple)):
        res = engine.solve_nodes(*[up(a) for a in src], wd, z0=up(z_in), opts=o)
    else:
        res = dict(z=up(z_in), status=up(np.zeros(batch, np.int32)), resid=up(np.zeros(batch)), pivots=up(np.zeros(batch, np.int32)),
                   active=up(np.zeros((batch, N), np.uint8)))
        if flag:
            src.solve(wd, opts=o, out=res)
        else:
            engine._bind_stream(dev)
            engine._call("qpn_solve_nodes_h", src.h, _ptr(wd), 0 if wd.ndim == 1 else wd.shape[1], _ptr(res["z"]), _ptr(res["status"]),
                         _ptr(res["resid"]), _ptr(res["pivots"]), _ptr(res["active"]), ctypes.byref(o), engine._mem(dev), None, 0)
    engine.synchronize()
    return {k: _host(res[k]) for k in KEYS}


def _sweep(nodes, w, dev=False, warm=None, out=None):
    """Nodes.solve as the sweep loop calls it (cold, or warm = a z)."""
    up = _up(dev)
    res = nodes.solve(up(w), warm=None if warm is None else (warm if out is not None else up(warm)), out=out)
    nodes.eng.synchronize()
    return {k: _host(res[k]) for k in KEYS}


def _bars(res, ref, what):
    scale = max(1.0, np.max(np.abs(ref["z"])))
    err = np.max(np.abs(res["z"] - ref["z"]))
    print(f"{what}: max |dz| {err:.2e} (bar {1e-9 * scale:.2e}), max resid {np.max(res['resid']):.2e}, pivots {res['pivots']}")
    assert np.array_equal(res["status"], ref["status"]), what
    assert np.array_equal(res["active"], ref["active"]), what
    assert err <= 1e-9 * scale and np.max(res["resid"]) <= 1e-8, what


def _same_bits(a, b):
    return [k for k in KEYS if np.ascontiguousarray(a[k]).tobytes() != np.ascontiguousarray(b[k]).tobytes()]


def _with_lam(z, lam, n):
    h = np.array(z)
    h[:, n:] = lam
    return h


# ---- 1. true hints
@pytest.mark.parametrize("n,m,mode,dev,per_node", [(130, 40, "loose", False, False), (160, 140, "plain", True, True),
                                                   (200, 150, "plain", False, True), (256, 256, "plain", True, False)])
def test_true_hints_hold(warm, oracle, n, m, mode, dev, per_node):
    rec, w = C.records(n, m, mode)
    if per_node:
        w = C.per_node(w)
    ref = _oracle(oracle, (n, m, mode, per_node), rec, w)
    h = warm.upload_nodes(*C.abi(rec))
    assert h.info()["symmetric"]
    cold = _sweep(h, w, dev)
    _bars(cold, ref, "cold")
    assert np.all(cold["pivots"] >= n) and np.any(cold["pivots"] > n)
    hot = _sweep(h, w, dev, warm=cold["z"])
    _bars(hot, ref, "hinted")
    assert np.all(hot["pivots"] == n)
    # the sweep loop's form: the hint is the z of the output buffers
    out = h.solve(_up(dev)(w))
    again = _sweep(h, w, dev, warm=out["z"], out=out)
    assert not _same_bits(hot, again), _same_bits(hot, again)
    h.close()


# ---- 2. w moved
@pytest.mark.parametrize("delta", [1e-3, 1e-1])
@pytest.mark.parametrize("n,m,dev,per_node", [(160, 140, False, True), (256, 256, True, False)])
def test_a_hint_from_before_a_move_of_w_saves_pivots(warm, oracle, n, m, dev, per_node, delta):
    rec, w = C.records(n, m, "plain")
    if per_node:
        w = C.per_node(w)
    w2 = C.moved(w, delta)
    ref2 = _oracle(oracle, (n, m, "plain", per_node, delta), rec, w2)
    h = warm.upload_nodes(*C.abi(rec))
    z = _sweep(h, w, dev)["z"]
    un = _sweep(h, w2, dev)
    hot = _sweep(h, w2, dev, warm=z)
    h.close()
    _bars(un, ref2, "un-hinted")
    _bars(hot, ref2, "hinted")
    assert np.sum(hot["pivots"] - n) < np.sum(un["pivots"] - n)


# ---- 3. wrong hints, survived
@pytest.mark.parametrize("kind", C.WRONG)
@pytest.mark.parametrize("n,m,mode,dev", [(130, 40, "loose", True), (160, 140, "plain", False)])
def test_wrong_hints_are_solved_all_the_same(warm, oracle, n, m, mode, dev, kind):
    rec, w = C.records(n, m, mode)
    ref = _oracle(oracle, (n, m, mode, False), rec, w)
    h = warm.upload_nodes(*C.abi(rec))
    hint = _with_lam(ref["z"], C.wrong(kind, ref["z"][:, n:], rec[5]), n)
    res = _run(warm, h, w, hint, True, dev)
    h.close()
    _bars(res, ref, kind)


@pytest.mark.parametrize("n,m,rows,dev", [(96, 200, 110, False), (70, 255, 100, True)])
def test_a_restart_after_a_failed_seed_finishes_by_block_pivoting(warm, oracle, n, m, rows, dev):
    """Loose records, a seed of `rows` rows: within the cap, above the rank n of S, so the seeded attempt fails in its first
    factorisation.  The cold rule names few rows here and the un-hinted call finishes by block principal pivoting (the twin: every
    node at (96, 200), three of four at (70, 255)); the restart has to do the same in the same launch -- pivots = n + the pairs
    the cold run switches, which is what the un-hinted call reports and what the twin counts.  A restart that kept the failure
    flag or the seed, or ran no rounds, would leave the node to the Lemke kernel, which counts its own pivots."""
    from qpn_amd import _lib
    from qpn_amd.level_batch import warm_big_host
    rec, w = C.records(n, m, "loose")
    ref = _oracle(oracle, (n, m, "loose", False), rec, w)
    S, c = C.schur(rec, w)
    twin = [warm_big_host(S[b], c[b], rec[5][b], rec[6][b]) for b in range(C.CNT)]
    bpp = np.array([r["finished"] for r in twin])
    assert bpp.sum() >= 3 and all(r["switched"] > 0 for r in twin if r["finished"])
    h = warm.upload_nodes(*C.abi(rec))
    hint = _with_lam(ref["z"], C.dependent(m, rows=rows), n)
    un = _sweep(h, w, dev)
    hot = _run(warm, h, w, hint, True, dev)
    warm.set_option(_lib.OPT_SYM_ROUTE, 0)
    lemke = _sweep(h, w, dev)                                   # the Lemke kernel alone: its own pivot counts
    h.close()
    _bars(un, ref, "un-hinted")
    _bars(hot, ref, "dependent seed, restarted")
    print("twin switched", [r["switched"] for r in twin], "Lemke alone", lemke["pivots"])
    assert np.array_equal(un["pivots"][bpp], n + np.array([r["switched"] for r in twin])[bpp])
    assert np.all(lemke["pivots"][bpp] != un["pivots"][bpp])    # (so the counts tell the two kernels apart)
    assert np.array_equal(hot["pivots"], un["pivots"])


def test_a_dependent_seed_on_nodes_the_cold_start_cannot_finish_either(warm, oracle):
    """(70, 255) plain: the seed (100 rows) and the cold rule both name more rows than S has rank; both attempts end in their first
    factorisation and the Lemke kernel solves the nodes, as it does un-hinted."""
    n, m = 70, 255
    rec, w = C.records(n, m, "plain")
    ref = _oracle(oracle, (n, m, "plain", False), rec, w)
    h = warm.upload_nodes(*C.abi(rec))
    res = _run(warm, h, w, _with_lam(ref["z"], C.dependent(m), n), True)
    h.close()
    _bars(res, ref, "dependent seed")


# ---- 4. dropped hints: bit for bit the call without the flag
@pytest.mark.parametrize("what", ["over the cap", "every row named", "zeros", "nan", "infinite sides"])
def test_dropped_hints_change_no_bit(warm, oracle, what):
    n, m, mode = (200, 150, "tight") if what == "over the cap" else (160, 140, "plain")
    rec, w = C.records(n, m, mode)
    ref = _oracle(oracle, (n, m, mode, False), rec, w)
    lam = ref["z"][:, n:]
    if what == "over the cap":
        named = np.count_nonzero(lam, axis=1)
        assert np.all(named > C.KMAX), named
    elif what == "every row named":
        lam = C.all_lower(lam, rec[5])
    elif what == "zeros":
        lam = np.zeros_like(lam); lam[:, 1::2] = -0.0
    elif what == "nan":
        lam = np.full_like(lam, np.nan)
    else:
        rec, lam = C.one_sided(rec)
        ref = _oracle(oracle, (n, m, mode, "one-sided"), rec, w)
    hint = _with_lam(ref["z"], lam, n)
    h = warm.upload_nodes(*C.abi(rec))
    for dev in (False, True):
        flagged = _run(warm, h, w, hint, True, dev)
        plain = _run(warm, h, w, hint, False, dev)
        assert not _same_bits(flagged, plain), (dev, _same_bits(flagged, plain))
        _bars(flagged, ref, what)
    h.close()


# ---- 5. calls that ignore the hint: bit for bit the call without the flag
@pytest.mark.parametrize("what", ["option 0", "general variants", "pivot budget", "asymmetric Qd", "records per call", "shape (96, 96)"])
def test_calls_outside_the_contract_ignore_the_hint(warm, oracle, what):
    from qpn_amd import _lib
    n, m = (96, 96) if what == "shape (96, 96)" else (160, 140)
    rec, w = C.records(n, m, "plain")
    if what == "asymmetric Qd":
        K = np.random.default_rng(3).standard_normal(rec[0].shape) * 0.02
        rec = (rec[0] + (K - K.transpose(0, 2, 1)),) + rec[1:]
    ref = _oracle(oracle, (n, m, "plain", "asym" if what == "asymmetric Qd" else False), rec, w)
    hint = np.array(ref["z"])
    if what == "option 0":
        warm.set_option(_lib.OPT_WARM_BIG, 0)
    if what == "general variants":
        warm.set_option(_lib.OPT_SYM_ROUTE, 0)
    src = C.abi(rec) if what == "records per call" else warm.upload_nodes(*C.abi(rec))
    if what not in ("records per call", "asymmetric Qd"):
        assert src.info()["symmetric"]
    budget = 100_000 if what == "pivot budget" else 0
    flagged = _run(warm, src, w, hint, True, True, budget)
    plain = _run(warm, src, w, hint, False, True, budget)
    if what != "records per call":
        src.close()
    assert not _same_bits(flagged, plain), _same_bits(flagged, plain)
    assert np.all(flagged["status"] == 1)
    if what == "option 0":
        assert np.any(flagged["pivots"] > n)                    # (block principal pivoting, un-hinted: it switches pairs)


def test_the_option_takes_0_and_1(warm):
    from qpn_amd import _lib
    from qpn_amd.engine import QpnError
    with pytest.raises(QpnError):
        warm.set_option(_lib.OPT_WARM_BIG, 2)
    with pytest.raises(QpnError):
        warm.set_option(99, 1)


# ---- 6. nodes that block principal pivoting cannot finish
@pytest.mark.parametrize("case", ["rank", "cap", "equality"])
def test_nodes_left_to_the_lemke_kernel_take_the_hint_in_their_stride(warm, oracle, case):
    if case == "equality":
        n, m = 100, 140
        Q, R, qd, A, B, l, u = P.synth_nodes(30_000 + 9, C.CNT, n, m)
        w = P.shared_params()
        x0 = np.random.default_rng(1).standard_normal((C.CNT, n))
        s0 = np.einsum("bij,bj->bi", A, x0) + B @ w
        l[:, :5] = u[:, :5] = s0[:, :5]                             # five equality rows through a common point
        l[:, 5:] = np.minimum(l[:, 5:], s0[:, 5:] - 0.1); u[:, 5:] = np.maximum(u[:, 5:], s0[:, 5:] + 0.1)
        rec = (Q, R, qd, A, B, l, u)
    else:
        n, m, mode = (96, 200, "plain") if case == "rank" else (200, 150, "tight")
        rec, w = C.records(n, m, mode)
    ref = _oracle(oracle, (case, "left"), rec, w)
    h = warm.upload_nodes(*C.abi(rec))
    cold = _sweep(h, w)
    hot = _sweep(h, w, warm=cold["z"])
    h.close()
    _bars(cold, ref, case + ", cold")
    _bars(hot, ref, case + ", hinted")


# ---- 7. with the crash cache of the large class
def test_hinted_sweeps_reuse_and_fill_the_big_crash_cache(warm, oracle):
    from qpn_amd import _lib
    n, m = 160, 140
    rec, w = C.records(n, m, "plain")
    ref = _oracle(oracle, (n, m, "plain", False), rec, w)
    warm.set_option(_lib.OPT_CRASH_CACHE_BIG, 1)
    h = warm.upload_nodes(*C.abi(rec))
    cold = _sweep(h, w, True)                               # the filling sweep
    assert h.info()["big_cached"]
    _bars(cold, ref, "filling sweep")
    for sweep in range(2):
        hot = _sweep(h, w, True, warm=cold["z"])
        assert h.info()["big_cached"]
        _bars(hot, ref, f"hinted reuse sweep {sweep}")
        assert np.all(hot["pivots"] == n)
    # a hinted sweep as the first of a fresh handle, the hint from the other handle's solution: it fills the cache
    g = warm.upload_nodes(*C.abi(rec))
    assert not g.info()["big_cached"]
    first = _sweep(g, w, True, warm=cold["z"])
    assert g.info()["big_cached"] and not g.info()["big_refused"]
    _bars(first, ref, "hinted filling sweep")
    assert np.all(first["pivots"] == n)
    second = _sweep(g, w, True, warm=first["z"])
    assert g.info()["big_cached"]
    _bars(second, ref, "hinted reuse sweep of the second handle")
    assert np.all(second["pivots"] == n)
    h.close(); g.close()
