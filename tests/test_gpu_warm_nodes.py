"""QPN_AVI_FLAG_WARM_DUALS on the GPU: the warm kernel (csrc/qpn_warm.hip) and the cold route behind it for what it declines.

The nodes and hints of tests/warm_cases.py (nine families, shapes (32, 32), (5, 7), (1, 32), (32, 1), (17, 32)) through the
per-call and the handle route, host and device memory, symmetric and general records, crash cache on and off, batches of 1,
70 and RESIDENT + 1.
  1. true hints: status SUCCESS, pivots 0, and the accuracy bar and masks solve_cases.check_against_truth applies to the cold
     routes (E_ref: the CPU oracle's error on the same nodes);
  2. each of the seven wrong hints: every output bit-equal to the same call without the flag;
  3. true and wrong hints alternating: each node as in 1 or 2;
  4. random hints: a node that comes back with pivots 0 claims the truth's active set and meets the bar, every other node is
     bit-equal to the cold call;
  5. a real sweep: cold at w, then w + dw with the previous z as the hint, dw drawn per node so small that the active set is
     proved unchanged (solve_ref's certificate with the old z's sides at the new parameters; a node for which no dw does is
     discarded and drawn again): every node is accepted;
  6. the flag at (48, 48) and on qpn_solve_avi_batch: the cold result, bit-equal;
  7. level_batch.WARM_DUALS_ROUTE through solve(): solved, x within the golden cases' tolerance of the route off.
"""
import numpy as np
import pytest
import torch

import goldenio as G
import solve_cases as SC
import solve_ref as SR
import warm_cases as WC

pytestmark = pytest.mark.gpu

KEYS = ("z", "status", "resid", "pivots", "active")
_E_REF = {}


def _abi(nodes):
    from qpn_amd.engine import colmajor
    Q, R, qd, A, B, l, u = SC.stack(nodes)
    return [colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u]


def _e_ref(oracle, n, m):
    """The oracle's worst error per family on the shape's nodes (computed once)."""
    if (n, m) not in _E_REF:
        nodes = WC.shape_nodes(n, m)
        ref = SC.oracle_solve(oracle, nodes, nodes[0]["w"])
        assert np.all(ref["status"] == 1)
        e = {}
        for c, zo in zip(nodes, ref["z"]):
            e[c["family"]] = max(e.get(c["family"], 0.0), SR.node_error(zo, SC.truth(c)[0], n, SC.row_norm(c)))
        _E_REF[n, m] = e
    return _E_REF[n, m]


def _host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _run(engine, src, w, hint, flag, dev, n):
    """One call with the hint in z.  src: the seven record arrays (per-call route) or a Nodes handle.  -> host copies of z,
    status, resid, pivots, active and of the x scatter (a [batch, n + 2] buffer of sevens: the two spare columns stay)."""
    from qpn_amd import _lib
    batch, N = hint.shape
    up = (lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()) if dev else (lambda a: np.array(a))
    o = engine.default_opts()
    if flag:
        o.flags |= _lib.AVI_FLAG_WARM_DUALS
    x = up(np.full((batch, n + 2), 7.0))
    if isinstance(src, list):
        res = engine.solve_nodes(*[up(a) for a in src], up(w), z0=up(hint), opts=o, x_out=x)
    else:
        out = dict(z=up(hint), status=up(np.zeros(batch, np.int32)), resid=up(np.zeros(batch)), pivots=up(np.zeros(batch, np.int32)),
                   active=up(np.zeros((batch, N), np.uint8)))
        wd = up(w)
        if flag:
            res = src.solve(wd, opts=o, out=out, x_out=x)
        else:
            # Nodes.solve adds COLD_START to every call that brings no hint, and a cold start is another call (the general
            # kernel behind the fused one reads z0): the SAME call without the flag is made at the ABI
            import ctypes as C
            from qpn_amd.engine import _ptr
            engine._bind_stream(dev)
            engine._call("qpn_solve_nodes_h", src.h, _ptr(wd), 0 if wd.ndim == 1 else wd.shape[1], _ptr(out["z"]), _ptr(out["status"]),
                         _ptr(out["resid"]), _ptr(out["pivots"]), _ptr(out["active"]), C.byref(o), engine._mem(dev), _ptr(x), n + 2)
            res = out
    engine.synchronize()
    got = {k: _host(res[k]) for k in KEYS}
    got["x"] = _host(x)
    return got


def _same_bits(a, b, idx=None):
    """The outputs of two calls, bit for bit (on the nodes idx) -> the names that differ."""
    pick = (lambda v: v) if idx is None else (lambda v: v[idx])
    return [k for k in a if np.ascontiguousarray(pick(a[k])).tobytes() != np.ascontiguousarray(pick(b[k])).tobytes()]


def _check_accepted(nodes, res, idx, where, e_ref, n):
    idx = list(idx)
    sub = [nodes[i] for i in idx]
    got = {k: res[k][idx] for k in KEYS}
    fails = [f"{where} [{i}] {nodes[i]['family']}: pivots {res['pivots'][i]}" for i in idx if res["pivots"][i] != 0]
    fails += SC.check_against_truth(sub, [SC.truth(c) for c in sub], got, where, {}, e_ref)
    for i in idx:
        if not np.array_equal(res["x"][i, :n], res["z"][i, :n]) or not np.all(res["x"][i, n:] == 7.0):
            fails.append(f"{where} [{i}]: x scatter")
    return fails


# the routes a batch of one shape is run through: (name, resident handle?, device memory?, families, crash cache)
ROUTES = [("call/host", False, False, None, 1), ("call/device", False, True, None, 1), ("handle-general/device", True, True, None, 1),
          ("handle-general/host", True, False, None, 1), ("handle-sym/device", True, True, SC.SYMMETRIC, 1),
          ("handle-sym-nocache/device", True, True, SC.SYMMETRIC, 0)]


class _Source:
    """The record source of one route over some nodes: the arrays, or a handle (closed on exit) that has made one cold sweep,
    so that a symmetric one with the crash cache on holds a valid cache."""

    def __init__(self, engine, route, nodes, reps=1):
        from qpn_amd import _lib
        self.engine, (self.name, self.handle, self.dev, fams, self.cache) = engine, route
        self.idx = [i for i, c in enumerate(nodes) if fams is None or c["family"] in fams]
        self.nodes = [nodes[i] for i in self.idx] * reps
        abi = _abi([nodes[i] for i in self.idx])
        if reps > 1:
            abi = [np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1))) for a in abi]
        self.src = abi
        self._lib = _lib

    def __enter__(self):
        if self.handle and self.nodes:
            self.engine.set_option(self._lib.OPT_CRASH_CACHE, self.cache)
            self.src = self.engine.upload_nodes(*self.src)
            self.src.solve(self.nodes[0]["w"])
            info = self.src.info()
            sym = all(np.array_equal(c["rec"][0], c["rec"][0].T) for c in self.nodes)     # (a 1 x 1 Qd of any family is)
            n, m = self.src.n, self.src.m
            assert info["symmetric"] == sym and info["crash_cached"] == (sym and self.cache == 1 and (n, m) == (32, 32)), info
        return self

    def __exit__(self, *exc):
        if self.handle and not isinstance(self.src, list):
            self.src.close()
            self.engine.set_option(self._lib.OPT_CRASH_CACHE, 1)


def _batches():
    """(n, m, reps): every shape once; (32, 32) also as a batch of 70 or more."""
    return [(n, m, 1) for n, m in WC.SHAPES] + [(32, 32, 5)]


def test_true_hints_are_accepted(engine, oracle):
    fails = []
    for n, m, reps in _batches():
        nodes = WC.shape_nodes(n, m)
        for route in ROUTES:
            if reps > 1 and route[0] not in ("call/device", "handle-sym/device"):
                continue
            with _Source(engine, route, nodes, reps) as s:
                assert reps == 1 or len(s.nodes) >= 70
                rng = np.random.default_rng([5, n, m])
                hints = np.stack([WC.true_hint(c, rng) for c in s.nodes])
                res = _run(engine, s.src, s.nodes[0]["w"], hints, True, s.dev, n)
                fails += _check_accepted(s.nodes, res, range(len(s.nodes)), f"({n},{m})x{reps} {s.name}", _e_ref(oracle, n, m), n)
    # a batch of one node
    nodes = WC.shape_nodes(32, 32)[:1]
    rng = np.random.default_rng(6)
    res = _run(engine, _abi(nodes), nodes[0]["w"], np.stack([WC.true_hint(nodes[0], rng)]), True, True, 32)
    fails += _check_accepted(nodes, res, [0], "(32,32) one node", _e_ref(oracle, 32, 32), 32)
    assert not fails, "\n".join(fails[:12]) + f"\n... {len(fails)} in all"


@pytest.mark.parametrize("kind", WC.WRONG)
def test_wrong_hints_give_the_cold_call_bit_for_bit(engine, kind):
    seen = 0
    for n, m in WC.SHAPES:
        rng = np.random.default_rng([7, n, m, WC.WRONG.index(kind)])
        pairs = [(c, WC.wrong_hint(c, kind, rng)) for c in WC.shape_nodes(n, m)]
        nodes = [c for c, z in pairs if z is not None]
        hint_of = {id(c): z for c, z in pairs if z is not None}
        if not nodes:
            continue
        for route in ROUTES:
            if (n, m) != (32, 32) and route[0] not in ("call/host", "handle-general/device"):
                continue
            with _Source(engine, route, nodes) as s:
                if not s.nodes:
                    continue
                hints = np.stack([hint_of[id(c)] for c in s.nodes])
                w = s.nodes[0]["w"]
                cold = _run(engine, s.src, w, hints, False, s.dev, n)
                warm = _run(engine, s.src, w, hints, True, s.dev, n)
                assert np.all(cold["status"] == 1), (kind, n, m, s.name)
                assert not _same_bits(cold, warm), (kind, n, m, s.name, _same_bits(cold, warm))
                seen += len(s.nodes)
    assert seen >= 10, (kind, seen)


@pytest.mark.parametrize("big", [False, True])
def test_mixed_batch_each_node_on_its_own(engine, oracle, big):
    """True and wrong hints alternate node by node: 70 or more nodes on every route, and RESIDENT + 1 or more on the symmetric
    handle -- the cold launch behind the warm kernel is then the mixed reuse / recompute launch over the decliners' list."""
    n = m = 32
    nodes = WC.shape_nodes(n, m)
    routes = [r for r in ROUTES if r[0] == "handle-sym/device"] if big else ROUTES
    fails = []
    for route in routes:
        per = sum(1 for c in nodes if route[3] is None or c["family"] in route[3])
        reps = (SC.RESIDENT // per + 1) if big else -(-70 // per)
        with _Source(engine, route, nodes, reps) as s:
            count = len(s.nodes)
            assert count > SC.RESIDENT if big else count >= 70
            rng = np.random.default_rng([8, reps])
            wrong = np.arange(count) % 2 == 1
            kinds = ("dropped", "swapped", "nan", "empty", "added")
            hints = []
            for i, c in enumerate(s.nodes):
                z = None
                if wrong[i]:
                    z = WC.wrong_hint(c, kinds[(i // 2) % len(kinds)], rng)
                    z = WC.wrong_hint(c, "nan", rng) if z is None else z
                hints.append(WC.true_hint(c, rng) if z is None else z)
            hints = np.stack(hints)
            w = s.nodes[0]["w"]
            cold = _run(engine, s.src, w, hints, False, s.dev, n)
            warm = _run(engine, s.src, w, hints, True, s.dev, n)
            diff = _same_bits(cold, warm, np.flatnonzero(wrong))
            if diff:
                fails.append(f"{s.name} x{reps}: wrong-hint nodes differ from the cold call in {diff}")
            # the accepted ones: all of them when the batch is small, a stride of them when it is tiled (copies of 16 nodes)
            idx = np.flatnonzero(~wrong)
            assert np.all(warm["status"][idx] == 1) and np.all(warm["pivots"][idx] == 0), s.name
            fails += _check_accepted(s.nodes, warm, idx[:: max(1, idx.size // 64)], f"{s.name} x{reps}", _e_ref(oracle, n, m), n)
            if s.handle:
                info = s.src.info()
                assert info["crash_cached"] == (route[3] is not None and route[4] == 1), info
    assert not fails, "\n".join(fails[:12])


def test_random_hints_never_a_wrong_accept(engine, oracle):
    fails, accepted, declined = [], 0, 0
    for n, m in WC.SHAPES:
        nodes = WC.shape_nodes(n, m) * 4
        rng = np.random.default_rng([9, n, m])
        hints = np.stack([WC.random_hint(c, rng) for c in nodes])
        w = nodes[0]["w"]
        src = _abi(nodes)
        cold = _run(engine, src, w, hints, False, True, n)
        warm = _run(engine, src, w, hints, True, True, n)
        zero = np.flatnonzero(warm["pivots"] == 0)
        rest = np.flatnonzero(warm["pivots"] != 0)
        for i in zero:                                    # the active set the point claims is the truth's
            c = nodes[i]
            got, want = WC.sides_of(warm["z"][i], n), c["side"]
            if not np.array_equal(got[~c["weak"]], want[~c["weak"]]):
                fails.append(f"({n},{m}) [{i}] {c['family']}: accepted with sides {got} against the truth's {want}")
        fails += _check_accepted(nodes, warm, zero, f"({n},{m}) random", _e_ref(oracle, n, m), n)
        diff = _same_bits(cold, warm, rest)
        if diff:
            fails.append(f"({n},{m}): nodes with pivots > 0 differ from the cold call in {diff}")
        accepted += int(np.sum(np.any(warm["z"][zero] != cold["z"][zero], axis=1)))
        declined += rest.size
    assert not fails, "\n".join(fails[:12])
    assert accepted > 0 and declined > 0, (accepted, declined)      # both outcomes occurred


def test_a_real_sweep_keeps_every_node(engine, oracle):
    """Cold at w, then w + dw with the previous z as the hint.  Per node, dw is drawn so small that the active set the previous z
    names -- the sides of its multipliers, which is all the hint says -- is still THE active set at w + dw: solve_ref's
    certificate with those sides at the new parameters.  A node for which no dw does (a weakly active row whose multiplier came
    out of the cold solve as a rounding error: it names a set that holds at no other w) is discarded and drawn again."""
    fails = []
    for n, m in [(32, 32), (17, 32)]:
        nodes = list(WC.shape_nodes(n, m))
        rng = np.random.default_rng([10, n, m])
        w0 = nodes[0]["w"]
        W, moved, todo = [None] * len(nodes), [None] * len(nodes), list(range(len(nodes)))
        for _ in range(12):
            first = _run(engine, _abi(nodes), w0, np.zeros((len(nodes), n + m)), False, True, n)
            assert np.all(first["status"] == 1)
            again = []
            for i in todo:
                c, ok = nodes[i], False
                side = WC.sides_of(first["z"][i], n)
                for scale in 1e-3 * 0.5 ** np.arange(6):
                    w = w0 + scale * rng.standard_normal(w0.size)
                    try:
                        zt, info = SR.solve_reference(*c["rec"], w, side)
                        ok = info["ok"]
                    except (AssertionError, np.linalg.LinAlgError, ValueError):
                        ok = False
                    if ok:
                        break
                if ok:
                    info["w"] = w
                    W[i], moved[i] = w, dict(c, w=w, side=side, _truth=(zt, info))
                else:
                    nodes[i] = SC.make_node(rng, n, m, c["family"], WC.P, w0)
                    again.append(i)
            todo = again
            if not todo:
                break
        assert not todo, [nodes[i]["family"] for i in todo]
        W = np.stack(W)
        res = _run(engine, _abi(nodes), W, first["z"], True, True, n)
        ref = SC.oracle_solve(oracle, moved, W)
        e_ref = {}
        for c, zo in zip(moved, ref["z"]):
            e_ref[c["family"]] = max(e_ref.get(c["family"], 0.0), SR.node_error(zo, c["_truth"][0], n, SC.row_norm(c)))
        fails += _check_accepted(moved, res, range(len(nodes)), f"({n},{m}) sweep", e_ref, n)
    assert not fails, "\n".join(fails[:12])


def test_other_size_classes_and_entries_ignore_the_flag(engine):
    import problems as P
    from qpn_amd import _lib
    from qpn_amd.engine import colmajor
    n = m = 48
    rng = np.random.default_rng(11)
    w = rng.standard_normal(WC.P)
    nodes = [SC.make_node(rng, n, m, f, WC.P, w) for f in ("k40", "skew", "k0")]
    hints = np.stack([WC.true_hint(c, rng) for c in nodes])
    cold = _run(engine, _abi(nodes), w, hints, False, True, n)
    warm = _run(engine, _abi(nodes), w, hints, True, True, n)
    assert np.all(cold["status"] == 1) and not _same_bits(cold, warm), _same_bits(cold, warm)
    # qpn_solve_avi_batch on the assembled blocks of the (32, 32) nodes
    nodes = WC.shape_nodes(32, 32)
    M, q, lo, hi, kind = P.reduced_blocks(*SC.stack(nodes), nodes[0]["w"])
    hints = np.stack([WC.true_hint(c, rng) for c in nodes])
    res = []
    for flag in (0, _lib.AVI_FLAG_WARM_DUALS):
        o = engine.default_opts()
        o.flags |= flag
        r = engine.solve_avi_batch(colmajor(M), q, lo, hi, z0=hints, kind=kind, opts=o)
        res.append({k: _host(r[k]) for k in KEYS})
    assert np.all(res[0]["status"] == 1) and np.any(res[0]["pivots"] > 0) and not _same_bits(*res), _same_bits(*res)


def test_route_switch_through_solve(engine):
    from qpn_amd import algorithm, examples, level_batch
    c = G.load("simple_bilevel_cases.json")
    jobs = [(lambda: examples.setup("simple_bilevel", gen_solution_map=True), np.array(list(w) + c["x0"], float)) for w in c["w"]]
    jobs.append((lambda: examples.setup("synthetic_pairs", pairs=20, n=6, m=8), None))
    assert len(jobs) == 9
    for make, x0 in jobs:
        out = []
        for route in (False, True):
            level_batch.WARM_DUALS_ROUTE = route
            try:
                out.append(algorithm.solve(make(), x0, engine=engine) if x0 is not None else algorithm.solve(make(), engine=engine))
            finally:
                level_batch.WARM_DUALS_ROUTE = False
        off, on = out
        assert off["solved"] and on["solved"]
        assert np.allclose(on["x_opt"], off["x_opt"], atol=c["atol"]), np.max(np.abs(on["x_opt"] - off["x_opt"]))
