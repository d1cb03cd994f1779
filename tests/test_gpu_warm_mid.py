"""The warm start of the mid-size classes on the GPU: qpn_nodes_set_warm, the warm kernel (csrc/qpn_warm_mid.hip) and the cold
kernels behind it for what it declines.

The nodes of tests/warm_mid_cases.py (the class corners of solve_cases.CELLS and (97, 64), ten families, three nodes each) with
warm_cases' hints, on resident handles that opted in.  Every comparison with the cold route is bit for bit over z, status, resid,
pivots, active and the x scatter buffer ([batch, n + 2] with two sentinel columns); "the same call without the flag" is made at
the ABI.
  1. true hints: inside level_batch.warm_mid_fits status SUCCESS, pivots 0, and the accuracy bar and masks of
     solve_cases.check_against_truth (E_ref: the CPU oracle's error on the same nodes); outside it the cold bits and pivots > 0;
  2. each of the seven wrong hints: the cold bits;
  3. true and wrong hints alternating on batches beyond each class's schedule threshold, with a schedule installed: each node as
     in 1 or 2, and a cold sweep afterwards equals one on a handle that never saw a warm sweep;
  4. random hints: a node with pivots 0 claims the truth's active set and meets the bar, every other one has the cold bits;
  5. a real sweep at (64, 64) and (97, 64): cold at w, then w + dw with the previous z as the hint, dw so small per node that
     solve_ref's certificate proves the set unchanged: every node is accepted;
  6. outside the contract -- a handle never opted in or set back to 0, per-call records, QPN_OPT_MID_ROUTE = 0,
     QPN_AVI_FLAG_COLD_START: the cold bits; set_warm(2) raises; (32, 32) and (160, 140) handles take the call unchanged;
  7. after qpn_nodes_update of qd, l, u the old hint declines and the new one is accepted; warm sweeps leave the decline census alone;
  8. level_batch.WARM_DUALS_MID through solve(): solved, x within the golden cases' tolerance of the route off.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import goldenio as G
import solve_cases as SC
import solve_ref as SR
import warm_cases as WC
import warm_mid_cases as MC

pytestmark = pytest.mark.gpu

KEYS = ("z", "status", "resid", "pivots", "active")
_REF = {}


def _abi(nodes):
    from qpn_amd.engine import colmajor
    Q, R, qd, A, B, l, u = SC.stack(nodes)
    return [colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u]


def _fits(n, k):
    from qpn_amd import level_batch
    return level_batch.warm_mid_fits(n, k)


def _reference(oracle, cls, n, m, per_node=False):
    """(w, truths, E_ref) of a shape's nodes, computed once: at the plant's shared w, or at solve_cases.per_node_params with the
    truth by certificate from the active set the oracle's answer claims.  E_ref: the oracle's worst error per family."""
    key = (n, m, per_node)
    if key not in _REF:
        nodes = MC.shape(n, m)[4]
        if per_node:
            w = SC.per_node_params(cls, nodes)
            ref = SC.oracle_solve(oracle, nodes, w)
            truths = [SC.truth_from_solution(c, w[i], ref["z"][i]) for i, c in enumerate(nodes)]
        else:
            w = nodes[0]["w"]
            ref = SC.oracle_solve(oracle, nodes, w)
            truths = [SC.truth(c) for c in nodes]
        assert np.all(ref["status"] == 1)
        e = {}
        for c, zo, (zt, _) in zip(nodes, ref["z"], truths):
            e[c["family"]] = max(e.get(c["family"], 0.0), SR.node_error(zo, zt, n, SC.row_norm(c)))
        _REF[key] = (w, truths, e)
    return _REF[key]


def _host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _run(engine, src, w, hint, flag, dev, n, flags=None, max_pivots=None):
    """One call with the hint in z.  src: the seven record arrays (per-call route) or a Nodes handle.  flags: the call's flag bits
    given outright, max_pivots: a pivot budget (both made at the ABI).  -> host copies of z, status, resid, pivots, active and of the x scatter (a [batch, n + 2]
    buffer of sevens: the two spare columns stay)."""
    from qpn_amd import _lib
    from qpn_amd.engine import _ptr
    batch, N = hint.shape
    up = (lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()) if dev else (lambda a: np.array(a))
    o = engine.default_opts()
    if flag:
        o.flags |= _lib.AVI_FLAG_WARM_DUALS
    if flags is not None:
        o.flags = flags
    if max_pivots is not None:
        o.max_pivots = max_pivots
    x = up(np.full((batch, n + 2), 7.0))
    if isinstance(src, list):
        res = engine.solve_nodes(*[up(a) for a in src], up(w), z0=up(hint), opts=o, x_out=x)
    else:
        out = dict(z=up(hint), status=up(np.zeros(batch, np.int32)), resid=up(np.zeros(batch)), pivots=up(np.zeros(batch, np.int32)),
                   active=up(np.zeros((batch, N), np.uint8)))
        wd = up(np.asarray(w, dtype=np.float64))
        if dev and wd.numel() == 0:                       # p = 0: an empty tensor with the unit stride Nodes.solve asks for
            wd = torch.zeros(1, dtype=torch.float64, device="cuda")[:0]
        if flag and flags is None and max_pivots is None:
            res = src.solve(wd, opts=o, out=out, x_out=x)
        else:
            # Nodes.solve adds COLD_START to every call that brings no hint, and a cold start is another call: the SAME call
            # without the flag is made at the ABI
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


def _check_accepted(nodes, truths, res, idx, where, e_ref, n):
    idx = list(idx)
    sub = [nodes[i] for i in idx]
    got = {k: res[k][idx] for k in KEYS}
    fails = [f"{where} [{i}] {nodes[i]['family']}: pivots {res['pivots'][i]}" for i in idx if res["pivots"][i] != 0]
    fails += SC.check_against_truth(sub, [truths[i] for i in idx], got, where, {}, e_ref)
    for i in idx:
        if not np.array_equal(res["x"][i, :n], res["z"][i, :n]) or not np.all(res["x"][i, n:] == 7.0):
            fails.append(f"{where} [{i}]: x scatter")
    return fails


class _Handle:
    """A resident handle over some nodes (tiled `reps` times), opted in unless told otherwise; closed on exit."""

    def __init__(self, engine, nodes, reps=1, warm=True):
        self.engine, self.nodes, self.warm = engine, list(nodes) * reps, warm
        abi = _abi(nodes)
        self.abi = [np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1))) for a in abi] if reps > 1 else abi

    def __enter__(self):
        self.h = self.engine.upload_nodes(*self.abi)
        if self.warm:
            self.h.set_warm(True)
        return self

    def __exit__(self, *exc):
        self.h.close()


ROUTES = [("general/device", None, True), ("general/host", None, False), ("sym/device", SC.SYMMETRIC, True),
          ("sym/host", SC.SYMMETRIC, False)]


@pytest.mark.parametrize("cls", MC.CLASSES)
def test_true_hints_on_an_opted_in_handle(engine, oracle, cls):
    fails, inside, outside = [], 0, 0
    for _, n, m, p, nodes in [s for s in MC.shapes() if s[0] == cls]:
        for name, fams, dev in ROUTES:
            idx = [i for i, c in enumerate(nodes) if fams is None or c["family"] in fams]
            sub = [nodes[i] for i in idx]
            with _Handle(engine, sub) as s:
                assert s.h.info()["symmetric"] == all(np.array_equal(c["rec"][0], c["rec"][0].T) for c in sub)
                for per_node in ((False, True) if name == "general/device" and p > 0 else (False,)):
                    w, truths, e_ref = _reference(oracle, cls, n, m, per_node)
                    truths = [truths[i] for i in idx]
                    w = w[idx] if per_node else w
                    rng = np.random.default_rng([5, n, m, per_node])
                    hints = np.stack([WC.hint_from_side(c, np.sign(zt[n:]), rng) for c, (zt, _) in zip(sub, truths)])
                    where = f"({n},{m}) {name}{' per-node w' if per_node else ''}"
                    res = _run(engine, s.h, w, hints, True, dev, n)
                    fit = np.array([_fits(n, MC.hinted_rows(z, n)) for z in hints])
                    fails += _check_accepted(sub, truths, res, np.flatnonzero(fit), where, e_ref, n)
                    inside += int(fit.sum())
                    if not fit.all():
                        cold = _run(engine, s.h, w, hints, False, dev, n)
                        out = np.flatnonzero(~fit)
                        diff = _same_bits(cold, res, out)
                        if diff or not np.all(res["pivots"][out] > 0):
                            fails.append(f"{where}: nodes outside warm_mid_fits differ from the cold call in {diff}, pivots {res['pivots'][out]}")
                        outside += out.size
    assert not fails, "\n".join(fails[:12]) + f"\n... {len(fails)} in all"
    assert inside > 0 and (outside > 0) == (cls == "wg2"), (inside, outside)     # (128, 100): kfull and the larger sets are outside


@pytest.mark.parametrize("kind", WC.WRONG)
def test_wrong_hints_give_the_cold_call_bit_for_bit(engine, kind):
    seen = 0
    for cls, n, m, p, nodes in MC.shapes():
        rng = np.random.default_rng([7, n, m, WC.WRONG.index(kind)])
        pairs = [(c, WC.wrong_hint(c, kind, rng)) for c in nodes]
        sub = [c for c, z in pairs if z is not None]
        if not sub:
            continue
        hints = np.stack([z for c, z in pairs if z is not None])
        for name, fams, dev in ROUTES[:1] if (n, m) not in ((48, 40), (64, 64), MC.LEADERS) else ROUTES[:2]:
            with _Handle(engine, sub) as s:
                w = sub[0]["w"]
                cold = _run(engine, s.h, w, hints, False, dev, n)
                warm = _run(engine, s.h, w, hints, True, dev, n)
                assert np.all(cold["status"] == 1), (kind, n, m, name)
                assert not _same_bits(cold, warm), (kind, n, m, name, _same_bits(cold, warm))
                seen += len(sub)
    assert seen >= 10, (kind, seen)


@pytest.mark.parametrize("cls", MC.CLASSES)
def test_mixed_batches_with_a_schedule(engine, oracle, cls):
    n, m, count = MC.TILED[cls]
    nodes = MC.shape(n, m)[4]
    w, truths, e_ref = _reference(oracle, cls, n, m)
    reps = -(-count // len(nodes))
    with _Handle(engine, nodes, reps) as s, _Handle(engine, nodes, reps, warm=False) as fresh:
        total = len(s.nodes)
        assert total >= count
        s.h.set_schedule(1); fresh.h.set_schedule(1)
        for _ in range(3):
            s.h.solve(w); fresh.h.solve(w)
        engine.synchronize()
        assert s.h.info()["scheduled"]
        rng = np.random.default_rng([8, n, m])
        wrong = np.arange(total) % 2 == 1
        kinds = ("dropped", "swapped", "nan", "empty", "added")
        hints = []
        for i, c in enumerate(s.nodes):
            z = None
            if wrong[i]:
                z = WC.wrong_hint(c, kinds[(i // 2) % len(kinds)], rng)
                z = WC.wrong_hint(c, "nan", rng) if z is None else z
            hints.append(WC.true_hint(c, rng) if z is None else z)
        hints = np.stack(hints)
        cold = _run(engine, s.h, w, hints, False, True, n)
        warm = _run(engine, s.h, w, hints, True, True, n)
        assert np.all(cold["status"] == 1)
        assert not _same_bits(cold, warm, np.flatnonzero(wrong)), _same_bits(cold, warm, np.flatnonzero(wrong))
        idx = np.flatnonzero(~wrong)
        assert all(_fits(n, MC.hinted_rows(hints[i], n)) for i in idx)
        assert np.all(warm["status"][idx] == 1) and np.all(warm["pivots"][idx] == 0)
        fails = _check_accepted(s.nodes, truths * reps, warm, idx[:: max(1, idx.size // 64)], f"({n},{m}) x{reps}", e_ref, n)
        assert not fails, "\n".join(fails[:12])
        # a cold sweep afterwards: as on a handle that never saw a warm sweep
        after = _run(engine, s.h, w, hints, False, True, n)
        never = _run(engine, fresh.h, w, hints, False, True, n)
        assert not _same_bits(after, never), _same_bits(after, never)
        assert not _same_bits(after, cold)


def test_random_hints_never_a_wrong_accept(engine, oracle):
    fails, accepted, declined = [], 0, 0
    for cls, n, m, p, base in MC.shapes():
        w, truths, e_ref = _reference(oracle, cls, n, m)
        nodes, truths = base * 2, truths * 2
        rng = np.random.default_rng([9, n, m])
        hints = np.stack([WC.random_hint(c, rng) for c in nodes])
        with _Handle(engine, nodes) as s:
            cold = _run(engine, s.h, w, hints, False, True, n)
            warm = _run(engine, s.h, w, hints, True, True, n)
        zero = np.flatnonzero(warm["pivots"] == 0)
        rest = np.flatnonzero(warm["pivots"] != 0)
        for i in zero:                                    # the active set the point claims is the truth's
            c = nodes[i]
            got, want = WC.sides_of(warm["z"][i], n), c["side"]
            if not np.array_equal(got[~c["weak"]], want[~c["weak"]]):
                fails.append(f"({n},{m}) [{i}] {c['family']}: accepted with sides {got} against the truth's {want}")
        fails += _check_accepted(nodes, truths, warm, zero, f"({n},{m}) random", e_ref, n)
        diff = _same_bits(cold, warm, rest)
        if diff:
            fails.append(f"({n},{m}): nodes with pivots > 0 differ from the cold call in {diff}")
        accepted += int(np.sum(np.any(warm["z"][zero] != cold["z"][zero], axis=1)))
        declined += rest.size
    assert not fails, "\n".join(fails[:12])
    assert accepted > 0 and declined > 0, (accepted, declined)      # both outcomes occurred


@pytest.mark.parametrize("n,m", [(64, 64), MC.LEADERS])
def test_a_real_sweep_keeps_every_node(engine, oracle, n, m):
    """Cold at w, then w + dw with the previous z as the hint.  Per node, dw is drawn so small that the active set the previous z
    names is still THE active set at w + dw: solve_ref's certificate with those sides at the new parameters.  A node for which
    no dw does (a weakly active row whose multiplier came out of the cold solve as a rounding error) is drawn again."""
    nodes = list(MC.shape(n, m)[4])
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
                nodes[i] = SC.make_node(rng, n, m, c["family"], w0.size, w0)
                again.append(i)
        todo = again
        if not todo:
            break
    assert not todo, [nodes[i]["family"] for i in todo]
    W = np.stack(W)
    assert all(_fits(n, MC.hinted_rows(z, n)) for z in first["z"])
    with _Handle(engine, nodes) as s:
        res = _run(engine, s.h, W, first["z"], True, True, n)
    ref = SC.oracle_solve(oracle, moved, W)
    e_ref = {}
    for c, zo in zip(moved, ref["z"]):
        e_ref[c["family"]] = max(e_ref.get(c["family"], 0.0), SR.node_error(zo, c["_truth"][0], n, SC.row_norm(c)))
    fails = _check_accepted(moved, [c["_truth"] for c in moved], res, range(len(nodes)), f"({n},{m}) sweep", e_ref, n)
    assert not fails, "\n".join(fails[:12])


def test_outside_the_contract_the_cold_bits(engine):
    from qpn_amd import _lib
    from qpn_amd.engine import QpnError
    n = m = 64
    nodes = MC.shape(n, m)[4]
    w = nodes[0]["w"]
    rng = np.random.default_rng(11)
    hints = np.stack([WC.true_hint(c, rng) for c in nodes])
    WARM, COLD = _lib.AVI_FLAG_WARM_DUALS, _lib.AVI_FLAG_COLD_START
    with _Handle(engine, nodes, warm=False) as s:
        cold = _run(engine, s.h, w, hints, False, True, n)
        assert np.all(cold["status"] == 1) and np.any(cold["pivots"] > 0)
        # a handle never opted in
        assert not _same_bits(cold, _run(engine, s.h, w, hints, True, True, n))
        s.h.set_warm(True)
        took = _run(engine, s.h, w, hints, True, True, n)
        assert np.all(took["pivots"] == 0) and np.all(took["status"] == 1)
        # QPN_OPT_MID_ROUTE = 0, QPN_AVI_FLAG_COLD_START
        engine.set_option(_lib.OPT_MID_ROUTE, 0)
        try:
            a, b = _run(engine, s.h, w, hints, False, True, n), _run(engine, s.h, w, hints, True, True, n)
        finally:
            engine.set_option(_lib.OPT_MID_ROUTE, 1)
        assert np.all(a["status"] == 1) and np.any(a["pivots"] > 0) and not _same_bits(a, b), _same_bits(a, b)
        a, b = _run(engine, s.h, w, hints, False, True, n, flags=COLD), _run(engine, s.h, w, hints, False, True, n, flags=COLD | WARM)
        assert np.all(a["status"] == 1) and np.any(a["pivots"] > 0) and not _same_bits(a, b), _same_bits(a, b)
        # a pivot budget that closes the mid route
        a, b = _run(engine, s.h, w, hints, False, True, n, max_pivots=n), _run(engine, s.h, w, hints, True, True, n, max_pivots=n)
        assert np.any(a["pivots"] > 0) and not _same_bits(a, b), _same_bits(a, b)
        # set back to 0
        s.h.set_warm(False)
        assert not _same_bits(cold, _run(engine, s.h, w, hints, True, True, n))
        with pytest.raises(QpnError):
            s.h.set_warm(2)
        assert not _same_bits(cold, _run(engine, s.h, w, hints, True, True, n))
    # per-call records with the flag
    a, b = _run(engine, _abi(nodes), w, hints, False, True, n), _run(engine, _abi(nodes), w, hints, True, True, n)
    assert np.all(a["status"] == 1) and not _same_bits(a, b), _same_bits(a, b)
    # handles of the other classes take the call, and nothing changes
    for (n2, m2), fams in (((32, 32), ("k40", "skew", "k0")), ((160, 140), ("k40", "k1e4"))):
        rng = np.random.default_rng([12, n2, m2])
        w2 = rng.standard_normal(3)
        other = [SC.make_node(rng, n2, m2, f, 3, w2) for f in fams]
        h2 = np.stack([WC.true_hint(c, rng) for c in other])
        with _Handle(engine, other, warm=False) as s:
            before = _run(engine, s.h, w2, h2, True, True, n2)
            s.h.set_warm(True)
            after = _run(engine, s.h, w2, h2, True, True, n2)
            s.h.set_warm(False)
        assert np.all(before["status"] == 1) and not _same_bits(before, after), (n2, m2, _same_bits(before, after))
        assert np.all(before["pivots"] == 0) == ((n2, m2) == (32, 32))


def test_a_record_update_voids_the_old_hint(engine, oracle):
    cls = "wg"
    n, m, p, nodes = SC.cell_cases(cls)[0]
    second = SC.second_plants(cls)
    w = nodes[0]["w"]
    rng = np.random.default_rng(13)
    old = np.stack([WC.true_hint(c, rng) for c in nodes])
    new = np.stack([WC.true_hint(c, rng) for c in second])
    changed = np.array([not np.array_equal(a["side"], b["side"]) for a, b in zip(nodes, second)])
    assert changed.sum() >= len(nodes) // 2
    with _Handle(engine, nodes) as s:
        first = _run(engine, s.h, w, old, True, True, n)
        assert np.all(first["pivots"] == 0) and np.all(first["status"] == 1)
        Q, R, qd, A, B, l, u = SC.stack(second)
        for f, a in (("qd", qd), ("l", l), ("u", u)):
            s.h.update(f, a)
        info0 = s.h.info()
        stale = _run(engine, s.h, w, old, True, True, n)
        fresh = _run(engine, s.h, w, new, True, True, n)
        info1 = s.h.info()
        assert (info0["decline_state"], info0["declined"]) == (info1["decline_state"], info1["declined"]) == (0, 0), (info0, info1)
        cold = _run(engine, s.h, w, old, False, True, n)
        assert np.all(cold["status"] == 1)
        idx = np.flatnonzero(changed)
        assert not _same_bits(cold, stale, idx), _same_bits(cold, stale, idx)
        assert np.all(stale["pivots"][idx] > 0)
        truths = [SC.truth(c) for c in second]
        ref = SC.oracle_solve(oracle, second, w)
        e_ref = {}
        for c, zo, (zt, _) in zip(second, ref["z"], truths):
            e_ref[c["family"]] = max(e_ref.get(c["family"], 0.0), SR.node_error(zo, zt, n, SC.row_norm(c)))
        fails = _check_accepted(second, truths, fresh, range(len(second)), "second plant", e_ref, n)
        assert not fails, "\n".join(fails[:12])


def test_route_switch_through_solve(engine):
    from qpn_amd import algorithm, examples, level_batch
    atol = G.load("simple_bilevel_cases.json")["atol"]
    out = []
    for route in (False, True):
        level_batch.WARM_DUALS_ROUTE = level_batch.WARM_DUALS_MID = route
        try:
            out.append(algorithm.solve(examples.setup("synthetic_pairs", pairs=6, n=36, m=40), engine=engine))
        finally:
            level_batch.WARM_DUALS_ROUTE = level_batch.WARM_DUALS_MID = False
    off, on = out
    assert off["solved"] and on["solved"]
    assert np.allclose(on["x_opt"], off["x_opt"], atol=atol), np.max(np.abs(on["x_opt"] - off["x_opt"]))
