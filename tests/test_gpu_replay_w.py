"""The computing positions of a mixed reuse sweep (crash_mix_rule.py) run the "replay W~" body of the fused symmetric n = m = 32
kernel (csrc/qpn_avi_schur.hip, CRASH == 3): they READ the crash cache -- the flag and the eight panels U' -- and rebuild W~ and
h from them instead of factoring Qd again.  The other mixed-launch suites hold every such position to array_equal against a
handle without the cache and against a fresh handle; this file pins what is specific to a body that reads the cache there:

* a node that declines -- failed pivot test, NaN in Ad, infinity in Ad, equality row -- does so through the stored flag (or, the
  equality row, behind the join) from a replaying position exactly as from a reusing one, and is counted once per sweep;
* the multiplier masks the read-back can meet, on replaying positions, where W~ stays in its tiles (CPU oracle, 1e-9: the parity
  bar of test_gpu_sparse_readback.py);
* both cache policies of the U' loads (QPN_OPT_LLC_BUDGET_MB = -1 and 0) give the same bits;
* an update of Ad or of Qd drops the cache, the next sweep refills it, and no stale panel or stale W~ survives;
* re-sorts of the schedule move nodes between the two kinds of position without a trace;
* the plain reuse instantiation (96 nodes) is what it was.

One batch serves all but the last: 4 500 nodes in natural order (launch position = node index), the smallest launch that takes
the mixed, staggered instantiation.  The first sweep of a handle FILLS the cache (no body reads it), so every run here makes one
sweep more than it checks replays."""
import os
import re

import numpy as np
import pytest

import crash_mix_rule as rule
import problems as P

pytestmark = pytest.mark.gpu

KEYS = ("z", "status", "resid", "pivots", "active", "x_out")
N = 32
CNT = 4500
OPEN = 1e6
W0 = np.random.default_rng(77).standard_normal(8)
# name -> (rows forced active at W0, what the set of nonzero multipliers must look like): the masks of test_gpu_sparse_readback.py
CASES = {
    "none": ([], lambda nz: len(nz) == 0),
    "one_low": ([5], lambda nz: len(nz) == 1 and nz[0] < 16),
    "one_high": ([21], lambda nz: len(nz) == 1 and nz[0] >= 16),
    "line_ends_15_16": ([15, 16], lambda nz: list(nz) == [15, 16]),
    "many": (list(range(32)), lambda nz: len(nz) >= 20),
}
DECLINES = ("pivot", "nan", "inf", "equality")
_cache = {}


def _positions():
    from_ = rule.reuse_from(CNT)
    comp = [p for p in range(16, from_) if rule.recomputes(p, rule.SHARE, from_)]
    reus = [p for p in range(16, from_) if not rule.recomputes(p, rule.SHARE, from_)]
    return comp, reus


def _layout():
    """Where the declining and the special nodes sit: each once on a replaying and once on a reusing position, spread over the
    launch; and the plain nodes the update test changes."""
    comp, reus = _positions()
    decl = {name: [comp[(j * len(comp)) // 4 + 1], reus[(j * len(reus)) // 4 + 1]] for j, name in enumerate(DECLINES)}
    spec = {name: [comp[(j * len(comp)) // 5 + 4], reus[(j * len(reus)) // 5 + 4]] for j, name in enumerate(CASES)}
    taken = {i for v in list(decl.values()) + list(spec.values()) for i in v}
    assert len(taken) == 2 * (len(DECLINES) + len(CASES))
    free_c = [p for p in comp if p not in taken]
    free_r = [p for p in reus if p not in taken]
    upd = {"Ad": [free_c[7], free_r[7]], "Qd": [free_c[len(free_c) // 2], free_r[len(free_r) // 2]]}
    return decl, spec, upd


def _special_record(node_id, rows):
    """A synthetic node with its constraint bounds opened to +-1e6 and the rows `rows` forced active at W0."""
    Q, R, qd, A, B, l, u = P.synth_node(node_id, N, N, 8)
    l = np.full(N, -OPEN); u = np.full(N, OPEN)
    x0 = -np.linalg.solve(Q, qd + R @ W0)
    s0 = A @ x0 + B @ W0
    for k in rows:
        l[k] = s0[k] + 1.0; u[k] = s0[k] + 2.0
    return Q, R, qd, A, B, l, u


def _oracle(oracle, recs, w):
    Q, R, qd, A, B, l, u = (np.stack(c) for c in zip(*recs))
    M, q, lo, hi, kind = P.reduced_blocks(Q, R, qd, A, B, l, u, w)
    return oracle.solve_avi_batch(M, q, lo, hi, kind=kind)


def _specials(oracle):
    """One record per case, confirmed by the CPU oracle before anything runs on the GPU; made once."""
    if "specials" not in _cache:
        out = {}
        for name, (rows, ok) in CASES.items():
            for node_id in range(9000, 9040):
                rec = _special_record(node_id, rows)
                ref = _oracle(oracle, [rec], W0)
                if ref["status"][0] == 1 and ok(np.flatnonzero(ref["z"][0, N:] != 0.0)):
                    out[name] = rec
                    break
            assert name in out, f"no candidate node gives the multipliers of case {name}"
        _cache["specials"] = out
    return _cache["specials"]


def _batch(oracle):
    """Column-major records as the ABI takes them; made once, never written to (the tests copy what they change)."""
    if "batch" not in _cache:
        from qpn_amd.engine import colmajor
        decl, spec, _ = _layout()
        Q, R, qd, A, B, l, u = (c.copy() for c in P.synth_nodes(900000 + CNT, CNT, N, N, 8))
        for name, rec in _specials(oracle).items():
            for i in spec[name]:
                Q[i], R[i], qd[i], A[i], B[i], l[i], u[i] = rec
        for i in decl["pivot"]:             # the first pivot is 1e-6 against the 1e-4 max |M| threshold; Qd stays symmetric
            Q[i, 0, :] = 0.0; Q[i, :, 0] = 0.0; Q[i, 0, 0] = 1e-6
        for i in decl["equality"]:
            u[i, 2] = l[i, 2]
        Ac = colmajor(A).copy()             # column-major Ad: [node][column of x][constraint row]
        for i in decl["nan"]:
            Ac[i, 7, 19] = np.nan           # passes the pivot test (made on H), W~ is not finite
        for i in decl["inf"]:
            Ac[i, 3, 2] = np.inf            # max |M| is infinite: the pivot test itself fails
        _cache["batch"] = [colmajor(Q), colmajor(R), qd, Ac, colmajor(B), l, u]
    return _cache["batch"]


def _np(res):
    return {k: np.array(v.cpu() if hasattr(v, "cpu") else v) for k, v in res.items() if v is not None}


def _solve(nodes, w):
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


def _fresh(engine, abi, w, period=0):
    nodes = engine.upload_nodes(*abi)
    nodes.set_schedule(period)
    out = _solve(nodes, w)
    nodes.close()
    return out


def _pair(engine, abi, period=0):
    nodes = engine.upload_nodes(*abi)
    off = engine.upload_nodes(*abi)
    nodes.set_schedule(period); off.set_schedule(period)
    return nodes, off


def _default_budget():
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quadraticprogramnetworks.jl_amd", "csrc",
                       "qpn_internal.h")
    m = re.search(r"#ifndef QPN_LLC_BUDGET_MB\s*\n#define QPN_LLC_BUDGET_MB\s+(-?\d+)\s*\n#endif", open(src).read())
    assert m
    return int(m.group(1))


def _params(rng, per_node_w):
    return rng.standard_normal((CNT, 8)) if per_node_w else rng.standard_normal(8)


def test_the_launch_mixes_and_every_special_node_sits_on_both_kinds_of_position():
    assert rule.SHARE > 0 and rule.mixed(CNT) and not rule.mixed(rule.RESIDENT)
    from_ = rule.reuse_from(CNT)
    decl, spec, upd = _layout()
    for pos in list(decl.values()) + list(spec.values()) + list(upd.values()):
        assert rule.recomputes(pos[0], rule.SHARE, from_) and not rule.recomputes(pos[1], rule.SHARE, from_)


@pytest.mark.parametrize("per_node_w", [False, True])
def test_declining_nodes_on_replaying_and_reusing_positions(engine, oracle, per_node_w):
    abi = _batch(oracle)
    decl, _, _ = _layout()
    bad = sorted(i for v in decl.values() for i in v)
    nodes, off = _pair(engine, abi)
    rng = np.random.default_rng(31 + per_node_w)
    try:
        for sweep in range(5):              # the first fills the cache; four read it
            w = _params(rng, per_node_w)
            a = _solve(nodes, w)
            engine.synchronize()
            info = nodes.info()
            assert info["crash_cached"] and not info["crash_refused"] and not info["scheduled"], info
            # (decline_state 3: the handle knows how many nodes decline and launches the general kernel behind every sweep)
            assert (info["decline_state"], info["declined"]) == (3, len(bad)), (sweep, info)
            with _uncached(engine):
                b = _solve(off, w)
                assert not off.info()["crash_cached"]
            _same(a, b, f"sweep {sweep} against QPN_OPT_CRASH_CACHE = 0")
            _same(a, _fresh(engine, abi, w), f"sweep {sweep} against a fresh handle's first sweep")
            # the declining nodes came back from the general kernel, never as -1; every other node solved
            assert not np.any(a["status"] == -1), np.flatnonzero(a["status"] == -1)
            ok = np.ones(CNT, bool); ok[bad] = False
            assert np.all(a["status"][ok] == 1)
    finally:
        nodes.close(); off.close()


def test_multiplier_masks_on_replaying_positions_against_the_oracle(engine, oracle):
    abi = _batch(oracle)
    _, where, _ = _layout()
    spec = _specials(oracle)
    names = list(spec)
    nodes, off = _pair(engine, abi)
    rng = np.random.default_rng(CNT)
    masks = set()
    try:
        for sweep in range(5):
            w = W0 if sweep < 2 else rng.standard_normal(8)        # (sweep 0 fills; sweep 1 replays at W0, the designed masks)
            a = _solve(nodes, w)
            assert nodes.info()["crash_cached"]
            with _uncached(engine):
                b = _solve(off, w)
            _same(a, b, f"sweep {sweep} against QPN_OPT_CRASH_CACHE = 0")
            ref = _oracle(oracle, [spec[nm] for nm in names], w)
            for j, nm in enumerate(names):
                for i in where[nm]:
                    assert a["status"][i] == 1 == ref["status"][j], (sweep, nm, i)
                    err = np.max(np.abs(a["z"][i] - ref["z"][j]))
                    print(f"sweep {sweep} {nm} node {i}: max |dz| against the oracle {err:.2e}")
                    assert err <= 1e-9, (sweep, nm, i, err)
                    assert np.array_equal(a["z"][i, N:] != 0.0, ref["z"][j, N:] != 0.0), (sweep, nm, i)
                    if sweep == 1:
                        assert CASES[nm][1](np.flatnonzero(a["z"][i, N:] != 0.0)), (nm, i)
            masks.add((a["z"][:, N:] != 0.0).tobytes())
        assert len(masks) == 4              # W0 twice, then the masks changed from sweep to sweep
    finally:
        nodes.close(); off.close()


@pytest.mark.parametrize("per_node_w", [False, True])
def test_both_cache_policies_of_the_panel_loads_give_the_same_bits(engine, oracle, per_node_w):
    from qpn_amd import _lib
    abi = _batch(oracle)
    default = _default_budget()
    stream, plain = _pair(engine, abi)
    off = engine.upload_nodes(*abi)
    off.set_schedule(0)
    rng = np.random.default_rng(53 + per_node_w)
    try:
        for sweep in range(5):
            w = _params(rng, per_node_w)
            engine.set_option(_lib.OPT_LLC_BUDGET_MB, -1)
            a = _solve(stream, w)
            info = stream.info()
            assert info["crash_cached"] and info["crash_streamed"] == (sweep > 0), (sweep, info)      # (a filling sweep reads no cache)
            engine.set_option(_lib.OPT_LLC_BUDGET_MB, 0)
            b = _solve(plain, w)
            info = plain.info()
            assert info["crash_cached"] and not info["crash_streamed"], (sweep, info)
            _same(a, b, f"sweep {sweep}: budget -1 against budget 0")
            with _uncached(engine):
                c = _solve(off, w)
                assert not off.info()["crash_streamed"]
            _same(a, c, f"sweep {sweep}: budget -1 against QPN_OPT_CRASH_CACHE = 0")
    finally:
        engine.set_option(_lib.OPT_LLC_BUDGET_MB, default)
        engine.set_option(_lib.OPT_CRASH_CACHE, 1)
        for h in (stream, plain, off):
            h.close()


def test_updates_of_ad_and_qd_drop_the_cache_and_leave_nothing_stale(engine, oracle):
    abi = list(_batch(oracle))
    _, _, upd = _layout()
    nodes = engine.upload_nodes(*abi)
    nodes.set_schedule(0)
    rng = np.random.default_rng(67)
    try:
        for sweep in range(2):              # fill, then one sweep that reads the cache
            w = rng.standard_normal(8)
            _same(_solve(nodes, w), _fresh(engine, abi, w), f"before the updates, sweep {sweep}")
        assert nodes.info()["crash_cached"]
        for field, index in (("Ad", 3), ("Qd", 0)):
            new = abi[index].copy()
            for i in upd[field]:            # one node on a replaying, one on a reusing position (Qd stays symmetric, positive definite)
                new[i] = new[i] * 1.25
            abi[index] = new
            nodes.update(field, new)
            assert not nodes.info()["crash_cached"], field
            for sweep in range(4):          # the refill, then three sweeps on the new panels and the new W~
                w = rng.standard_normal(8)
                a = _solve(nodes, w)
                assert nodes.info()["crash_cached"], (field, sweep)
                _same(a, _fresh(engine, abi, w), f"after the update of {field}, sweep {sweep} against a fresh handle")
    finally:
        nodes.close()


def test_scheduled_sweeps_move_nodes_between_the_bodies(engine, oracle):
    abi = _batch(oracle)
    nodes, off = _pair(engine, abi, 16)
    rng = np.random.default_rng(71)
    try:
        for sweep in range(40):
            w = rng.standard_normal(8)
            a = _solve(nodes, w)
            assert nodes.info()["crash_cached"]
            with _uncached(engine):
                b = _solve(off, w)
            _same(a, b, f"scheduled sweep {sweep} against QPN_OPT_CRASH_CACHE = 0")
        assert nodes.info()["scheduled"] and off.info()["scheduled"]
    finally:
        nodes.close(); off.close()


def test_plain_reuse_96_nodes_is_unchanged(engine):
    from qpn_amd.engine import colmajor
    assert not rule.mixed(96)
    Q, R, qd, A, B, l, u = P.synth_nodes(900096, 96, N, N, 8)
    abi = [colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u]
    nodes, off = _pair(engine, abi)
    rng = np.random.default_rng(96)
    try:
        for sweep in range(4):
            w = rng.standard_normal(8)
            a = _solve(nodes, w)
            assert nodes.info()["crash_cached"]
            with _uncached(engine):
                b = _solve(off, w)
            _same(a, b, f"sweep {sweep} against QPN_OPT_CRASH_CACHE = 0")
            assert np.all(a["status"] == 1)
    finally:
        nodes.close(); off.close()
