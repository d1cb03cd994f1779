"""Sweeps that stream the crash cache past the last-level cache (QPN_OPT_LLC_BUDGET_MB; the STREAM instantiations of
csrc/qpn_avi_schur.hip) fetch U', S and the W~ columns with non-temporal loads.  That is a cache policy of the loads and nothing
else, so every output must keep its bits: each sweep here runs on four handles over the same records -- budget -1 (every reuse
sweep streams), budget 0 (none does), QPN_OPT_CRASH_CACHE off, and a fresh handle's first sweep (which fills the cache) -- and all
six outputs are compared with array_equal.  qpn_nodes_info's bit 4 must be set exactly on the sweeps that streamed: reuse sweeps
under budget -1, never a filling sweep, never under budget 0 or with the cache off.

Batches: 96 nodes (the plain reuse instantiation <..., 2>) and 4 500 nodes in natural order (the smallest mixed launch of the
staggered instantiation <..., 3>: launch position = node index).  Each batch holds a node with a NaN in Ad on a reusing position
(Stage A fails it when the cache is filled -- flag 2 -- and it declines in every sweep), a node whose multipliers are all zero
(its read-back requests no column of W~) and one with at least 20 nonzero multipliers; in the mixed launch the last two sit once
on a computing and once on a reusing position.  Six sweeps with different parameters, then a qpn_nodes_update of Qd (the cache
is dropped and refilled) and two more.  Host and device callers."""
import os
import re

import numpy as np
import pytest

import crash_mix_rule as rule
import problems as P

pytestmark = pytest.mark.gpu

KEYS = ("z", "status", "resid", "pivots", "active", "x_out")
N = 32
SWEEPS = 6
OPEN = 1e6
W0 = np.random.default_rng(77).standard_normal(8)
CASES = {"none": ([], lambda nz: len(nz) == 0), "many": (list(range(32)), lambda nz: len(nz) >= 20)}
_cache = {}


def _default_budget():
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quadraticprogramnetworks.jl_amd", "csrc",
                       "qpn_internal.h")
    m = re.search(r"#ifndef QPN_LLC_BUDGET_MB\s*\n#define QPN_LLC_BUDGET_MB\s+(-?\d+)\s*\n#endif", open(src).read())
    assert m
    return int(m.group(1))


def _special_record(node_id, rows):
    """A synthetic node with its constraint bounds opened to +-1e6 and the rows `rows` forced active at W0."""
    Q, R, qd, A, B, l, u = P.synth_node(node_id, N, N, 8)
    l = np.full(N, -OPEN); u = np.full(N, OPEN)
    x0 = -np.linalg.solve(Q, qd + R @ W0)
    s0 = A @ x0 + B @ W0
    for k in rows:
        l[k] = s0[k] + 1.0; u[k] = s0[k] + 2.0
    return Q, R, qd, A, B, l, u


def _specials(oracle):
    """One record per case, confirmed by the CPU oracle before anything runs on the GPU; made once."""
    if "specials" not in _cache:
        out = {}
        for name, (rows, ok) in CASES.items():
            for node_id in range(9000, 9040):
                rec = _special_record(node_id, rows)
                Q, R, qd, A, B, l, u = (c[None] for c in rec)
                M, q, lo, hi, kind = P.reduced_blocks(Q, R, qd, A, B, l, u, W0)
                ref = oracle.solve_avi_batch(M, q, lo, hi, kind=kind)
                if ref["status"][0] == 1 and ok(np.flatnonzero(ref["z"][0, N:] != 0.0)):
                    out[name] = rec
                    break
            assert name in out, f"no candidate node gives the multipliers of case {name}"
        _cache["specials"] = out
    return _cache["specials"]


def _batch(oracle, cnt, where, nan_node):
    from qpn_amd.engine import colmajor
    key = ("base", cnt)
    if key not in _cache:
        _cache[key] = P.synth_nodes(700000 + cnt, cnt, N, N, 8)
    Q, R, qd, A, B, l, u = (c.copy() for c in _cache[key])
    for name, rec in _specials(oracle).items():
        for i in where[name]:
            Q[i], R[i], qd[i], A[i], B[i], l[i], u[i] = rec
    Ac = colmajor(A).copy()
    Ac[nan_node, 7, 19] = np.nan            # column-major Ad: [node][column of x][constraint row]
    return [colmajor(Q), colmajor(R), qd, Ac, colmajor(B), l, u]


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


def _run(engine, oracle, cnt, device, where, nan_node):
    from qpn_amd import _lib
    abi = _batch(oracle, cnt, where, nan_node)
    default = _default_budget()

    def budget(v):
        engine.set_option(_lib.OPT_LLC_BUDGET_MB, v)

    stream, plain, off = (engine.upload_nodes(*abi) for _ in range(3))
    for h in (stream, plain, off):
        h.set_schedule(0)                   # natural order: launch position = node index
    rng = np.random.default_rng(cnt)
    streamed = []

    def sweep(tag, w, recs, fills):
        budget(-1)
        a = _solve(stream, w, device)
        info = stream.info()
        assert info["crash_cached"] and info["crash_streamed"] == (not fills), (tag, info)
        streamed.append(info["crash_streamed"])
        budget(0)
        b = _solve(plain, w, device)
        info = plain.info()
        assert info["crash_cached"] and not info["crash_streamed"], (tag, info)
        _same(a, b, f"{tag}: budget -1 against budget 0")
        budget(-1)
        engine.set_option(_lib.OPT_CRASH_CACHE, 0)
        c = _solve(off, w, device)
        info = off.info()
        engine.set_option(_lib.OPT_CRASH_CACHE, 1)
        assert not info["crash_cached"] and not info["crash_streamed"], (tag, info)
        _same(a, c, f"{tag}: budget -1 against QPN_OPT_CRASH_CACHE = 0")
        fresh = engine.upload_nodes(*recs)
        fresh.set_schedule(0)
        d = _solve(fresh, w, device)
        assert not fresh.info()["crash_streamed"], tag          # (a filling sweep reads no cache)
        fresh.close()
        _same(a, d, f"{tag}: budget -1 against a fresh handle's first sweep")
        return a

    try:
        for s in range(SWEEPS):
            a = sweep(f"sweep {s}", W0 if s == 0 else rng.standard_normal(8), abi, s == 0)
            # the node with the NaN declines (flag 2) and comes back from the general kernel; every other node solves
            assert not np.any(a["status"] == -1)
            ok = np.ones(cnt, bool); ok[nan_node] = False
            assert np.all(a["status"][ok] == 1)
            if s == 0:
                for i in where["none"]:
                    assert np.count_nonzero(a["z"][i, N:]) == 0, i
                for i in where["many"]:
                    assert np.count_nonzero(a["z"][i, N:]) >= 20, i
        engine.synchronize()
        info = stream.info()
        assert (info["decline_state"], info["declined"]) == (3, 1), info
        # an update of Qd drops the cache: the next sweep fills it (and streams nothing), the one after streams again
        Qc = abi[0].copy()
        taken = {nan_node} | {i for v in where.values() for i in v}
        for i in [i for i in range(cnt) if i not in taken][:3] + [cnt - 1]:
            Qc[i] = Qc[i] * 1.25
        new = list(abi); new[0] = Qc
        for h in (stream, plain, off):
            h.update("Qd", Qc)
        assert not stream.info()["crash_cached"]
        for s in range(2):
            sweep(f"after the update, sweep {s}", rng.standard_normal(8), new, s == 0)
        assert streamed == [False] + [True] * (SWEEPS - 1) + [False, True]
    finally:
        budget(default)
        engine.set_option(_lib.OPT_CRASH_CACHE, 1)
        for h in (stream, plain, off):
            h.close()


@pytest.mark.parametrize("device", [False, True])
def test_streamed_plain_reuse_sweeps_96_nodes(engine, oracle, device):
    assert not rule.mixed(96)
    _run(engine, oracle, 96, device, {"none": [14], "many": [71]}, 50)


@pytest.mark.parametrize("device", [False, True])
def test_streamed_mixed_reuse_sweeps_4500_nodes(engine, oracle, device):
    cnt = 4500
    assert rule.mixed(cnt)
    from_ = rule.reuse_from(cnt)
    comp = [p for p in range(16, from_) if rule.recomputes(p, rule.SHARE, from_)]
    reus = [p for p in range(16, from_) if not rule.recomputes(p, rule.SHARE, from_)]
    where = {"none": [comp[3], reus[40], from_ + 7], "many": [comp[len(comp) // 2], reus[len(reus) // 2], cnt - 2]}
    for pos in where.values():
        assert rule.recomputes(pos[0], rule.SHARE, from_) and not rule.recomputes(pos[1], rule.SHARE, from_)
    _run(engine, oracle, cnt, device, where, reus[5])
