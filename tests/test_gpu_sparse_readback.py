"""Reuse sweeps of the fused symmetric n = m = 32 kernel fetch W~ after the pivot loop, column by column, and only the columns
whose multiplier is not zero (csrc/qpn_internal.h, crash_w_index; the read-back of csrc/qpn_avi_schur.hip).  A skipped column
stands in the product x = W~ lambda - h as +0.0, so every output must keep its bits: each sweep here is compared -- array_equal
-- with the same sweep of a handle whose crash cache is off (which computes W~ and multiplies all of it) and with the first
sweep of a fresh handle (which fills the cache), and the special nodes with the CPU oracle (1e-9, the parity bar of smoke()).

The special nodes pin the masks the read-back can meet.  They are synthetic nodes whose constraint bounds are opened to +-1e6
and whose chosen rows k are then forced active: with x0 = -H^-1 g the unconstrained minimiser and s0 = A x0 + B w, row k gets
[l_k, u_k] = [s0_k + 1, s0_k + 2].  The oracle confirms, before anything runs on the GPU, that their nonzero multipliers are:
none; exactly one in a column < 16; exactly one in a column >= 16; several, all in columns < 16; several, all in columns >= 16;
two at the ends of a tile's lines (lc = 15 and lc = 0: columns 15 and 16, and columns 0 and 31); at least 20.  Every sweep takes
another parameter vector, so the active sets of all nodes -- and with them the masks -- change from sweep to sweep.

Batches: 96 nodes (the plain reuse instantiation) and 4 500 nodes in natural order (the mixed, staggered instantiation: launch
position = node index), where every special node sits once on a computing and once on a reusing position of crash_mix_rule."""
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

# name -> (rows forced active, what the set of nonzero multipliers must look like)
CASES = {
    "none": ([], lambda nz: len(nz) == 0),
    "one_low": ([5], lambda nz: len(nz) == 1 and nz[0] < 16),
    "one_high": ([21], lambda nz: len(nz) == 1 and nz[0] >= 16),
    "all_low": ([1, 4, 9, 14], lambda nz: len(nz) >= 2 and all(k < 16 for k in nz)),
    "all_high": ([17, 22, 30], lambda nz: len(nz) >= 2 and all(k >= 16 for k in nz)),
    "line_ends_15_16": ([15, 16], lambda nz: list(nz) == [15, 16]),
    "line_ends_0_31": ([0, 31], lambda nz: list(nz) == [0, 31]),
    "many": (list(range(32)), lambda nz: len(nz) >= 20),
}
_cache = {}


def _special_record(node_id, rows):
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
    """The special records, one per case, found among a few candidate node ids with the oracle (CPU only); made once."""
    if "specials" not in _cache:
        out = {}
        for name, (rows, ok) in CASES.items():
            for node_id in range(9000, 9040):
                rec = _special_record(node_id, rows)
                ref = _oracle(oracle, [rec], W0)
                nz = np.flatnonzero(ref["z"][0, N:] != 0.0)
                if ref["status"][0] == 1 and ok(nz):
                    out[name] = rec
                    break
            assert name in out, f"no candidate node gives the multipliers of case {name}"
        _cache["specials"] = out
    return _cache["specials"]


def _batch(oracle, cnt, where):
    """Column-major records of `cnt` synthetic nodes with the special records at the node indices where[name] (lists)."""
    from qpn_amd.engine import colmajor
    key = ("base", cnt)
    if key not in _cache:
        _cache[key] = P.synth_nodes(500000 + cnt, cnt, N, N, 8)
    Q, R, qd, A, B, l, u = (c.copy() for c in _cache[key])
    for name, rec in _specials(oracle).items():
        for i in where[name]:
            Q[i], R[i], qd[i], A[i], B[i], l[i], u[i] = rec
    return [colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u]


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


def _fresh(engine, abi, w):
    nodes = engine.upload_nodes(*abi)
    nodes.set_schedule(0)
    out = _solve(nodes, w)
    nodes.close()
    return out


def _run(engine, oracle, cnt, where):
    spec = _specials(oracle)
    names = list(spec)
    abi = _batch(oracle, cnt, where)
    nodes = engine.upload_nodes(*abi)
    off = engine.upload_nodes(*abi)
    nodes.set_schedule(0); off.set_schedule(0)      # natural order: launch position = node index
    rng = np.random.default_rng(cnt)
    masks = set()

    def sweep(tag, w, recs):
        a = _solve(nodes, w)
        assert nodes.info()["crash_cached"]
        with _uncached(engine):
            b = _solve(off, w)
            assert not off.info()["crash_cached"]
        _same(a, b, f"{tag} against QPN_OPT_CRASH_CACHE = 0")
        _same(a, _fresh(engine, list(recs), w), f"{tag} against a fresh handle's first sweep")
        ref = _oracle(oracle, [spec[nm] for nm in names], w)
        for j, nm in enumerate(names):
            for i in where[nm]:
                assert a["status"][i] == 1 == ref["status"][j], (tag, nm, i)
                err = np.max(np.abs(a["z"][i] - ref["z"][j]))
                assert err <= 1e-9, (tag, nm, i, err)
                assert np.array_equal(a["z"][i, N:] != 0.0, ref["z"][j, N:] != 0.0), (tag, nm, i)
        masks.add((a["z"][:, N:] != 0.0).tobytes())
        return a

    for s in range(SWEEPS):
        sweep(f"sweep {s}", W0 if s == 0 else rng.standard_normal(8), abi)
    assert len(masks) == SWEEPS                     # the multipliers' masks did change from sweep to sweep
    # an update of Qd drops the cache; the next sweep refills it in the same layout
    Qc = abi[0].copy()
    changed = [i for i in range(cnt) if all(i not in v for v in where.values())][:3] + [cnt - 1]
    for i in changed:
        Qc[i] = Qc[i] * 1.25
    new = list(abi); new[0] = Qc
    nodes.update("Qd", Qc); off.update("Qd", Qc)
    assert not nodes.info()["crash_cached"]
    for s in range(2):
        sweep(f"after the update, sweep {s}", rng.standard_normal(8), new)
    nodes.close(); off.close()


def _nonfinite_run(engine, oracle, cnt, nan_nodes, inf_node):
    """A NaN in Ad passes the pivot test (it is made on H, and max |M| ignores a NaN) and makes W~ not finite, where skipping a
    column of W~ would not give the bits of the full product.  Stage A of every symmetric variant -- computing, filling, mixed --
    therefore fails such a node like one that failed the pivot test: it declines in EVERY sweep, from either kind of position, is
    counted by the handle on its first sweep, and comes back from the general kernel -- never as status -1, and with the same bits
    from a reuse sweep, from a handle with the cache off and from a fresh handle.  An infinity in Ad makes max |M| infinite: the
    pivot test itself fails, in every sweep alike."""
    where = {name: [] for name in CASES}
    abi = _batch(oracle, cnt, where)
    A = abi[3].copy()                       # column-major Ad: [node][column of x][constraint row]
    for i in nan_nodes:
        A[i, 7, 19] = np.nan
    if inf_node is not None:
        A[inf_node, 3, 2] = np.inf
    abi[3] = A
    nodes = engine.upload_nodes(*abi)
    off = engine.upload_nodes(*abi)
    nodes.set_schedule(0); off.set_schedule(0)
    rng = np.random.default_rng(7 + cnt)
    for s in range(4):
        w = rng.standard_normal(8)
        a = _solve(nodes, w)
        engine.synchronize()
        info = nodes.info()
        # (decline_state 3: the handle knows how many nodes decline, and launches the general kernel behind every sweep)
        want = len(nan_nodes) + (0 if inf_node is None else 1)
        assert info["crash_cached"] and (info["decline_state"], info["declined"]) == (3, want), info
        with _uncached(engine):
            b = _solve(off, w)
        _same(a, b, f"sweep {s} against QPN_OPT_CRASH_CACHE = 0")
        _same(a, _fresh(engine, abi, w), f"sweep {s} against a fresh handle's first sweep")
        assert not np.any(a["status"] == -1), np.flatnonzero(a["status"] == -1)
        ok = np.ones(cnt, bool); ok[list(nan_nodes)] = False
        if inf_node is not None:
            ok[inf_node] = False
        assert np.all(a["status"][ok] == 1)
    nodes.close(); off.close()


def test_a_node_whose_w_is_not_finite_declines_in_every_sweep_96_nodes(engine, oracle):
    _nonfinite_run(engine, oracle, 96, [50], None)
    _nonfinite_run(engine, oracle, 96, [50], 61)


def test_a_node_whose_w_is_not_finite_declines_in_every_sweep_4500_nodes(engine, oracle):
    cnt = 4500
    from_ = rule.reuse_from(cnt)
    comp = [p for p in range(16, from_) if rule.recomputes(p, rule.SHARE, from_)]
    reus = [p for p in range(16, from_) if not rule.recomputes(p, rule.SHARE, from_)]
    _nonfinite_run(engine, oracle, cnt, [comp[5], reus[5], cnt - 3], reus[9])


def test_the_oracle_confirms_the_special_nodes(oracle):
    spec = _specials(oracle)
    assert set(spec) == set(CASES)
    counts = {}
    for name, rec in spec.items():
        nz = np.flatnonzero(_oracle(oracle, [rec], W0)["z"][0, N:] != 0.0)
        assert CASES[name][1](nz), (name, nz)
        counts[name] = len(nz)
    assert counts["none"] == 0 and counts["one_low"] == 1 and counts["one_high"] == 1 and counts["many"] >= 20


def test_plain_reuse_sweeps_96_nodes(engine, oracle):
    assert not rule.mixed(96)
    where = {name: [3 + 11 * j] for j, name in enumerate(CASES)}
    _run(engine, oracle, 96, where)


def test_mixed_reuse_sweeps_4500_nodes(engine, oracle):
    cnt = 4500
    assert rule.mixed(cnt)
    from_ = rule.reuse_from(cnt)
    comp = [p for p in range(16, from_) if rule.recomputes(p, rule.SHARE, from_)]
    reus = [p for p in range(16, from_) if not rule.recomputes(p, rule.SHARE, from_)]
    assert len(comp) >= len(CASES) and len(reus) >= len(CASES)
    # one copy on a computing position, one on a reusing position of the mixed part, spread over the launch; the first and the
    # last case also in the reuse-only tail
    where = {}
    for j, name in enumerate(CASES):
        where[name] = [comp[(j * len(comp)) // len(CASES)], reus[(j * len(reus)) // len(CASES)]]
    where["none"].append(from_ + 7)
    where["many"].append(cnt - 2)
    for name, pos in where.items():
        assert rule.recomputes(pos[0], rule.SHARE, from_) and not rule.recomputes(pos[1], rule.SHARE, from_)
    _run(engine, oracle, cnt, where)
