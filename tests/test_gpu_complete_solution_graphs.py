"""Uncapped solution graphs on the MI355X: qpn_finish_pieces against its numpy twin (level_batch.finish_pieces_host) bit for bit
on synthetic pieces of every size class, qpn_recipes_batch_range against slices of qpn_recipes_batch, and the CPU file's
counterexample and parity checks on the HIP engine (tests/test_complete_solution_graphs.py)."""
import warnings

import numpy as np
import pytest

import qpn_amd  # noqa: F401
from qpn_amd import algorithm, examples, level_batch
from qpn_amd.avi_solutions import _probe_vector
from qpn_amd.engine import QpnError

pytestmark = pytest.mark.gpu

SIZES = [1, 4, 16, 32, 33, 64, 128, 256]


def synthetic_pieces(n, m, seed=0, pieces=None):
    """reduced_pieces-shaped input with three items: item 0 reads all n + p columns, items 1 and 2 lack padded parameters;
    item 2 misses its point everywhere.  It holds power-of-two scaled copies (duplicates), sign-flipped rows, nearly parallel
    rows (merge), valid all-zero rows (merge) and flagged pieces."""
    g = np.random.default_rng(seed + 97 * n + m)
    p = max(2, n // 2)
    oc, cap = n + p, n + 2 * m
    P = pieces or (36 if cap <= 200 else 14)
    rec_of = (np.arange(P) % 3).astype(np.int32)
    ncols = np.array([oc, oc - 1, max(1, oc - 2)], np.int32)
    take = np.zeros((3, oc), np.int32); xk = np.zeros((3, oc)); probe = np.zeros((3, oc))
    for k in range(3):
        take[k, :ncols[k]] = g.permutation(oc)[:ncols[k]]
        xk[k, :ncols[k]] = g.standard_normal(ncols[k])
        probe[k, :ncols[k]] = _probe_vector(int(ncols[k]))
    Ar = np.zeros((P, oc, cap)); lr = np.full((P, cap), -np.inf); ur = np.full((P, cap), np.inf)
    rows = np.zeros(P, np.int32); flags = np.zeros(P, np.int32)
    for t in range(P):
        k = rec_of[t]; nc = ncols[k]
        r = int(g.integers(1, cap + 1)); rows[t] = r
        A = g.standard_normal((r, nc))
        A[np.abs(A) < 0.05] = 1e-10                         # entries the 1e-8 drop removes
        A *= 10.0 ** g.integers(-4, 3, size=(r, 1))         # rows at any scale
        if r > 2 and t % 6 == 2:
            A[1] = -A[0]                                    # a sign-flipped copy of a row: merge
        if r > 4 and t % 6 == 4:
            A[3] = A[2] * (1 + 1e-11)                       # nearly parallel: merge
        if r > 5 and t % 5 == 1:
            A[5] = 0.0                                      # a valid all-zero row: merge
        ax = A @ xk[k, :nc]
        lo = ax - np.abs(g.standard_normal(r)); hi = ax + np.abs(g.standard_normal(r))
        eq = g.random(r) < 0.3
        lo[eq] = hi[eq] = ax[eq]
        lo[g.random(r) < 0.1] = -np.inf; hi[g.random(r) < 0.1] = np.inf
        if r > 2 and t % 6 == 2:
            lo[1], hi[1] = -hi[0], -lo[0]
        if k == 2:                                          # item 2: the point misses every piece
            lo = np.where(np.isfinite(lo), lo + 1.0 + t, lo); hi = lo + 0.5
        Ar[t][take[k, :nc], :r] = A.T
        lr[t, :r] = lo; ur[t, :r] = hi
        if t % 7 == 6:
            flags[t] = 1
    for t in range(3, P, 6):                                # duplicates: an earlier piece of the same item scaled by 4
        if flags[t - 3] == 0 and rec_of[t] != 2:
            Ar[t] = 4.0 * Ar[t - 3]; lr[t] = 4.0 * lr[t - 3]; ur[t] = 4.0 * ur[t - 3]; rows[t] = rows[t - 3]
    return dict(Ar=Ar, lr=lr, ur=ur, rows=rows, flags=flags, rec_of=rec_of, ncols=ncols, take=take, xk=xk, probe=probe, n=n, m=m)


def _args(d, conv=lambda a: a):
    return (conv(d["Ar"]), conv(d["lr"]), conv(d["ur"]), conv(d["rows"]), conv(d["flags"]), conv(d["rec_of"]), conv(d["ncols"]),
            conv(d["take"]), conv(d["xk"]), conv(d["probe"]), d["n"], d["m"])


def _worst_scale(d):
    """Per piece, the size of what its worst violation sums (|A| |x| and the finite bounds over the valid rows): worst is a
    difference of such terms, in an order numpy does not fix, so it agrees to 1e-13 relative to this."""
    P, _, cap = d["Ar"].shape
    out = np.ones(P)
    for k in range(3):
        plain = np.nonzero((d["rec_of"] == k) & (d["flags"] == 0))[0]
        nc = int(d["ncols"][k])
        _, A3, L2, U2, _, _, _ = level_batch._finish_host(d["Ar"], d["lr"], d["ur"], d["rows"], plain, d["take"][k, :nc],
                                                          d["xk"][k, :nc], d["probe"][k, :nc])
        valid = np.arange(cap)[None, :] < d["rows"][plain][:, None]
        bnd = np.where(valid & np.isfinite(L2), np.abs(L2), 0.0) + np.where(valid & np.isfinite(U2), np.abs(U2), 0.0)
        terms = np.where(valid, np.abs(A3) @ np.abs(d["xk"][k, :nc]), 0.0) + bnd
        out[plain] = np.maximum(1.0, terms.max(axis=1))
    return out


def _check_same(got, ref, scale):
    h = lambda a: np.asarray(a.cpu() if hasattr(a, "cpu") else a)
    assert got["stored"] == ref["stored"]
    assert np.array_equal(h(got["status"]), ref["status"])
    assert np.array_equal(h(got["hash"]).view(np.uint64), ref["hash"])
    assert np.array_equal(h(got["dup_of"]), ref["dup_of"])
    assert np.array_equal(h(got["store_of"]), ref["store_of"])
    for key in ("As", "ls", "us", "rows_s"):
        assert np.array_equal(h(got[key]), ref[key]), key
    w, wr = h(got["worst"]), ref["worst"]
    with np.errstate(invalid="ignore"):                     # (infinite violations: equal on both sides)
        assert np.all((w == wr) | (np.abs(w - wr) <= 1e-13 * scale))


@pytest.mark.parametrize("n", SIZES)
def test_finish_pieces_matches_twin(engine, n):
    import torch
    d = synthetic_pieces(n, n)
    ref = level_batch.finish_pieces_host(*_args(d))
    st = ref["status"]
    # the inputs reach every branch
    assert np.any(st & 1) and np.any(st & 8) and np.any(st & 4) and np.any((st & 2) != 0)
    assert not np.any(st[d["rec_of"] == 2] & 1)
    scale = _worst_scale(d)
    _check_same(engine.finish_pieces(*_args(d)), ref, scale)
    def dev(a):
        a = np.ascontiguousarray(a)
        return torch.as_tensor(a, device="cuda:0")
    _check_same(engine.finish_pieces(*_args(d, dev)), ref, scale)


def test_finish_pieces_mixed_sizes(engine):
    """n != m classes, including both kernel layouts."""
    for n, m in ((1, 4), (4, 1), (16, 40), (33, 64), (64, 16), (128, 256), (256, 128)):
        d = synthetic_pieces(n, m, seed=3)
        _check_same(engine.finish_pieces(*_args(d)), level_batch.finish_pieces_host(*_args(d)), _worst_scale(d))


def test_finish_pieces_bad_arguments(engine):
    d = synthetic_pieces(4, 4)
    a = list(_args(d))
    rec = d["rec_of"].copy(); rec[0] = 3
    with pytest.raises(QpnError):
        engine.finish_pieces(*a[:5], rec, *a[6:])
    tk = d["take"].copy(); tk[0, 0] = d["Ar"].shape[1]
    with pytest.raises(QpnError):
        engine.finish_pieces(*a[:7], tk, *a[8:])
    rows = d["rows"].copy(); rows[0] = d["Ar"].shape[2] + 1
    with pytest.raises(QpnError):
        engine.finish_pieces(*a[:3], rows, *a[4:])
    with pytest.raises(QpnError):                           # cap != n + 2m
        engine.finish_pieces(*a[:10], 4, 5)
    with pytest.raises(QpnError):                           # a store too small
        engine.finish_pieces(*a, store_cap=0)


def test_recipes_batch_range_equals_slices(engine):
    import torch
    g = np.random.default_rng(11)
    masks = g.integers(1, 256, size=(4, 6)).astype(np.uint8)
    tot = [int(np.prod([bin(int(v)).count("1") for v in row])) for row in masks]
    K, node_of = engine.recipes_batch(masks, np.concatenate([[0], np.cumsum(tot)]).astype(np.int64))
    base = np.concatenate([[0], np.cumsum(tot)])
    first = np.array([0, 5, tot[2] - 1, 3], np.int64); cnt = np.array([7, 0, 1, tot[3] - 3], np.int64)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    want = np.concatenate([K[base[b] + first[b]: base[b] + first[b] + cnt[b]] for b in range(4)])
    for mk in (masks, torch.as_tensor(masks, device="cuda:0")):
        K2, no2 = engine.recipes_batch(mk, off, first=first)
        K2 = np.asarray(K2.cpu() if hasattr(K2, "cpu") else K2); no2 = np.asarray(no2.cpu() if hasattr(no2, "cpu") else no2)
        assert np.array_equal(K2, want) and np.array_equal(no2, np.repeat(np.arange(4), cnt))
        with pytest.raises(QpnError):                      # one recipe beyond node 2's product
            engine.recipes_batch(mk, off, first=np.array([0, 5, tot[2], 3], np.int64))
        with pytest.raises(QpnError):
            engine.recipes_batch(mk, off, first=np.array([-1, 0, 0, 0], np.int64))


def test_counterexample_on_hip(engine):
    from test_complete_solution_graphs import counterexample_net
    net, lead, fol = counterexample_net()
    with pytest.warns(UserWarning, match="only the first 64"):
        r = algorithm.solve(net, engine=engine)
    assert r["solved"] and r["truncated"] == [fol] and np.max(np.abs(r["x_opt"])) <= 1e-9
    net, lead, fol = counterexample_net(max_pieces=None)
    r = algorithm.solve(net, engine=engine)
    e7 = np.zeros(7); e7[6] = 1.0
    assert r["solved"] and r["truncated"] == []
    assert np.max(np.abs(r["x_opt"][:7] - e7)) <= 1e-6 and np.max(np.abs(r["x_opt"][7:] - e7)) <= 1e-6


@pytest.mark.parametrize("chunk", [None, 5])
def test_parity_on_hip(engine, chunk):
    from test_complete_solution_graphs import _level, _same_pieces, parity_levels
    for net, players, x in parity_levels(engine):
        recs, batches, rets, want = _level(net, players, x, engine)
        ref = level_batch.solution_pieces(net, recs, batches, rets, x, engine, want, max_pieces=10 ** 9)
        got = level_batch.solution_pieces(net, recs, batches, rets, x, engine, want, max_pieces=None, _chunk=chunk)
        _same_pieces(ref, got)


def test_pairs_40_uncapped(engine):
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*local recipes.*")
        r = algorithm.solve(examples.setup("synthetic_pairs", pairs=40, n=32, m=32, max_pieces=None), engine=engine)
    assert r["solved"] and r["truncated"] == []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = algorithm.solve(examples.setup("synthetic_pairs", pairs=40, n=32, m=32), engine=engine)
    assert c["solved"]
    if not c["truncated"]:
        assert np.max(np.abs(r["x_opt"] - c["x_opt"])) <= 1e-9
