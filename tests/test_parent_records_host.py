"""Inner-node records from a static store, a pool of child pieces and column maps, on the CPU: the numpy twin
level_batch.assemble_parent_records_host is the normative statement of qpn_assemble_parent_nodes, so it is pinned here against
today's host code -- node_record -> (free_equalities) -> batch_records / RecordBatch -- array for array and bit for bit, and the
opt-in wiring (level_batch.PARENT_RECORDS_ROUTE = "device") is driven through a spy engine that the twin serves.  The `-m gpu`
twin of this file is tests/test_gpu_parent_records.py."""
import collections

import numpy as np
import pytest

import qpn_amd  # noqa: F401
from qpn_amd import algorithm, examples, level_batch
from qpn_amd.level_batch import (PR_BAD_COLUMN, PR_BAD_EQ, PR_BAD_INDEX, PR_BAD_MAP, PR_BAD_ROWS, PR_OK, assemble_parent_records_host,
                                 batch_records, free_equalities, node_record, parent_batches)
from qpn_amd.programs import Poly

import parent_cases as PC

INF = np.inf
ARRAYS = ("Qc", "Rc", "qd", "Ac", "Bc", "l", "u")


def same_bits(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def assert_batches_equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g.where, g.n, g.m, g.p, g.nx) == (w.where, w.n, w.m, w.p, w.nx)
        assert np.array_equal(g.m_true, w.m_true) and np.array_equal(g.dec, w.dec) and np.array_equal(g.par, w.par)
        for name in ARRAYS:
            assert same_bits(getattr(g, name), getattr(w, name)), (name, g.where)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("case", PC.CASES, ids=lambda c: c[0])
def test_twin_equals_todays_code(case, form):
    """Every array of the twin's records equals node_record -> (free_equalities) -> batch_records, signs of zeros included."""
    net, items = PC.build(case)
    recs = [node_record(net, pid, ch) for pid, ch in items]
    if form:
        recs = [free_equalities(r) for r in recs]
    want = batch_records(recs)
    eng = PC.TwinEngine()
    got, rest = parent_batches(net, items, eng, form)
    assert rest == [] and eng.n["assemble_parent_nodes"] == len(want)
    assert_batches_equal(got, want)


def test_cases_cover_what_they_claim():
    """The shapes the cases are there for do occur: both sides of ROW_PAD, a padded p, -0.0, +-inf, every equality mix."""
    seen = collections.Counter()
    for case in PC.CASES:
        net, items = PC.build(case)
        for pid, ch in items:
            rec = node_record(net, pid, ch)
            fe = free_equalities(rec)
            seen[f"rows{len(rec['l'])}"] += 1
            seen[f"n0_{rec['dec'].size}"] += 1; seen[f"children{len(ch)}"] += 1
            seen[f"base{len(level_batch._static(net, pid)['l'])}"] += 1
            for P in ch:
                eq = np.isfinite(P.l) & (P.l == P.u)
                seen[f"piece{len(P)}"] += 1
                seen["all_eq"] += bool(len(P) and eq.all()); seen["no_eq"] += bool(len(P) and not eq.any())
                seen["negzero"] += bool(np.any(np.signbit(P.local()[1]) & (P.local()[1] == 0)))
                seen["inf"] += bool(np.any(np.isinf(P.l)) and np.any(np.isinf(P.u)))
            st = level_batch._static(net, pid)
            seen["base_eq"] += bool(np.any(np.isfinite(st["l"]) & (st["l"] == st["u"])))
            seen["solve_m0"] += len(fe["l"]) == 0
        pars = {level_batch._static(net, pid)["par"].size for pid, _ in items}
        seen["p_padded"] += len(pars) > 1
    for key in ("rows16", "rows17", "n0_2", "n0_4", "children1", "children2", "base0", "base3", "piece0", "piece1", "piece5", "all_eq",
                "no_eq", "negzero", "inf", "base_eq", "p_padded"):
        assert seen[key] > 0, key


def test_unread_column_under_zero_coefficients():
    """A piece column the parent does not read maps to -1; under zero coefficients the record is node_record's (whose second
    branch appends the variable as a zero parameter column: the twin's padded p)."""
    net, items = PC.build(PC.CASES[0])
    pid, ch = items[0]
    eng = PC.TwinEngine()
    parent_batches(net, [(pid, ch)], eng, 0)
    for form in (0, 1):
        a = list(eng.args[0]); a[0] = form
        desc, pA, moff, mdat = (np.array(a[k]) for k in (12, 13, 16, 17))
        assert len(desc) == 1 and len(moff) == 2
        r, c = int(desc[0, 1]), int(desc[0, 2])
        A = np.hstack([pA.reshape(r, c), np.zeros((r, 1))])
        desc[0, 2] = c + 1
        cols, _ = ch[0].local()
        extra = net.num_vars - 1                                   # read by nobody, above every parameter of the parent
        wide = Poly.from_sorted(net.num_vars, np.append(cols, extra), A.copy(), ch[0].l, ch[0].u, normalise=False)
        rec = node_record(net, pid, [wide])
        assert rec["par"].size == level_batch._static(net, pid)["par"].size + 1 and rec["par"][-1] == extra
        rec = free_equalities(rec) if form else rec
        (want,) = batch_records([rec])
        a[1], a[2], a[3] = want.n - want.nx, want.m, want.p
        a[12], a[13], a[16], a[17] = desc, A.ravel(), np.array([0, c + 1], np.int32), np.append(mdat, -1).astype(np.int32)
        out = assemble_parent_records_host(*a)
        assert out[7].tolist() == [PR_OK]
        for name, arr in zip(ARRAYS, out):
            assert same_bits(arr[0], getattr(want, name)[0]), (form, name)
        # ... and a non-zero coefficient there makes the item bad
        A[r - 1, c] = 1e-300
        a[13] = A.ravel()
        assert assemble_parent_records_host(*a)[7].tolist() == [PR_BAD_COLUMN]


def test_bad_items_get_their_err():
    net, items = PC.build(PC.CASES[1])
    eng = PC.TwinEngine()
    parent_batches(net, items, eng, 1)
    base = PC.biggest_call(eng)
    good = assemble_parent_records_host(*base)
    assert not good[7].any() and len(good[7]) >= 2
    for name, edit, code in PC.bad_edits(base):
        a = edit([np.array(v) if isinstance(v, np.ndarray) else v for v in base])
        out = assemble_parent_records_host(*a)
        assert out[7][0] == code, (name, out[7])
        assert not out[7][1:].any(), name                             # the neighbours are untouched ...
        for k in range(7):
            assert same_bits(out[k][1:], good[k][1:]), (name, k)
        # ... and the bad item is its parent's static blocks over inert rows
        n0 = base[6].shape[1]
        pa = int(a[18][0])
        Qc, Rc, qd, Ac, Bc, l, u = (o[0] for o in out[:7])
        if 0 <= pa < base[6].shape[0]:
            assert same_bits(Qc[:n0, :n0], base[4][pa]) and same_bits(qd[:n0], base[6][pa])
        else:
            assert not Qc.any() and not qd.any() and not Rc.any()
        assert not Qc[n0:].any() and not Qc[:, n0:].any() and not qd[n0:].any() and not Rc[:, n0:].any()
        assert not Ac.any() and not Bc.any() and np.all(l == -INF) and np.all(u == INF)
    assert {c for _, _, c in PC.bad_edits(base)} == {PR_BAD_INDEX, PR_BAD_MAP, PR_BAD_COLUMN, PR_BAD_ROWS, PR_BAD_EQ}


def _routes(fn):
    out = {}
    for route in ("host", "device"):
        level_batch.PARENT_RECORDS_ROUTE = route
        try:
            out[route] = fn()
        finally:
            level_batch.PARENT_RECORDS_ROUTE = "host"
    return out["host"], out["device"]


def test_wiring_through_a_spy_engine(monkeypatch):
    """verify_items and solve_level on a two-level net with a kink (two pieces for the one child): the device route returns what
    the host route returns, with one assemble call per shape and form, every distinct piece in the pool once, and no per-item
    node_record call."""
    net, x, S = PC.kinked_pairs()
    leaders = sorted(net.network_depth_map[1])
    items = [(pid, [P]) for pid in leaders for P in S[sorted(net.network_edges[pid])[0]]]
    assert len(items) > len(leaders)                                   # a kink: some child has two pieces
    calls = collections.Counter()
    real = level_batch.node_record
    monkeypatch.setattr(level_batch, "node_record", lambda *a, **k: (calls.update(node_record=1), real(*a, **k))[1])

    def verify():
        eng = PC.TwinEngine()
        calls.clear()
        recs, batches, out = level_batch.verify_items(net, items, x, eng)
        return eng, calls["node_record"], [r["pid"] for r in recs], batches, out
    (eh, nh, pids_h, bh, oh), (ed, nd, pids_d, bd, od) = _routes(verify)
    assert nh == len(items) and nd == 0 and pids_h == pids_d
    assert eh.n["assemble_parent_nodes"] == 0 and ed.n["assemble_parent_nodes"] == len(bd) == len(bh)
    assert ed.calls["verify_nodes"] == eh.calls["verify_nodes"]
    for a, b in zip(oh, od):
        assert a["solution"] == b["solution"] and a["path"] == b["path"] and a["e"] == b["e"]
        assert (a["lam"] is None) == (b["lam"] is None) and (a["lam"] is None or same_bits(a["lam"], b["lam"]))
    assert_batches_equal(bd, bh)                                        # (the one download per batch fills the record arrays)
    distinct = {id(P) for _, ch in items for P in ch}
    for a in ed.args:
        assert a[0] == 0 and len(a[12]) == len(distinct)                # the pool: every distinct piece once

    assign = {j: S[j][0] for j in S}

    def solve():
        eng = PC.TwinEngine()
        calls.clear()
        xo = level_batch.solve_level(net, leaders, x, assign, engine=eng)
        return eng, calls["node_record"], xo
    (eh, nh, xh), (ed, nd, xd) = _routes(solve)
    assert nh == len(leaders) and nd == 0
    assert same_bits(xh, xd)
    assert ed.n["assemble_parent_nodes"] == ed.calls["solve_nodes"] == eh.calls["solve_nodes"] >= 1
    assert all(a[0] == 1 and len(a[12]) == len(leaders) for a in ed.args)


def test_items_with_an_unread_column_stay_on_the_host_route(monkeypatch):
    net, x, S = PC.kinked_pairs()
    pid = sorted(net.network_depth_map[1])[0]
    P = S[sorted(net.network_edges[pid])[0]][0]
    cols, A = P.local()
    other = next(v for v in range(net.num_vars) if v not in level_batch._static(net, pid)["reads"])
    order = np.argsort(np.append(cols, other), kind="stable")
    wide = Poly.from_sorted(net.num_vars, np.append(cols, other)[order], np.hstack([A, np.zeros((len(P), 1))])[:, order], P.l, P.u,
                            normalise=False)
    items = [(pid, [P]), (pid, [wide])]

    def verify():
        eng = PC.TwinEngine()
        recs, batches, out = level_batch.verify_items(net, items, x, eng)
        return eng, out
    (eh, oh), (ed, od) = _routes(verify)
    assert ed.n["assemble_parent_nodes"] == 1 and len(ed.args[0][18]) == 1           # one item made on the device, one on the host
    for a, b in zip(oh, od):
        assert a["solution"] == b["solution"] and a["path"] == b["path"]
        assert (a["lam"] is None) == (b["lam"] is None) and (a["lam"] is None or same_bits(a["lam"], b["lam"]))


def test_default_route_is_the_host_route():
    assert level_batch.PARENT_RECORDS_ROUTE == "host"
    net, x, S = PC.kinked_pairs()
    eng = PC.TwinEngine()
    algorithm.solve(net, engine=eng)
    assert eng.n["assemble_parent_nodes"] == 0


def test_simple_bilevel_golden_cases_with_the_route_on():
    """combine_at / solve() on the reference's own end-to-end cases: x is bit-equal with the route on and off."""
    import goldenio as G
    c = G.load("simple_bilevel_cases.json")
    assert len(c["w"]) == 8
    for w in c["w"]:
        x0 = np.array(list(w) + c["x0"], float)

        def run():
            eng = PC.TwinEngine()
            return eng, algorithm.solve(examples.setup("simple_bilevel", gen_solution_map=True), x0, engine=eng)
        (eh, a), (ed, b) = _routes(run)
        assert a["solved"] and b["solved"] and same_bits(a["x_opt"], b["x_opt"]), w
        assert len(a["Sol"][2]) == len(b["Sol"][2])
        assert eh.n["assemble_parent_nodes"] == 0 and ed.n["assemble_parent_nodes"] >= 1
