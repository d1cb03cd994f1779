"""polyhedra_host.irredundant_bounds_host, the normative statement of qpn_irredundant_bounds, against references that share no code
with it: planted answers, HiGHS on the pieces the feature is for (irredundant_cases.check_as_sets), wrong methods that the checks
must catch; then polyhedra.irredundant_batch and solve() with QPNetOptions.irredundant_pieces on the twin engine."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import irredundant_cases as ic
from irredundant_cases import INF

import qpn_amd  # noqa: F401
from qpn_amd import algorithm, examples, polyhedra
from qpn_amd import polyhedra_host as ph
from qpn_amd.engine import colmajor
from qpn_amd.programs import Poly
from twin_engine import TwinEngine

OK, EMPTY, ITER_LIMIT = ph.IB_OK, ph.IB_EMPTY, ph.IB_ITER_LIMIT
UNDECIDED, NONE, KEPT_EQUALITY, REMOVED_ZERO_ROW = ph.RED_UNDECIDED, ph.RED_NONE, ph.RED_KEPT_EQUALITY, ph.RED_REMOVED_ZERO_ROW
KEPT_UNBOUNDED, KEPT_BY_OPTIMUM, REMOVED = ph.RED_KEPT_UNBOUNDED, ph.RED_KEPT_BY_OPTIMUM, ph.RED_REMOVED
SEEDS = range(30)


RedTwinEngine = ic.red_twin_engine


def _one(A, l, u, **kw):
    out = ph.irredundant_bounds_host(colmajor(A[None]), l[None], u[None], **kw)
    return {k: v[0] for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _planted(shape):
    """The twin on the family at `shape`, once: -> (the batch, the twin's output)."""
    batch = ic.planted_batch(shape, SEEDS)
    return batch, ph.irredundant_bounds_host(colmajor(batch[0]), batch[1], batch[2])


@functools.lru_cache(maxsize=None)
def _pieces():
    return [(name, A, l, u, _one(A, l, u)) for name, A, l, u in ic.pieces()]


# ---- 1. planted answers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1)] + ic.PLANTED_SHAPES)
def test_exactly_the_planted_bounds_go(shape):
    (A, l, u), out = _planted(shape)
    r = A.shape[1]
    assert np.all(out["status"] == OK) and np.all(out["fail_row"] == -1)
    assert np.array_equal(out["lr"], l)
    want = u.copy(); want[:, r - 3:] = INF
    assert np.array_equal(out["ur"], want)                                          # the appended copy goes, row 0 itself stays
    zero = shape == (1, 1)                                                          # 0.5 (a_1 + a_0) is the zero row there
    assert np.all(np.delete(out["how"][:, :, 0], r - 2, axis=1) == NONE)
    assert np.all(out["how"][:, r - 2, 0] == (REMOVED_ZERO_ROW if zero else NONE))  # (an all-zero row: both sides, infinite or not)
    assert np.all(np.isin(out["how"][:, :r - 3, 1], (KEPT_BY_OPTIMUM, KEPT_UNBOUNDED)))   # (without a facet the set may be unbounded)
    assert np.all((out["how"][:, :, 1] == KEPT_UNBOUNDED) == (out["ext"][:, :, 1] == INF))
    assert np.all(out["how"][:, r - 2, 1] == (REMOVED_ZERO_ROW if zero else REMOVED))
    assert np.all(out["how"][:, [r - 3, r - 1], 1] == REMOVED)
    assert np.all(np.isnan(out["ext"][:, :, 0]))
    lp_ran = out["how"][:, :, 1] != REMOVED_ZERO_ROW
    assert np.all(~np.isnan(out["ext"][:, :, 1]) == lp_ran)
    assert np.all(out["lps"] == 1 + r - (1 if zero else 0)) and np.all(out["iters"] >= 0)
    # a facet is passed by a wide margin without its bound, a planted bound by none: no verdict hangs on the tolerance
    gap = out["ext"][:, :, 1] - u
    assert np.all(gap[:, :r - 3] > 1e-6) and np.all(gap[:, r - 3:][lp_ran[:, r - 3:]] <= 1e-10)


def test_the_planted_family_as_sets_and_the_constant():
    """Check 2 on the planted family (none of its bounds may be left out), the hand cases and the pieces; the twin's worst
    violation of a removed bound is what irredundant_cases says it is, to within a factor of 2."""
    worst = 0.0
    for shape in ic.PLANTED_SHAPES:
        (A, l, u), out = _planted(shape)
        for k in SEEDS:
            w, left_out, _ = ic.check_as_sets(A[k], l[k], u[k], out["lr"][k], out["ur"][k], max_left_out=0.0)
            worst = max(worst, w)
    for name, A, l, u, out in _pieces():
        if out["status"] == OK:
            worst = max(worst, ic.check_as_sets(A, l, u, out["lr"], out["ur"])[0])
    print(f"the twin's worst violation of a removed bound: {worst:.4g} (TWIN_WORST {ic.TWIN_WORST:.4g}, TAU {ic.TAU:.4g})")
    assert ic.TWIN_WORST / 2 <= worst <= 2 * ic.TWIN_WORST and ic.TAU == 1000 * ic.TWIN_WORST


def test_hand_cases():
    A, l, u = ic.hand_batch()
    out = ph.irredundant_bounds_host(colmajor(A), l, u)
    got = {name: {k: v[t] for k, v in out.items()} for t, name in enumerate(ic.HAND)}
    inf = INF
    g = got["equality"]                                     # the equality stays, both box bounds of x0 are implied by it
    assert g["status"] == OK and g["how"].tolist() == [[KEPT_EQUALITY] * 2, [KEPT_UNBOUNDED] * 2, [REMOVED] * 2, [NONE, REMOVED]]
    assert g["lr"].tolist() == [1.0, -1.0, -inf, -inf] and g["ur"].tolist() == [1.0, 1.0, inf, inf]
    assert np.isnan(g["ext"][0]).all() and g["ext"][2].tolist() == [1.0, 1.0] and g["lps"] == 6
    g = got["zero row"]
    assert g["status"] == OK and g["how"][2].tolist() == [REMOVED_ZERO_ROW] * 2 and np.isnan(g["ext"][2]).all()
    assert g["lr"].tolist() == [-1.0, -1.0, -inf, -inf] and g["ur"].tolist() == [1.0, 1.0, inf, 1.0]
    g = got["one side"]                                     # -5 <= x0 + x1 goes (the box reaches -2), x0 + x1 <= 1 stays
    assert g["status"] == OK and g["how"][3].tolist() == [REMOVED, KEPT_BY_OPTIMUM] and g["ext"][3].tolist() == [-2.0, 2.0]
    assert g["lr"].tolist() == [-1.0, -1.0, -inf, -inf] and g["ur"].tolist() == [1.0, 1.0, inf, 1.0]
    g = got["unbounded"]
    assert g["status"] == OK and g["how"][3].tolist() == [NONE, KEPT_UNBOUNDED] and g["ext"][3, 1] == inf
    assert g["ur"].tolist() == [1.0, inf, inf, 4.0]
    for name, lps in (("empty", 1), ("crossed", 0)):        # the input back, nothing decided
        g = got[name]
        t = list(ic.HAND).index(name)
        assert g["status"] == EMPTY and g["fail_row"] == -1 and g["lps"] == lps
        assert np.array_equal(g["lr"], l[t]) and np.array_equal(g["ur"], u[t])
        assert np.all(g["how"] == UNDECIDED) and np.isnan(g["ext"]).all()
    for t, name in enumerate(ic.HAND):                      # ... and HiGHS agrees on the ones that have a point
        if got[name]["status"] == OK:
            ic.check_as_sets(A[t], l[t], u[t], got[name]["lr"], got[name]["ur"], max_left_out=0.0)
        else:
            assert ic.highs_min(A[t], l[t], u[t], np.zeros(2)) is None


def test_an_iteration_limit_gives_the_input_back():
    """max_iters = 1: "one side" starts at the corner (-1, -1), which is feasible (0 steps) and the minimum of row 3 (0 steps, its
    lower bound REMOVED); the maximum of row 3 needs two steps.  ITER_LIMIT with fail_row = 3, and the removal is no verdict any more."""
    A, l, u = ic.HAND["one side"]
    g = _one(A, l, u, opts=dict(max_iters=1))
    assert g["status"] == ITER_LIMIT and g["fail_row"] == 3 and g["lps"] == 3 and g["iters"] == 1
    assert np.array_equal(g["lr"], l) and np.array_equal(g["ur"], u)
    assert np.all(g["how"] == UNDECIDED)
    assert g["ext"][3, 0] == -2.0 and np.isnan(g["ext"][3, 1])
    full = _one(A, l, u)
    assert full["status"] == OK and full["how"][3, 0] == REMOVED
    # over a family: some end in the feasibility solve (fail_row -1), some in a row's solve; every one of them returns its input
    (A, l, u), _ = _planted((16, 8))
    cut = ph.irredundant_bounds_host(colmajor(A), l, u, opts=dict(max_iters=1))
    bad = cut["status"] != OK
    assert np.all(cut["status"][bad] == ITER_LIMIT) and bad.any()
    assert np.array_equal(cut["lr"][bad], l[bad]) and np.array_equal(cut["ur"][bad], u[bad])
    assert not np.isin(cut["how"][bad], (REMOVED, REMOVED_ZERO_ROW)).any()


def test_a_nonbasic_row_outside_its_restored_bound_takes_the_bound():
    """1 (d) on a state made by hand (the loop does not make it: irredundant_bounds_host's docstring says why).  The unit box after
    the feasibility solve: both s nonbasic at -1.  Row 0's lower bound is relaxed, its s pushed to -3 as a solve might have left
    it, and restored: it sits at -1 again and the next solve ends OPTIMAL there.  Without the rule the point violates the restored
    bound for good and the solve is a FAILURE."""
    A = np.eye(2); l = np.array([-1.0, -1.0]); u = np.array([1.0, 1.0])
    for rule in (True, False):
        lw, uw = l.copy(), u.copy()
        status, S, _ = ph._lp_feasible(A, lw, uw, dict(ph.LP_DEFAULT_OPTS))
        assert status == ph.LP_OPTIMAL and sorted(S.cn.tolist()) == [2, 3] and S.xn.tolist() == [-1.0, -1.0]
        j = S.cn.tolist().index(2)
        ph._red_relax(S, lw, uw, 0, 0)
        assert lw[0] == -INF and S.ls[0] == -INF and S.xn[j] == -1.0
        S.xn[j] = -3.0
        if rule:
            ph._red_restore(S, lw, uw, 0, 0, -1.0)
            assert S.xn[j] == -1.0
        else:
            lw[0] = -1.0; S.ls[0] = -1.0
        assert lw[0] == -1.0 and S.ls[0] == -1.0
        status, x, obj = ph._lp_resolve(S, np.array([0.0, 1.0]))
        if rule:
            assert status == ph.LP_OPTIMAL and obj == -1.0 and x.tolist() == [-1.0, -1.0]
        else:
            assert status == ph.LP_FAILURE
    # the upper side, and a value inside the restored bound, which stays
    lw, uw = l.copy(), u.copy()
    _, S, _ = ph._lp_feasible(A, lw, uw, dict(ph.LP_DEFAULT_OPTS))
    j = S.cn.tolist().index(3)
    ph._red_relax(S, lw, uw, 1, 1); S.xn[j] = 2.5; ph._red_restore(S, lw, uw, 1, 1, 1.0)
    assert S.xn[j] == 1.0 and uw[1] == 1.0 and S.us[1] == 1.0
    ph._red_relax(S, lw, uw, 1, 1); S.xn[j] = 0.25; ph._red_restore(S, lw, uw, 1, 1, 1.0)
    assert S.xn[j] == 0.25


# ---- 2. as sets, on the pieces the feature is for ----------------------------------------------------------------------------------
# rows before -> after, as HiGHS pruning from the last row to the first gives them too; the two pieces that stay are EMPTY (HiGHS
# agrees: no point), so nothing of them is pruned and they come back as they went in.  "64-65-2/2" is the input of the first
# Fourier-Motzkin step of the piece that grows to 1101 rows, beyond the kernel's 1024.
ROWS = {"5-6-3/0": (11, 10), "5-6-3/1": (10, 10), "5-6-3/2": (15, 9), "40-33-3/0": (73, 73), "40-33-3/1": (72, 49),
        "64-65-2/0": (129, 70), "64-65-2/1": (128, 68), "64-65-2/2 (first step's input)": (130, 130), "pairs/0": (11, 11),
        "scaled/0": (11, 10)}


def test_the_projected_pieces_as_sets():
    got = _pieces()
    assert [name for name, *_ in got] == list(ROWS)
    for name, A, l, u, out in got:
        assert (ic.rows_left(l, u), ic.rows_left(out["lr"], out["ur"])) == ROWS[name], name
        if ROWS[name][0] == ROWS[name][1] and name not in ("5-6-3/1", "pairs/0"):
            assert out["status"] == EMPTY and ic.highs_min(A, l, u, np.zeros(A.shape[1])) is None, name
            assert np.array_equal(out["lr"], l) and np.array_equal(out["ur"], u)
        else:
            assert out["status"] == OK, name
            ic.check_as_sets(A, l, u, out["lr"], out["ur"])


# ---- 3. wrong methods must fail ---------------------------------------------------------------------------------------------------
def test_the_restated_method_is_the_twin():
    for A, l, u in [ic.planted(8, 4, s)[:3] for s in range(4)] + [p[1:] for p in ic.pieces()[:3]]:
        lr, ur = ic.irredundant_with(None, A, l, u)
        out = _one(A, l, u)
        assert np.array_equal(lr, out["lr"]) and np.array_equal(ur, out["ur"])


@pytest.mark.parametrize("bug", ic.BUGS)
def test_a_wrong_method_is_caught(bug):
    """Each mutation fails the planted answer, and check 2 says why: "all at once" and "not restored" remove a bound the final set
    passes, "tolerance reversed" keeps a bound the others imply."""
    A, l, u, planted = ic.planted(8, 4, 0)
    lr, ur = ic.irredundant_with(bug, A, l, u)
    gone = np.nonzero(~np.isfinite(ur))[0].tolist()
    assert gone != planted
    if bug == "all at once":
        assert 0 in gone and planted[0] in gone                                    # both of the two equal rows
    with pytest.raises(AssertionError, match="is passed by the pruned set" if bug != "tolerance reversed" else "is implied by the others"):
        ic.check_as_sets(A, l, u, lr, ur)


# ---- 4. the front end and solve() ---------------------------------------------------------------------------------------------------
def _dense(p):
    A, l, u = p.vectorize() if hasattr(p, "vectorize") else p
    return np.atleast_2d(np.asarray(A, dtype=np.float64)), np.asarray(l, dtype=np.float64), np.asarray(u, dtype=np.float64)


def _within(P, Q):
    """Every finite bound of Q holds on P to TAU, by HiGHS (both over the same variables); an empty P is within anything."""
    (A, l, u), (B, lq, uq) = _dense(P), _dense(Q)
    if ic.highs_min(A, l, u, np.zeros(A.shape[1])) is None:
        return True
    for i in range(len(lq)):
        for sign, b in ((1.0, lq[i]), (-1.0, -uq[i])):
            if np.isfinite(b) and (b - ic.highs_min(A, l, u, sign * B[i])) / max(1.0, abs(b)) > ic.TAU:
                return False
    return True


def test_irredundant_batch_returns_what_it_cannot_prune():
    trips = [ic.planted(8, 4, s)[:3] for s in range(3)] + [ic.HAND["empty"], ic.HAND["crossed"]]
    big = (np.vstack([np.eye(2)] * 513), np.full(1026, -1.0), np.ones(1026))         # 1026 rows: beyond the kernel's limits
    wide = (np.ones((1, 257)), np.zeros(1), np.ones(1))
    items = trips + [big, wide]
    eng = TwinEngine()                                                              # an engine without the method
    got = polyhedra.irredundant_batch(items, eng)
    assert len(got) == len(items) and all(g is p for g, p in zip(got, items)) and eng.log == []
    eng = RedTwinEngine()
    got = polyhedra.irredundant_batch(items, eng)
    assert [m for m, _ in eng.log] == ["irredundant_bounds"] * 2                    # one call per shape within the limits
    assert eng.log[0][1][0] == "float64[2, 2, 4]" and eng.log[1][1][0] == "float64[3, 4, 11]"
    assert all(got[k] is items[k] for k in (3, 4, 5, 6))                            # EMPTY twice, beyond the limits twice
    for k in range(3):
        A, l, u = got[k].vectorize()
        assert isinstance(got[k], Poly) and np.array_equal(A, trips[k][0][:8]) and np.array_equal(u, np.ones(8)) and np.all(l == -INF)
    assert polyhedra.irredundant_batch([], eng) == []
    same = (np.eye(2), -np.ones(2), np.ones(2))                                     # nothing to remove: the item itself
    assert polyhedra.irredundant_batch([same], eng)[0] is same


def test_irredundant_batch_keeps_order_flags_and_the_local_form():
    """Rows: x0 in (-1, 1] open below; x1 <= 1 open; x0 <= 2 open (implied); -5 <= x0 + x1 < 1.5: the lower bound goes, its flag
    with it, the open upper one stays; x1 >= -1."""
    A = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    l = np.array([-1.0, -INF, -INF, -5.0, -1.0]); u = np.array([1.0, 1.0, 2.0, 1.5, INF])
    olo = np.array([True, False, False, True, False]); ohi = np.array([False, True, True, True, False])
    dense = Poly(A, l, u, open_lo=olo, open_hi=ohi)
    local = Poly.from_local(7, [5, 2], A[:, ::-1], l, u, open_lo=olo, open_hi=ohi)   # the same rows over variables 2 and 5 of 7
    eng = RedTwinEngine()
    got = polyhedra.irredundant_batch([dense, local], eng)
    assert len(eng.log) == 1 and eng.log[0][1][0] == "float64[2, 2, 5]"              # the local form goes up over its own columns
    for g, p in zip(got, (dense, local)):
        assert g is not p and g.ncols == p.ncols and len(g) == 4
        assert np.array_equal(g.A, p.A[[0, 1, 3, 4]])
        assert g.l.tolist() == [-1.0, -INF, -INF, -1.0] and g.u.tolist() == [1.0, 1.0, 1.5, INF]
        assert g.open_lo.tolist() == [True, False, False, False] and g.open_hi.tolist() == [False, True, True, False]
    assert got[1]._cols.tolist() == [2, 5] and got[0]._cols is None


@functools.lru_cache(maxsize=None)
def _solved(on):
    eng = RedTwinEngine()
    net = examples.setup("robust_avoid_simple", seed=1, irredundant_pieces=on)
    return algorithm.solve(net, engine=eng), eng, net


def test_solve_config_2_with_irredundant_pieces():
    (off, eng_off, net_off), (on, eng_on, net_on) = _solved(False), _solved(True)
    assert off["solved"] and on["solved"]
    assert np.max(np.abs(on["x_opt"] - off["x_opt"])) <= 1e-9
    assert "irredundant_bounds" not in [m for m, _ in eng_off.log] and "irredundant_bounds" in [m for m, _ in eng_on.log]
    assert sorted(on["Sol"]) == sorted(off["Sol"])
    fewer = 0
    for pid in sorted(off["Sol"]):
        a, b = off["Sol"][pid], on["Sol"][pid]
        assert (a is None) == (b is None)
        if a is None:
            continue
        assert len(a) == len(b), pid                                                # the same number of pieces per node
        for p, q in zip(a, b):
            assert len(q) <= len(p)                                                 # no piece has more rows than before
            fewer += len(q) < len(p)
            assert _within(p, q) and _within(q, p), pid                             # the same set, both ways
    assert fewer >= 1
    # the memo: per node, the graph process_level handed over and its pruning, which is what the answer holds
    memo = net_on.__dict__["_irredundant_memo"]
    assert net_off.__dict__["_irredundant_memo"] == {} and sorted(memo) == [pid for pid in sorted(on["Sol"]) if on["Sol"][pid] is not None]
    assert all(len(raw) == len(got) and all(len(q) <= len(p) for p, q in zip(raw, got)) for raw, got in memo.values())


def test_a_graph_handed_back_unchanged_is_not_pruned_again():
    """solve_base's memo: the second sweep of a level whose process_level returns the graph objects of the first sends nothing."""
    net = examples.setup("robust_avoid_simple", seed=1, irredundant_pieces=True)
    eng = RedTwinEngine()
    first = algorithm.solve(net, engine=eng)
    n1 = [m for m, _ in eng.log].count("irredundant_bounds")
    assert first["solved"] and n1 >= 1
    # the same net from its answer: process_level's own memo hands the same graphs back (solve() would reset both memos)
    memo = net.__dict__["_irredundant_memo"]
    before = {pid: got for pid, (raw, got) in memo.items()}
    again = algorithm.solve_base(net, first["x_opt"], level=1, proj_vectors=[], rng=np.random.default_rng(1), engine=eng)
    assert again["solved"] and again["x_opt"].tobytes() == first["x_opt"].tobytes()
    assert [m for m, _ in eng.log].count("irredundant_bounds") == n1                # not one more call
    assert len(before) == 4 and all(memo[pid][1] is before[pid] for pid in before)


def test_the_option_travels_and_is_off_by_default(tmp_path):
    import json
    import os
    from qpn_amd import interchange
    from qpn_amd.programs import QPNetOptions
    assert QPNetOptions().irredundant_pieces is False
    net = examples.setup("simple_bilevel", irredundant_pieces=True)
    interchange.save_qpnet(str(tmp_path), net)
    assert interchange.load_qpnet(str(tmp_path)).options.irredundant_pieces is True
    meta_path = os.path.join(str(tmp_path), "meta.json")
    with open(meta_path) as f:
        meta = json.load(f)
    del meta["options"]["irredundant_pieces"]                                       # a net written before the option existed
    with open(meta_path, "w") as f:
        json.dump(meta, f)
    assert interchange.load_qpnet(str(tmp_path)).options.irredundant_pieces is False
