"""The projection of degenerate solution-graph pieces (qpn_project_pieces) on the CPU: level_batch.project_pieces_host, the entry's
numpy twin, over the cases of tests/project_cases.py -- bit for bit against avi_solutions.eliminate_multipliers' core and against
that function as it was before it was split, against reduced_pieces on pieces that are not degenerate, as SETS against an LP
reference that eliminates nothing (which also has to catch three wrong eliminations), the cap rule, and the route through
level_batch.solution_pieces: solve() with an engine that has project_pieces returns the same pieces in the same order as without.
GPU side of the same cases: tests/test_gpu_project_pieces.py."""
import numpy as np
import pytest

import project_cases as pc
import reduced_cases as rc

import qpn_amd  # noqa: F401
from qpn_amd import algorithm, avi_solutions, examples, level_batch
from qpn_amd.programs import Poly

INF = np.inf


def _eliminate_multipliers_before(P, n, m, tol=1e-9, max_rows=4096):
    """avi_solutions.eliminate_multipliers as it stood before project_rows was taken out of it, word for word."""
    A, l, u = (np.array(a, dtype=np.float64) for a in P.vectorize())
    alive = np.ones(A.shape[0], bool)
    left = []
    for j in range(n, n + m):
        col = np.where(alive & (l == u) & np.isfinite(l), np.abs(A[:, j]), 0.0)
        i = int(np.argmax(col)) if col.size else -1
        if i < 0 or col[i] <= tol:
            if np.any(alive & (np.abs(A[:, j]) > tol)):
                left.append(j)
            continue
        piv = A[i, j]
        for k in np.nonzero(alive & (np.abs(A[:, j]) > 0.0))[0]:
            if k == i:
                continue
            f = A[k, j] / piv
            A[k] -= f * A[i]; A[k, j] = 0.0
            l[k] -= f * l[i]; u[k] -= f * u[i]
        alive[i] = False
    A, l, u = A[alive], l[alive], u[alive]
    for j in left:
        zero = np.abs(A[:, j]) <= tol
        Az, lz, uz = A[zero], l[zero], u[zero]
        ub, lb = [], []
        for k in np.nonzero(~zero)[0]:
            for a_, b_ in ((A[k], u[k]), (-A[k], -l[k])):
                if not np.isfinite(b_):
                    continue
                (ub if a_[j] > 0 else lb).append((a_ / abs(a_[j]), b_ / abs(a_[j])))
        if len(ub) * len(lb) + Az.shape[0] > max_rows:
            raise RuntimeError("eliminate_multipliers: the piece needs a polyhedral projection (too many rows)")
        rows = [(au + al, bu + bl) for au, bu in ub for al, bl in lb]
        A = np.vstack([Az] + [r[0][None] for r in rows]) if rows else Az
        l = np.concatenate([lz, np.full(len(rows), -INF)]); u = np.concatenate([uz, np.array([r[1] for r in rows])])
        A[:, j] = 0.0
    keep_cols = [c for c in range(A.shape[1]) if c < n or c >= n + m]
    return Poly(A[:, keep_cols], l, u)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _fill_beyond(out, t):
    Ar, lr, ur, rows, _ = out
    r = int(rows[t])
    return not Ar[t][:, r:].any() and np.all(lr[t][r:] == -INF) and np.all(ur[t][r:] == INF)


@pytest.mark.parametrize("name", pc.CASES)
def test_twin_equals_eliminate_multipliers_bit_for_bit(oracle, name):
    """Per piece: the twin's rows are project_rows' (the core of eliminate_multipliers) bit for bit, the rest is fill; and
    eliminate_multipliers gives what it gave before the split, bit for bit."""
    c = pc.case(name)
    n, m, p = c["shape"]
    out = pc.twin_output(name)
    assert out[0].shape == (len(c["K"]), n + p, c["cap"]) and not out[4].any()
    for t in range(len(c["K"])):
        A, l, u = pc.kept_rows(name, t)
        core = avi_solutions.project_rows(A, l, u, n, m)
        r = int(out[3][t])
        assert core[0].shape == (r, n + p)
        assert _bits(out[0][t][:, :r].T) == _bits(core[0]) and _bits(out[1][t][:r]) == _bits(core[1]) and _bits(out[2][t][:r]) == _bits(core[2])
        assert _fill_beyond(out, t)
        P = Poly(A, l, u, normalise=False)
        now, before = avi_solutions.eliminate_multipliers(P, n, m), _eliminate_multipliers_before(P, n, m)
        for a, b in zip(now.vectorize(), before.vectorize()):
            assert _bits(a) == _bits(b)
        for a, b in zip(now.vectorize(), Poly(*core).vectorize()):
            assert _bits(a) == _bits(b)
    if name == "pairs":                                               # what the case is for: two columns are left
        assert len(avi_solutions.pin_multipliers(*pc.kept_rows(name, 0), n, m)[3]) == 2


def test_twin_equals_reduced_pieces_where_nothing_is_degenerate(oracle):
    """On pieces without a leftover column the first n + 2m rows are reduced_pieces' output bit for bit, fill included, and
    nothing but fill lies beyond."""
    from oracle_engine import OracleEngine
    shape = (5, 6, 3)
    n, m, p = shape
    c = rc.case(shape, "gauss")
    want = rc.twin_output(shape, "gauss")
    assert not np.asarray(want[4]).any()
    lifted = OracleEngine().local_pieces(*c["args"], c["K"], node_of=c["node_of"])
    got = level_batch.project_pieces_host(*lifted, n, m)
    cap0 = n + 2 * m
    assert got[0].shape[2] == level_batch.project_cap(n, m) > cap0
    assert _bits(got[0][:, :, :cap0]) == _bits(want[0]) and _bits(got[1][:, :cap0]) == _bits(want[1]) and _bits(got[2][:, :cap0]) == _bits(want[2])
    assert np.array_equal(got[3], want[3]) and not got[4].any()
    assert all(_fill_beyond(got, t) for t in range(len(c["K"])))


_worst = {}


@pytest.mark.parametrize("name", pc.CASES)
def test_twin_output_is_the_projection_as_a_set(oracle, name):
    """The twin's rows against the LP reference: inside points in (TAU_IN), outside points out (TAU_OUT), at most 10 % skipped."""
    worst, least = pc.check_projection(pc.twin_output(name), pc.points(name))
    _worst[name] = worst
    print(f"{name}: worst inside violation {worst:.3e} (TAU_IN {pc.TAU_IN:.2e}), smallest outside violation {least:.3e}")


def test_tau_in_is_the_measured_constant(oracle):
    """TAU_IN = 1000 x the twin's worst inside violation over all cases, and that worst is what project_cases.py says it is."""
    for name in pc.CASES:
        if name not in _worst:
            _worst[name] = pc.check_projection(pc.twin_output(name), pc.points(name))[0]
    worst = max(_worst.values())
    print({k: f"{v:.3e}" for k, v in _worst.items()})
    assert pc.TAU_IN == 1000 * pc.TWIN_WORST
    assert 0.5 * pc.TWIN_WORST <= worst <= 2.0 * pc.TWIN_WORST, worst


@pytest.mark.parametrize("bug", pc.BUGS)
def test_a_wrong_elimination_fails_the_set_check(oracle, bug):
    """The reference has to tell: a Fourier-Motzkin step with a pair left out, with bounds not scaled, or with a row's bounds in
    each other's place is refused on the doubled-row case (all three show there: its step divides by 2 and its bounds are not 0);
    the first and the last also on the two-pairs case.  The restatement without a bug is the product's step bit for bit."""
    for name in ("scaled", "pairs"):
        c = pc.case(name)
        n, m, p = c["shape"]
        right = pc.project_with(None, name, 0)
        twin = pc.twin_output(name)
        r = int(twin[3][0])
        assert int(right[3][0]) == r and _bits(right[0][0]) == _bits(twin[0][0][:, :r]) and _bits(right[2][0]) == _bits(twin[2][0][:r])
        pc.check_projection(right, [pc.points(name)[0]])
        if name == "pairs" and bug == "bounds not scaled":
            continue                                                  # (copies of a row: the step divides by 1)
        with pytest.raises(AssertionError, match="cut off|let in"):
            pc.check_projection(pc.project_with(bug, name, 0), [pc.points(name)[0]])


def test_swapping_the_lists_as_wholes_changes_no_row(oracle):
    """ub and lb in each other's place is NOT a wrong elimination: every entry of one list still meets every entry of the other
    and au + al = al + au bit for bit, so the same rows come out in another order.  No set-level check can, or need, refuse it."""
    for name in ("scaled", "pairs", "5-6-3"):
        a, b = pc.project_with(None, name, 0), pc.project_with("lists swapped", name, 0)
        rows = lambda o: sorted((_bits(o[0][0][:, k]) + _bits(o[1][0][k:k + 1]) + _bits(o[2][0][k:k + 1])) for k in range(int(o[3][0])))
        assert rows(a) == rows(b)


def test_overflow_case_is_what_it_says(oracle):
    """(64, 65, 2) (b) at cap = n + 2m = 194: the step would make 1101 rows, so the piece comes back with flag 4, rows 0 and all
    fill; with room for them the rows come."""
    c = pc.case(pc.OVERFLOW)
    n, m, p = c["shape"]
    assert c["cap"] == n + 2 * m == 194 and len(c["K"]) == 1
    Ar, lr, ur, rows, flags = pc.twin_output(pc.OVERFLOW)
    assert flags.tolist() == [4] and rows.tolist() == [0]
    assert not Ar.any() and np.all(lr == -INF) and np.all(ur == INF) and Ar.shape == (1, n + p, 194)
    A, l, u = pc.kept_rows(pc.OVERFLOW, 0)
    assert avi_solutions.project_rows(A, l, u, n, m, max_rows=pc.OVERFLOW_ROWS - 1) is None
    assert avi_solutions.project_rows(A, l, u, n, m, max_rows=pc.OVERFLOW_ROWS)[0].shape[0] == pc.OVERFLOW_ROWS
    with pytest.raises(ValueError):
        level_batch.project_pieces_host(*pc.lifted(pc.OVERFLOW), n, m, cap=193)


def test_project_cap():
    assert level_batch.project_cap(5, 16) == 256 and level_batch.project_cap(64, 65) == 776 and level_batch.project_cap(256, 256) == 3072
    assert level_batch.project_cap(1, 511) == 4092
    assert (level_batch.PROJECT_CAP_MIN, level_batch.PROJECT_CAP_FACTOR, level_batch.PROJECT_CAP_MAX) == (256, 4, 4096)


# ---- the route through solution_pieces ----------------------------------------------------------------------------------------
def _stub_engine():
    from oracle_engine import OracleEngine

    class WithProjection(OracleEngine):
        """The CPU engine plus project_pieces = project_pieces_host over ONE local_pieces call for all the pieces handed in."""
        projected = 0
        project_calls = 0

        def project_pieces(self, Qc, Rc, qd, Ac, Bc, l, u, K, node_of=None, tol=1e-9, cap=None):
            self.project_calls += 1
            self.projected += len(K)
            lifted = OracleEngine.local_pieces(self, Qc, Rc, qd, Ac, Bc, l, u, K, node_of=node_of)
            return level_batch.project_pieces_host(*lifted, np.shape(qd)[1], np.shape(l)[1], tol=tol, cap=cap)
    return WithProjection()


def _solve_recording(eng, seed, monkeypatch):
    """solve() on config 2 with every solution graph: -> (result, the keys of every piece solution_pieces returned, in order,
    the number of per-piece host reductions)."""
    keys, host = [], [0]
    pieces, reduce = level_batch.solution_pieces, level_batch._reduce_on_host

    def recording(*a, **k):
        out = pieces(*a, **k)
        keys.append([None if lst is None else [level_batch._poly_key(P) for P in lst] for lst in out])
        return out

    def counting(*a, **k):
        host[0] += 1
        return reduce(*a, **k)
    monkeypatch.setattr(level_batch, "solution_pieces", recording)
    monkeypatch.setattr(level_batch, "_reduce_on_host", counting)
    net = examples.setup("robust_avoid_simple", seed=seed)
    net.options.max_pieces = None
    ret = algorithm.solve(net, engine=eng)
    monkeypatch.setattr(level_batch, "solution_pieces", pieces)
    monkeypatch.setattr(level_batch, "_reduce_on_host", reduce)
    return ret, keys, host[0]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_solve_returns_the_same_pieces_with_and_without_project_pieces(oracle, monkeypatch, seed):
    """Config 2, max_pieces = None: an engine with project_pieces gives pieces with the same keys in the same order, and the same
    point, as one without; its flagged pieces go through the one call per round and none through the per-piece route.  With
    cap = n + 2m the pieces that do not fit fall back to that route, and still nothing changes."""
    from oracle_engine import OracleEngine
    want, want_keys, host0 = _solve_recording(OracleEngine(), seed, monkeypatch)
    assert host0 >= 2                                                 # (the run has flagged pieces at all)
    eng = _stub_engine()
    got, got_keys, host1 = _solve_recording(eng, seed, monkeypatch)
    assert got_keys == want_keys
    assert got["solved"] == want["solved"] and _bits(got["x_opt"]) == _bits(want["x_opt"])
    assert host1 == 0 and eng.projected == host0 and 1 <= eng.project_calls <= host0
    if seed == 1:
        monkeypatch.setattr(level_batch, "PROJECT_CAP_MIN", 0)
        monkeypatch.setattr(level_batch, "PROJECT_CAP_FACTOR", 1)
        eng = _stub_engine()
        got, got_keys, host2 = _solve_recording(eng, seed, monkeypatch)
        assert got_keys == want_keys and _bits(got["x_opt"]) == _bits(want["x_opt"])
        assert eng.projected == host0 and 0 <= host2 <= host0
