"""level_batch.warm_big_host: the numpy twin of block principal pivoting on a large symmetric node's Schur problem and of its warm
start (QPN_OPT_WARM_BIG) -- the seed rule, the cap rule, the restart and the rounds, on the cases of
tests/warm_big_cases.py.  No GPU.

* cold runs take at least 4 rounds at the plain shapes; a true hint (the cold solution's multipliers) takes ONE round, switches
  no pair and ends in the cold run's sides;
* after a relative move of w by 1e-1 the old multipliers still save rounds against the cold run at the new w: no node takes
  more, the batch takes fewer, and at the plain shapes (where a cold run has rounds to save: the loose nodes need one or two)
  every node takes fewer; the sides are the cold run's;
* wrong hints (10 % of the rows redrawn, every finite-lower row at lower, all signs flipped) end in the cold run's sides;
* a hint over the cap, of NaNs, of zeros, or on infinite sides only, gives the cold output array for array;
* a seed within the cap but above the rank of S fails in its first factorisation and the workgroup restarts cold: on loose records,
  where the cold run finishes by block pivoting, the restart finishes too, with the cold run's multipliers, sides and count of
  pairs switched (one round more); at (70, 255) plain, where the cold rule itself names more rows than S has rank and the cold
  run ends NOT solved in its first round, the restarted run ends not solved as well (the Lemke kernel's node either way)."""
import numpy as np
import pytest

import warm_big_cases as C
from qpn_amd.level_batch import BPP_KMAX, warm_big_host

SHAPES = [(130, 40, "loose"), (160, 140, "plain"), (200, 150, "plain"), (256, 256, "plain")]
_cache = {}


def _twin(S, c, l, u, hint=None):
    return [warm_big_host(S[b], c[b], l[b], u[b], None if hint is None else hint[b]) for b in range(len(c))]


def _case(n, m, mode):
    """records, the Schur problems at the shared w and their cold runs: computed once, read only"""
    key = (n, m, mode)
    if key not in _cache:
        rec, w = C.records(n, m, mode)
        S, c = C.schur(rec, w)
        cold = _twin(S, c, rec[5], rec[6])
        _cache[key] = (rec, w, S, c, cold)
    return _cache[key]


def _same_output(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_the_cap_is_the_kernels():
    assert BPP_KMAX == C.KMAX == 112


@pytest.mark.parametrize("n,m,mode", SHAPES)
def test_a_true_hint_takes_one_round(n, m, mode):
    rec, w, S, c, cold = _case(n, m, mode)
    assert all(r["finished"] and not r["seeded"] for r in cold)
    print("cold rounds", [r["rounds"] for r in cold], "switched", [r["switched"] for r in cold])
    if mode == "plain":
        assert all(r["rounds"] >= 4 for r in cold)
    lam = np.array([r["lam"] for r in cold])
    hot = _twin(S, c, rec[5], rec[6], lam)
    for r, r0 in zip(hot, cold):
        assert r["finished"] and r["seeded"] and not r["restarted"]
        assert r["rounds"] == 1 and r["switched"] == 0
        assert np.array_equal(r["side"], r0["side"])
        assert np.max(np.abs(r["lam"] - r0["lam"])) <= 1e-9 * max(1.0, np.max(np.abs(r0["lam"])))


@pytest.mark.parametrize("n,m,mode", SHAPES)
def test_a_hint_from_before_a_move_of_w_saves_rounds(n, m, mode):
    rec, w, S, c, cold = _case(n, m, mode)
    lam = np.array([r["lam"] for r in cold])
    S2, c2 = C.schur(rec, C.moved(w, 1e-1))
    cold2 = _twin(S2, c2, rec[5], rec[6])
    hot2 = _twin(S2, c2, rec[5], rec[6], lam)
    print("cold", [r["rounds"] for r in cold2], "hinted", [r["rounds"] for r in hot2], "switched", [r["switched"] for r in hot2])
    for r, r0 in zip(hot2, cold2):
        assert r["finished"] and r0["finished"] and np.array_equal(r["side"], r0["side"])
        assert r["rounds"] <= r0["rounds"]
        if mode == "plain":
            assert r["rounds"] < r0["rounds"]
    assert sum(r["rounds"] for r in hot2) < sum(r["rounds"] for r in cold2)


@pytest.mark.parametrize("kind", C.WRONG)
@pytest.mark.parametrize("n,m,mode", SHAPES)
def test_wrong_hints_end_in_the_cold_sides(n, m, mode, kind):
    rec, w, S, c, cold = _case(n, m, mode)
    lam = np.array([r["lam"] for r in cold])
    hint = C.wrong(kind, lam, rec[5])
    for r, r0, h in zip(_twin(S, c, rec[5], rec[6], hint), cold, hint):
        assert r["finished"] and np.array_equal(r["side"], r0["side"])
        assert r["seeded"] == (1 <= np.count_nonzero(h) <= BPP_KMAX)
        assert np.max(np.abs(r["lam"] - r0["lam"])) <= 1e-9 * max(1.0, np.max(np.abs(r0["lam"])))


def test_a_seed_over_the_cap_is_dropped(oracle):
    """(200, 150) tight: the solution holds more rows at a bound than the tiles have room for."""
    import problems as P
    n, m = 200, 150
    rec, w, S, c, cold = _case(n, m, "tight")
    M, q, lo, hi, kd = P.reduced_blocks(*rec, w)
    ref = oracle.solve_avi_batch(M, q, lo, hi, kind=kd)
    assert np.all(ref["status"] == 1)
    lam = ref["z"][:, n:]
    named = np.count_nonzero(lam, axis=1)
    print("rows named", named)
    assert np.all(named > BPP_KMAX) and np.all((128 <= named) & (named <= 138))
    for r, r0 in zip(_twin(S, c, rec[5], rec[6], lam), cold):
        assert not r["seeded"]
        _same_output(r, r0)


@pytest.mark.parametrize("what", ["nan", "zero", "infinite side"])
def test_hints_that_name_nothing_give_the_cold_output(what):
    rec, w, S, c, cold = _case(160, 140, "plain")
    l, u = rec[5], rec[6]
    if what == "nan":
        hint = np.full_like(l, np.nan)
    elif what == "zero":
        hint = np.zeros_like(l); hint[:, 1::2] = -0.0
    else:
        rec, hint = C.one_sided(rec)
        l, u = rec[5], rec[6]
        cold = _twin(S, c, l, u)
    for r, r0 in zip(_twin(S, c, l, u, hint), cold):
        assert r0["finished"] and not r["seeded"]
        _same_output(r, r0)


@pytest.mark.parametrize("n,m,rows,finish", [(96, 200, 110, 4), (70, 255, 100, 3)])
def test_a_restart_after_a_dependent_seed_finishes_what_the_cold_run_finishes(n, m, rows, finish):
    """Loose records: S = A Q^-1 A' has rank n, the seed names `rows` > n rows (within the cap), the cold rule few enough.  The
    seeded attempt fails in its first factorisation; the restart has to clear the failure, forget the seed and run the rounds."""
    rec, w, S, c, cold = _case(n, m, "loose")
    print("cold finished", [r["finished"] for r in cold], "rounds", [r["rounds"] for r in cold], "switched", [r["switched"] for r in cold])
    assert sum(r["finished"] for r in cold) == finish
    assert all(r["rounds"] >= 4 for r in cold if r["finished"])            # (the restart has rounds to run)
    for r, r0 in zip(_twin(S, c, rec[5], rec[6], C.dependent(m, rows=rows)), cold):
        assert r["seeded"] and r["restarted"]
        assert r["finished"] == r0["finished"]
        assert r["rounds"] == 1 + r0["rounds"] and r["switched"] == r0["switched"]
        assert np.array_equal(r["lam"], r0["lam"]) and np.array_equal(r["side"], r0["side"])


def test_a_dependent_seed_where_the_cold_run_does_not_finish_either():
    """(70, 255) plain: S has rank 70, the seed names 100 rows, and the cold rule names more than 70 as well -- both attempts end
    in their first factorisation, NOT solved (finished = False, lam = 0: the node is the Lemke kernel's, hinted or not)."""
    rec, w, S, c, cold = _case(70, 255, "plain")
    assert not any(r0["finished"] for r0 in cold) and all(r0["rounds"] == 1 for r0 in cold)
    for r, r0 in zip(_twin(S, c, rec[5], rec[6], C.dependent(255)), cold):
        assert r["seeded"] and r["restarted"] and not r["finished"]
        assert r["rounds"] == 1 + r0["rounds"]                 # the seeded attempt ends in its first factorisation
        for k in ("lam", "side", "finished", "switched"):
            assert np.array_equal(r[k], r0[k]), k
