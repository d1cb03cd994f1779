"""The case builder of tests/stage_b_cases.py through the CPU oracle: every class of every shape shows its marker without a
GPU, so a case set that lost a path of the Stage B pivot loop fails here before it fails to test anything on the device."""
import numpy as np
import pytest

import stage_b_cases as S
import stage_b_lemke as L

SHAPES = [(32, 32), (16, 16), (20, 12), (20, 20)]


def _single(oracle, rec, max_pivots=0):
    return S.oracle_solve(oracle, tuple(c[None] for c in rec), S.W0, max_pivots=max_pivots)


@pytest.mark.parametrize("n,m", SHAPES)
def test_every_class_shows_its_marker_in_the_oracle(oracle, n, m):
    names = S.class_names(m)
    assert len(names) == len(set(names)) and (m < 32 or len(names) == 18)
    for name in names:
        rec, meta = S.special(name, n, m)
        S.check_marker(name, rec, meta, _single(oracle, rec), 0, n)


@pytest.mark.parametrize("n,m", SHAPES)
def test_the_flips_node_takes_the_bound_flip_branch_in_both_directions(oracle, n, m):
    """`pivots` exceeds the number of basis changes, by a flip from lo to hi and one from hi to lo at least; the walk that says
    so is the oracle's: same status, same pivot count."""
    o = oracle.default_opts()
    rec, _ = S.special("flips", n, m)
    ref = _single(oracle, rec)
    wk = L.walk(*rec, S.W0, o.piv_tol, o.feas_tol)
    assert wk["status"] == ref["status"][0] == S.SUCCESS
    assert wk["pivots"] == ref["pivots"][0] - n
    assert +1 in wk["flips"] and -1 in wk["flips"], wk["flips"]
    assert wk["pivots"] == wk["basis_changes"] + len(wk["flips"]) > wk["basis_changes"]
    for w in (S.W0, S.W1):                              # multipliers of a few units: the 1e-9 bar is asked of well-scaled numbers
        z = S.oracle_solve(oracle, tuple(c[None] for c in rec), w)["z"][0]
        assert np.abs(z[n:]).max() <= 10.0


@pytest.mark.parametrize("n,m", SHAPES)
def test_the_walk_is_the_oracles_on_every_class(oracle, n, m):
    """The walk reproduces the oracle's status and pivot count on every class, and only `flips` (and, at one shape, `many`) flips:
    the classes whose pivot count is asserted exactly take no flip."""
    o = oracle.default_opts()
    for name in S.class_names(m):
        if name == "equal":
            continue                                    # (declined: not a node of this loop)
        rec, _ = S.special(name, n, m)
        ref = _single(oracle, rec)
        wk = L.walk(*rec, S.W0, o.piv_tol, o.feas_tol)
        assert (wk["status"], wk["pivots"]) == (ref["status"][0], ref["pivots"][0] - n), name
        if name not in ("flips", "many"):
            assert wk["flips"] == [], name


def test_the_row_registers_and_tile_columns_are_all_there():
    rows = [S.reg_row(j) for j in range(8)]
    assert [((k >> 4) << 2) | ((k >> 2) & 3) for k in rows] == list(range(8))       # the kernel's rsel of pivot row k
    assert sorted({k & 3 for k in rows}) == [0, 1, 2, 3]                              # every lane group owns a pivot row
    assert {k < 16 for k in rows} == {True, False}                                    # entering columns in both tile columns


@pytest.mark.parametrize("n,m", [(32, 32)])
def test_the_pivot_budget_stops_the_long_node_and_not_the_short_ones(oracle, n, m):
    budget = n + S.BUDGET_EXTRA
    rec, _ = S.special("many", n, m)
    ref = _single(oracle, rec, max_pivots=budget)
    assert ref["status"][0] == S.MAX_ITERS and ref["pivots"][0] == budget
    rec, meta = S.special("row_reg_5", n, m)
    S.check_marker("row_reg_5", rec, meta, _single(oracle, rec, max_pivots=budget), 0, n)


def test_the_batches_hold_every_class_once():
    for name, (kind, cnt, n, m, seed) in S.SCENARIOS.items():
        if cnt > 1000:
            continue                                    # (the same builder; the large batch is made by the GPU test alone)
        recs, where = S.scenario_records(name)
        want = [nm for nm in S.class_names(m) if not (kind == "budget" and nm == "equal")]
        assert list(where) == want and len(set(where.values())) == len(want)
        for nm, i in where.items():
            rec, _ = S.special(nm, n, m)
            for a, b in zip(rec, recs):
                if not (kind == "handle_asym" and a is rec[0]):
                    assert np.array_equal(a, b[i])
