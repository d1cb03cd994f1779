"""The reference of the convexity tests (tests/convexity_ref.py) and their cases (tests/convexity_cases.py), checked on the CPU:
the enclosure against the closed forms, its width, the condition on the inputs, and that every verdict is decidable."""
from __future__ import annotations

import numpy as np
import pytest

import convexity_cases as CC
import convexity_ref as CR

LD = np.longdouble
SHAPES = [s for s, _ in CC.SHAPES]


def _ids(s):
    return f"{s[0]}x{s[1]}"


def test_every_family_and_boundary_is_present():
    cases = CC.all_cases()
    fam = {(c["family"], c["hessian"]) for nodes in cases.values() for c in nodes}
    assert {f for f, _ in fam} == set(CC.ROWS) and {h for _, h in fam} == set(CC.HESSIANS)
    ds = {c["n"] - c["rank"] for nodes in cases.values() for c in nodes}
    assert {0, 1, 2} <= ds
    wide = [c for c in cases[(4, 1024)] if c["family"] == "wide" and c["scale"] == 0]
    assert sorted(c["rank"] for c in wide) == [2, 3, 4] and all(c["sel"].shape[0] == 500 for c in wide)
    assert any(c["scale"] == 100 for c in cases[(32, 32)]) and any(c["scale"] == -100 for c in cases[(32, 32)])
    for (n, m), cls in CC.SHAPES:
        dep = {c["family"] for c in cases[(n, m)]} & set(CC.DEPENDENT)
        assert m < 2 or {"dup_neg", "dup_same", "dup_scaled", "unit_pair"} <= dep, (n, m, dep)
        if cls == "wave":
            assert len(cases[(n, m)]) % CC.CVX_WAVES
    # the marked rows are what the node says they are
    for nodes in cases.values():
        for c in nodes:
            got = CR.selected_rows(c["A"], c["eq"])
            assert got.shape == c["sel"].shape and np.array_equal(np.sort(got, axis=0), np.sort(c["sel"], axis=0))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_inputs_meet_their_condition(shape):
    for c in CC.all_cases()[shape]:
        assert CC.sigma_ok(c), (c["family"], c["hessian"], shape)
        k = c["sel"].shape[0]
        if k:                                              # the rank by construction is the rank numpy sees, clear of any threshold
            sv = np.linalg.svd(c["sel"], compute_uv=False)
            r = c["rank"]
            assert np.all(sv[:r] >= CC.SIGMA_RATIO * sv[0]) and np.all(sv[r:] <= 1e-12 * sv[0]), (c["family"], shape, sv[r:].max() / sv[0])


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_enclosure_is_tight_contains_the_closed_form_and_decides_the_verdict(shape):
    n_closed = 0
    for c in CC.all_cases()[shape]:
        t = CC.truth(c)
        where = (c["family"], c["hessian"], shape, c["variant"], c["scale"])
        assert t["d"] == c["n"] - c["rank"]
        if t["d"] == 0:
            assert t["lo"] == t["hi"] == np.inf
            continue
        assert t["lo"] <= t["hi"] and t["hi"] - t["lo"] <= CR.EPS * t["snorm"], (where, float(t["hi"] - t["lo"]), t["snorm"])
        if c["lam"] is not None:
            # (the closed form is evaluated in longdouble: good to a few 2^-64 of its size)
            slack = 16 * CR.LD_EPS * max(abs(float(c["lam"])), t["snorm"])
            assert LD(t["lo"]) - slack <= c["lam"] <= LD(t["hi"]) + slack, (where, t["lo"], float(c["lam"]), t["hi"])
            n_closed += 1
        # plain64 is the yardstick of the kernel's bar: its own error stays far inside the old tolerance
        assert CR.accuracy_bar(t["e64"], t["snorm"]) <= CR.OLD_BAR * max(1.0, t["snorm"]), (where, t["e64"])
        # the verdict convex = (min_eig > -tol) is decidable: the truth is not within 1e-3 tol of -tol, nor within the reach of
        # an answer that meets the floor of the accuracy bar 16 times over
        gap = CR.dist(-CC.TOL, t["lo"], t["hi"])
        assert gap > 1e-3 * CC.TOL and gap > 16 * CR.FLOOR * t["snorm"], (where, t["lo"], t["hi"])
    if shape[0] > 1:
        assert n_closed >= 5


def test_reference_on_hand_made_nodes():
    # S = diag(1, -1): free it is -1; x2 pinned by two opposing rows it is 1; both pinned: nothing left
    Qd = np.diag([0.5, -0.5]) + np.array([[0.0, 3.0], [-3.0, 0.0]])
    lo, hi, d = CR.reference(Qd, np.zeros((0, 2)), 0)
    assert d == 2 and lo <= -1.0 <= hi and hi - lo <= CR.EPS
    lo, hi, d = CR.reference(Qd, np.array([[0.0, 1.0], [0.0, -1.0]]), 1)
    assert d == 1 and lo <= 1.0 <= hi and hi - lo <= CR.EPS
    assert CR.reference(Qd, np.eye(2), 2) == (np.inf, np.inf, 0)
    assert CR.plain64(Qd, np.array([[0.0, 1.0], [0.0, -1.0]]), 1) == (pytest.approx(1.0, abs=1e-15), 1)
    # a dense pin: S = I - 3 u u', rows +-u: the reduced Hessian is the identity on u's complement
    rng = np.random.default_rng(3)
    u = rng.standard_normal(7); u /= np.linalg.norm(u)
    S = np.eye(7) - 3.0 * np.outer(u, u)
    lo, hi, d = CR.reference(0.5 * S, np.stack([u, -u]), 1)
    assert d == 6 and abs(lo - 1.0) <= 1e-14 and abs(hi - 1.0) <= 1e-14
    lo, hi, d = CR.reference(0.5 * S, np.zeros((0, 7)), 0)
    assert d == 7 and abs(lo + 2.0) <= 1e-14 and abs(hi + 2.0) <= 1e-14
