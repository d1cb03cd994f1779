"""The box-MCP reference (tests/mcp_ref.py) and its planted cases (tests/mcp_cases.py) checked on the CPU:

* the reference certifies every case of every cell, recovers the plant within what one rounding of q allows, every case is
  mask-safe, every state appears where N allows, and every cell's items take the route the cell names (mcp_cases.route_of, the
  launchers' shape tests restated, with both ends of every register block size and every 256-row class reached);
* the reference has teeth: a bound row on the other side, the solution of the transposed problem, a perturbation of 1e-11 and
  GAVI multipliers of the opposite sign convention are each rejected by the certificate and / or the accuracy bar;
* the CPU oracle against the truth: SUCCESS, the masks of the truth, and an error within a cap per family;
* planted non-solutions: an infeasible item ends in RAY_TERM beside untouched neighbours, a pivot budget of 1 in MAX_ITERS.
"""
import numpy as np
import pytest

import mcp_cases as MC
import mcp_ref as MR
import solve_ref as SR

U = 2.0 ** -53                                            # unit roundoff of fp64

# The oracle's worst mcp_error against the truth per family, measured on this file's case set (every cell, both parts of
# scan_many, the feasible items of the non-solution batches, the CSC and checker cases), and the cap: 10 x the measurement (the
# margin covers other seeds).   family: (measured, cap)
ORACLE_CAPS = {
    "sym":  (6.2e-15, 6.2e-14),
    "skew": (5.1e-15, 5.1e-14),
    "k1e4": (1.2e-12, 1.2e-11),
}

SETS = list(MC.CELLS) + ["scan_many_nine", "scan_many_two", "nonsolutions", "csc", "check"]


def _batches(name):
    """(label, cases, shared) of a case set."""
    if name in MC.CELLS:
        return [(f"{name} N={N} {kinds} {f}", cases, name == "shared") for N, kinds, f, cases in MC.cell_cases(name)]
    if name == "scan_many_nine":
        return [(name, MC.scan_many_nine(), False)]
    if name == "scan_many_two":
        return [(name, MC.scan_many_two()[0], False)]
    if name == "nonsolutions":
        return [(f"{name} N={N}", [c for c in MC.nonsolution_batch(N) if not c.get("infeasible")], False)
                for N in MC.NONSOLUTION_SIZES]
    if name == "csc":
        return [(f"csc N={N}", [MC.csc_case(N)[0]], False) for N in (12, 130)]
    return [(f"check N={N}", MC.check_batch(N)[0], False) for N in MC.CHECK_FORMS]


@pytest.mark.parametrize("name", SETS)
def test_reference_recovers_the_plant_and_certifies_it(name):
    for label, cases, _ in _batches(name):
        for c in cases:
            z, info = MC.truth(c)
            assert info["ok"], f"{label}: {info['why']}"
            assert info["resid"] <= SR.RESID_BOUND
            # the data differ from the plant's by one rounding of q: |dz_U|_2 <= |M_UU^-1|_2 u |q|_2
            K, rhs, Urows, _ = MR.linear_system(*MC.data(c), c["state"])
            smin = np.linalg.svd(K, compute_uv=False)[-1] if Urows.size else 1.0
            allow = U * np.linalg.norm(c["q"]) / smin
            dz = float(np.linalg.norm(np.asarray(z - c["plant"], dtype=np.float64)))
            assert dz <= 1.01 * allow + 1e-18, f"{label}: |z* - plant| = {dz:.2e}, the rounding allows {allow:.2e}"
            assert MR.mask_safe(z, *MC.data(c)), f"{label}: not mask-safe"
            # every state at least once where N allows
            kind = np.zeros(c["N"], np.uint8) if c["kind"] is None else c["kind"]
            if c["kinds"] in ("box", "mixed") and name != "csc":
                for g, table in ((0, MR.STD_STATES), (1, MR.GAVI_STATES)):
                    rows = c["state"][kind == g]
                    if rows.size >= len(table):
                        assert set(rows) == set(table), f"{label}: states {sorted(set(rows))}"


def test_weak_rows_sit_on_their_bound():
    """A weak row's bound is the truth rounded to the feasible side: the row is feasible exactly, within one ulp of the bound,
    and carries the two codes of a bound with a zero residual."""
    seen = 0
    for N, kinds, f, cases in MC.cell_cases("reg_box"):
        for c in cases:
            z = MC.truth(c)[0]
            for i in np.flatnonzero(c["state"] == "weak"):
                lo = abs(z[i] - c["l"][i]) <= abs(z[i] - c["u"][i])
                b = c["l"][i] if lo else c["u"][i]
                assert (z[i] >= b if lo else z[i] <= b) and abs(z[i] - b) <= np.spacing(abs(b))
                assert MR.expected_masks(z, *MC.data(c))[i] == (3 if lo else 6)
                seen += 1
    assert seen > 20


def test_route_restatement():
    """Every instantiation the cell table names is reached, by the restated shape tests of the launchers."""
    # qpn_avi_reg_block_size's thresholds and the 256-row classes: both sides of each
    for lim, bs in MC.REG_BS:
        assert MC.route_of(lim, None, None, None) == ("reg", bs)
        if lim < 64:
            assert MC.route_of(lim + 1, None, None, None) == ("reg", MC.REG_BS[[b for _, b in MC.REG_BS].index(bs) + 1][1])
    assert [MC.route_of(N, None, None, None) for N in (65, 256, 257, 512, 513, 768, 769, 1024)] == \
        [("big", k) for k in (1, 1, 2, 2, 3, 3, 4, 4)]
    route = lambda c: MC.route_of(c["N"], c["kind"], c["l"], c["u"])
    reached = {}
    for cell, want in MC.EXPECT.items():
        for N, kinds, f, cases in MC.cell_cases(cell):
            for c in cases:
                r = route(c)
                assert r[0] == (want if (N >= 2 or cell != "scan_mixed") else "reg"), f"{cell} N={N} {kinds}: {r}"
                reached.setdefault(r, set()).add(N)
    for lim, bs in MC.REG_BS:                              # both ends of every block size (the first one from N = 1)
        lo = 1 if bs == 1 else [l for l, _ in MC.REG_BS][[b for _, b in MC.REG_BS].index(bs) - 1] + 1
        assert {lo, lim} <= reached["reg", bs], (bs, reached["reg", bs])
    assert all(("scan", bs) in reached for _, bs in MC.SCAN_BS)
    assert {2, 8} <= reached["scan", 1] and {9, 16} <= reached["scan", 2] and {17, 32} <= reached["scan", 4] and \
        {33, 64} <= reached["scan", 8]
    assert all(("big", k) in reached for k in (1, 2, 3, 4)) and 1024 in reached["big", 4] and {256, 257} <= (
        reached["big", 1] | reached["big", 2])
    assert all(("big_gated", k) in reached for k in (1, 2, 3))
    # the shared cell's batches go where their kinds send them
    assert {route(c)[0] for _, _, _, cs in MC.cell_cases("shared") for c in cs} == {"reg", "scan", "big"}
    # scan_many: every third item is kept by the Schur kernel's shape test, the others go to the scan kernel
    nine = MC.scan_many_nine()
    assert len(nine) == 2 * MC.SCAN_GRID + 5
    assert all(route(c) == (("schur",) if i % 3 == 0 else ("scan", 2)) for i, c in enumerate(nine))
    # ... so block g of the 2048 gathers its flagged items among g, g + 2048 and g + 4096 (2048 = 2 mod 3: one of the three is
    # node-shaped): two flagged items in most blocks, the third position in use in the first five
    flagged = np.array([i % 3 != 0 for i in range(len(nine))])
    per_block = np.bincount(np.arange(len(nine))[flagged] % MC.SCAN_GRID, minlength=MC.SCAN_GRID)
    assert per_block.max() == 2 and np.sum(per_block == 2) > 600 and flagged[2 * MC.SCAN_GRID:].sum() >= 3
    two, idx = MC.scan_many_two()
    assert idx.size == 64 * MC.SCAN_GRID + 3 and all(route(c) == ("scan", 1) for c in two)
    # a swapped item fails the ballot-mask test only: the same rows in node order are kept
    c = MC.cell_cases("scan_mixed")[-1][3][0]
    assert c["kinds"] == "swapped" and c["N"] == 64
    p = np.r_[32:64, 0:32]
    assert MC.route_of(64, c["kind"][p], c["l"][p], c["u"][p]) == ("schur",) and route(c) == ("scan", 8)
    c = next(cs[0] for N, kinds, f, cs in MC.cell_cases("big_mixed") if kinds == "swapped")
    p = np.r_[60:130, 0:60]
    assert MC.route_of(130, c["kind"][p], c["l"][p], c["u"][p]) == ("big_crash", 1) and route(c) == ("big_gated", 1)


# ---- teeth -------------------------------------------------------------------------------------------------------------------
def _case(family, kinds="mixed", N=17):
    cell = "scan_mixed" if kinds == "mixed" else "reg_box"
    return next(cs for n, k, f, cs in MC.cell_cases(cell) if (n, k, f) == (N, kinds, family))


def _bar(oracle, cases):
    ref = MC.oracle_solve(oracle, cases)
    return SR.accuracy_bar(max(MR.mcp_error(ref["z"][i], MC.truth(c)[0]) for i, c in enumerate(cases)))


def test_teeth_wrong_side():
    hit = 0
    for c in _case("sym"):
        M, q, l, u, kind = MC.data(c)
        for a, b in (("lower", "upper"), ("at_l", "at_u")):
            rows = np.flatnonzero((c["state"] == a) & np.isfinite(u))
            if rows.size:
                state = c["state"].copy()
                state[rows[0]] = b
                z, info = MR.solve_reference(M, q, l, u, kind, state)
                assert not info["ok"], info                                  # (whichever row the moved solution breaks first)
                hit += 1
    assert hit >= 2


def test_teeth_transposed_problem(oracle):
    cases = _case("skew")
    for c in cases:
        M, q, l, u, kind = MC.data(c)
        zT, _ = MR.solve_reference(np.ascontiguousarray(M.T), q, l, u, kind, c["state"])
        assert not MR.certificate(zT, M, q, l, u, kind, c["state"])[0]
        assert MR.mcp_error(zT, MC.truth(c)[0]) > 1e-3 > _bar(oracle, cases)


def test_teeth_small_noise(oracle):
    cases = _case("sym")
    c = cases[0]
    zt = MC.truth(c)[0]
    z = np.asarray(zt, dtype=np.float64) + 1e-11
    assert MR.mcp_error(z, zt) > _bar(oracle, cases)
    assert not MR.certificate(z, *MC.data(c), c["state"])[0]


def test_teeth_wrong_sign_convention(oracle):
    cases = _case("sym")
    c = next(c for c in cases if np.isin(c["state"], ("at_l", "at_u")).any())
    zt = MC.truth(c)[0]
    z = zt.copy()
    z[c["kind"] == 1] *= -1
    ok, why = MR.certificate(z, *MC.data(c), c["state"])
    assert not ok
    assert MR.mcp_error(z, zt) > 0.5 > _bar(oracle, cases)


def test_checker_restatement_is_decided():
    """The violation counts the GPU test compares qpn_check_avi_batch with: no compared quantity is near its threshold (a count
    that rounding could change would be no assertion), the truth has degree 0 and every planted violation raises its flag."""
    for N in MC.CHECK_FORMS:
        for c in MC.check_batch(N)[0]:
            M, q, l, u, kind = MC.data(c)
            deg, _, margin = MR.check_degree(M, q, l, u, kind, np.asarray(MC.truth(c)[0], dtype=np.float64))
            assert deg == 0 and margin > 0.9e-6
            for w, (_, _, _, flag) in enumerate(MC.VIOLATIONS):
                qv, zv, i = MC.violated(c, w)
                deg, flags, margin = MR.check_degree(M, qv, l, u, kind, zv)
                assert flags[i] & flag and deg >= 1 and margin > 1e-9, (N, w, deg, margin)


# ---- the CPU oracle against the truth ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_oracle_against_the_truth(oracle, name, capsys):
    worst, count = {}, 0
    for label, cases, shared in _batches(name):
        ref = MC.oracle_solve(oracle, cases, shared)
        assert np.all(ref["status"] == MC.SUCCESS), f"{label}: status {ref['status']}"
        fails, _, cnt = MC.check_against_truth(cases, ref, label)
        assert not fails, "\n".join(fails[:12])
        assert cnt == len(cases)
        for i, c in enumerate(cases):
            worst[c["family"]] = max(worst.get(c["family"], 0.0), MR.mcp_error(ref["z"][i], MC.truth(c)[0]))
        count += cnt
    with capsys.disabled():
        print(f"\n[oracle {name}] {count} items  " + "  ".join(f"{f} {e:.1e}" for f, e in sorted(worst.items())))
    for f, e in worst.items():
        assert e <= ORACLE_CAPS[f][1], f"{name}: the oracle's error on {f} is {e:.2e}, cap {ORACLE_CAPS[f][1]:.1e}"


# ---- planted non-solutions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", MC.NONSOLUTION_SIZES)
def test_oracle_on_planted_non_solutions(oracle, N):
    cases = MC.nonsolution_batch(N)
    ref = MC.oracle_solve(oracle, cases)
    assert list(ref["status"]) == [MC.SUCCESS, MC.RAY_TERM, MC.SUCCESS, MC.SUCCESS]
    keep = [0, 2, 3]
    fails, _, cnt = MC.check_against_truth([cases[i] for i in keep], {k: ref[k][keep] for k in ("z", "status", "active")}, f"N={N}")
    assert not fails and cnt == 3, fails
    # A budget of one pivot.  The budget bounds the Lemke loop (Stage B) alone: the crash (Stage A) before it takes one pivot per
    # free STD variable and per equality GAVI row whatever the budget, and counts them; Stage B then pivots only while the count
    # is below the budget -- once here if the crash took none, else not at all.  `pivots` is their sum.
    ref = MC.oracle_solve(oracle, cases, max_pivots=1)
    assert np.all(ref["status"] == MC.MAX_ITERS)
    assert list(ref["pivots"]) == [max(1, MC.crash_pivots(c)) for c in cases]
