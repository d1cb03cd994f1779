"""The node-solve reference (tests/solve_ref.py) and its planted cases (tests/solve_cases.py) checked on the CPU:

* the reference recovers the plant within what the rounding of qd and of the active bounds allows, its certificate holds on every
  case of every cell, every case outside the rowscale family is mask-safe, and every cell's shapes map to the route it names;
* the reference has teeth: a wrong active side, the solution of the symmetrised problem, a perturbation of 1e-11 and a multiplier
  of the wrong sign convention are each rejected by the certificate and / or the accuracy bar;
* the CPU oracle against the truth -- the first check of the oracle that owes nothing to its own pivot rule: SUCCESS, the masks of
  the truth, and an error within a cap per family.
"""
import numpy as np
import pytest

import solve_cases as SC
import solve_ref as SR

U = 2.0 ** -53                                            # unit roundoff of fp64

# The oracle's worst node_error against the truth per family, measured on this file's case set (every cell, both plants), and the
# cap: 10 x the measurement (the margin covers other seeds).   family: (measured, cap)
ORACLE_CAPS = {
    "k40":      (2.9e-14, 2.9e-13),
    "k1e4":     (5.0e-11, 5.0e-10),
    "k1e6":     (3.1e-09, 3.1e-08),
    "axis":     (6.5e-10, 6.5e-09),
    "skew":     (1.6e-14, 1.6e-13),
    "nearsym":  (4.5e-14, 4.5e-13),
    "weak":     (2.6e-14, 2.6e-13),
    "k0":       (5.4e-15, 5.4e-14),
    "kfull":    (2.3e-10, 2.3e-09),
    "rowscale": (2.7e-12, 2.7e-11),
}


def _all_nodes(cell):
    for n, m, p, nodes in SC.cell_cases(cell):
        yield n, m, p, nodes
    if cell in ("f32_handle_sym", "f32_mixed"):
        n, m, p, _ = SC.cell_cases(cell)[0]
        yield n, m, p, SC.second_plants(cell)


@pytest.mark.parametrize("cell", list(SC.CELLS))
def test_reference_recovers_the_plant_and_certifies_it(cell):
    fams = set()
    for n, m, p, nodes in _all_nodes(cell):
        if cell in SC.ROUTE:
            assert SC.route_of(n, m) == SC.ROUTE[cell], f"{cell}: ({n}, {m}) goes to {SC.route_of(n, m)}"
        for c in nodes:
            z, info = SC.truth(c)
            tag = f"{cell} ({n}, {m}) {c['family']}"
            assert info["ok"], f"{tag}: {info['why']}"
            assert info["resid"] <= SR.RESID_BOUND
            # the data differ from the plant's by one rounding of qd and of the active bounds: |dz|_2 <= |K^-1|_2 u |[qd; b_act]|_2
            Q, R, qd, A, B, l, u = c["rec"]
            K, rhs, rows = SR.kkt_system(*c["rec"], c["w"], c["side"])
            bact = np.where(c["side"][rows] > 0, l[rows], u[rows])
            allow = U * np.linalg.norm(np.concatenate([qd, bact])) / np.linalg.svd(K, compute_uv=False)[-1]
            dz = float(np.linalg.norm(np.asarray(z - c["plant"], dtype=np.float64)))
            assert dz <= 1.01 * allow + 1e-18, f"{tag}: |z* - plant| = {dz:.2e}, the roundings allow {allow:.2e}"
            act = c["side"] != 0
            assert info["min_lam"] * (c["row_scale"][act].max() if act.any() else 1) >= 0.49
            if c["family"] != "rowscale":
                assert SR.mask_safe(z, *c["rec"], c["w"]), f"{tag}: not mask-safe"
                weak = SR.expected_masks(z, *c["rec"], c["w"])[n:][c["weak"]] >> 4
                assert c["weak"].sum() == (2 if c["family"] == "weak" else 0) and set(weak) <= {3, 6}   # both codes
                assert info["min_slack"] >= (0.19 if c["family"] != "weak" else -SR.WEAK_SLACK * 100)
            fams.add(c["family"])
    assert fams == set().union(*(SC.cell_families(cell, n, m) for n, m, _, _ in SC.CELLS[cell]))


def test_route_restatement():
    assert SC.route_of(48, 40, mid_route=0) == "general" and SC.route_of(128, 100, mid_route=0) == "big2"
    assert SC.route_of(64, 12, max_pivots=64 + 40) == "wg" and SC.route_of(64, 12, max_pivots=64) == "general"
    assert SC.route_of(32, 0) == "general" and SC.route_of(33, 0) == "general" and SC.route_of(257, 5) == "general"
    assert SC.route_of(64, 65) == "wg2" and SC.route_of(64, 129) == "general" and SC.route_of(65, 129) == "big2"


def _k40_node(need_two_sided=False):
    n, m, p, nodes = SC.cell_cases("f32_call")[0]
    for c in nodes:
        l, u = c["rec"][5], c["rec"][6]
        both = np.flatnonzero((c["side"] != 0) & np.isfinite(l) & np.isfinite(u))
        if c["family"] == "k40" and (both.size or not need_two_sided):
            return c, both
    raise AssertionError("no such node")


def _bar(oracle):
    """The accuracy bar of tests/test_gpu_solve_reference.py on the k40 family of the f32_call cell."""
    n, m, p, nodes = SC.cell_cases("f32_call")[0]
    ref = SC.oracle_solve(oracle, nodes, nodes[0]["w"])
    e = max(SR.node_error(ref["z"][i], SC.truth(c)[0], n) for i, c in enumerate(nodes) if c["family"] == "k40")
    return SR.accuracy_bar(e)


def test_teeth_wrong_side():
    c, both = _k40_node(need_two_sided=True)
    side = c["side"].copy()
    side[both[0]] *= -1
    z, info = SR.solve_reference(*c["rec"], c["w"], side)
    assert not info["ok"] and ("wrong sign" in info["why"] or "infeasible" in info["why"]), info


def test_teeth_symmetrised_problem(oracle):
    n, m, p, nodes = SC.cell_cases("f32_call")[0]
    c = next(c for c in nodes if c["family"] == "nearsym")
    Q = c["rec"][0]
    zs, info = SR.solve_reference(0.5 * (Q + Q.T), *c["rec"][1:], c["w"], c["side"])
    assert info["ok"]                                                   # (the symmetrised node's own solution)
    ok, why, _ = SR.certificate(zs, *c["rec"], c["w"], c["side"])
    assert not ok and "stationarity" in why
    e = SR.node_error(zs, SC.truth(c)[0], n)
    assert 1e-9 < e < 1e-5 and e > _bar(oracle)


def test_teeth_small_noise(oracle):
    c, _ = _k40_node()
    zt = SC.truth(c)[0]
    z = np.asarray(zt, dtype=np.float64) + 1e-11 * np.random.default_rng(1).standard_normal(zt.size)
    assert SR.node_error(z, zt, c["rec"][0].shape[0]) > _bar(oracle)
    z[c["rec"][0].shape[0]:][c["side"] == 0] = 0.0
    assert not SR.certificate(z, *c["rec"], c["w"], c["side"])[0]


def test_teeth_wrong_sign_convention(oracle):
    c, _ = _k40_node()
    n = c["rec"][0].shape[0]
    zt = SC.truth(c)[0]
    z = zt.copy()
    z[n:] = -z[n:]
    ok, why, _ = SR.certificate(z, *c["rec"], c["w"], c["side"])
    assert not ok and "wrong sign" in why
    assert SR.node_error(z, zt, n) > _bar(oracle)


@pytest.mark.parametrize("cell", list(SC.CELLS))
def test_oracle_against_the_truth(oracle, cell, capsys):
    tally, fails = {}, []
    for n, m, p, nodes in _all_nodes(cell):
        ref = SC.oracle_solve(oracle, nodes, nodes[0]["w"])
        fails += SC.check_against_truth(nodes, [SC.truth(c) for c in nodes], ref, f"{cell} ({n}, {m})", tally)
    with capsys.disabled():
        print(f"\n[oracle {cell}] " + "  ".join(f"{f} {t[0]:.1e}/{t[1]}" for f, t in sorted(tally.items())))
    assert not fails, "\n".join(fails[:12])
    assert "mask-unsafe" not in tally
    for f, (e, cnt) in tally.items():
        assert e <= ORACLE_CAPS[f][1], f"{cell}: the oracle's error on {f} is {e:.2e}, cap {ORACLE_CAPS[f][1]:.1e}"


def test_budget_case_is_within_its_budget(oracle):
    """The general cell of the GPU test runs a fused shape with a pivot budget of n + 40: the oracle solves every case within it."""
    n, m, p, nodes = SC.cell_cases("wg")[2]
    assert (n, m) == (64, 12)
    ref = SC.oracle_solve(oracle, nodes, nodes[0]["w"], max_pivots=n + 40)
    assert np.all(ref["status"] == 1) and ref["pivots"].max() <= n + 40
