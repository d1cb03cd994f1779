"""Every route of qpn_launch_verify_nodes (csrc/qpn_verify.hip) against the independent reference of tests/verify_ref.py.

verify_solution (src/qp_processing.jl:57-149) is the accept gate of the outer loop: a false accept reports a wrong equilibrium as
solved, a false reject costs sweeps.  The cases (tests/verify_cases.py) plant q~ = A_bar lam* + r_perp with r_perp exactly
orthogonal to range(A_bar), over near-parallel active pairs, row scales, |q~| up to 1e5, dependent rows, sign-forced fallbacks
and exact thresholds; the reference brackets r* = min over sign-feasible lam of |A_bar lam - q~| in [r_lo, r_hi].

* soundness, every case: an accept carries multipliers that pass verify_ref.certificate; r_lo > 2 * 1e-4 is rejected;
* completeness: r_hi <= 0.5 * 1e-4 is accepted wherever cond(A_bar with unit columns) <= 1e4 and |q~| <= 1e5;
* the route matrix: every cell received cases that must be accepted and cases that must be rejected;
* Engine.verify_nodes and Nodes.verify (resident records) give the same flags, paths and multipliers.
"""
import numpy as np
import pytest

import verify_cases as VC
import verify_ref as VR

pytestmark = pytest.mark.gpu
TOL = 1e-4
COND_MAX, QNORM_MAX = 1e4, 1e5


def _run(engine, recs, tol=TOL):
    from qpn_amd.engine import colmajor
    Q, R, qd, A, B, l, u, xd, w = recs
    sol, lam, path = engine.verify_nodes(colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u, xd, w, tol=tol)
    nodes = engine.upload_nodes(colmajor(Q), colmajor(R), qd, colmajor(A), colmajor(B), l, u)
    try:
        s2, l2, p2 = nodes.verify(xd, w, tol=tol)
    finally:
        nodes.close()
    return (np.asarray(sol), np.asarray(lam), np.asarray(path)), (np.asarray(s2), np.asarray(l2), np.asarray(p2))


def _check_batch(engine, cell, cases, tally):
    recs = VC.stack(cases)
    (sol, lam, path), (s2, l2, p2) = _run(engine, recs)
    # the two entry points: the same flags and paths; the same multipliers bit for bit, except in the overflow cell, where which
    # nodes win a slot of verify_wide_node's workspace (and which go to verify_stage1) depends on the order workgroups start
    assert np.array_equal(sol, s2) and np.array_equal(path, p2), f"{cell}: verify_nodes and Nodes.verify disagree"
    if cell != "mid_overflow":
        assert np.array_equal(lam, l2), f"{cell}: multipliers of verify_nodes and Nodes.verify differ"
    Q, R, qd, A, B, l, u, xd, w = recs
    fails = []
    for i, c in enumerate(cases):
        rec = c["rec"]
        ref = VR.verify_reference(*rec, tol=TOL)
        n, m = qd.shape[1], l.shape[1]
        route = VC.route_of(n, m, ref.k, cell)
        cs = tally.setdefault(route, dict(accept=0, reject=0, straddle=0, dependent=0, false_reject=0, n=0))
        cs["n"] += 1
        cs["dependent"] += int(ref.k > np.linalg.matrix_rank(A[i][ref.cols]) if ref.k else 0)
        qn = float(np.linalg.norm(ref.qt))
        what = (f"{cell}/{route} [{i}] {c['tag']}: n={n} m={m} k={ref.k} cond_eq={ref.cond_eq:.1e} |q~|={qn:.1e} "
                f"r* in [{ref.r_lo:.3e}, {ref.r_hi:.3e}] -> kernel flag {sol[i]} path {path[i]}")
        must_acc, must_rej = ref.r_hi <= 0.5 * TOL, ref.r_lo > 2 * TOL
        cs["accept"] += int(must_acc)
        cs["reject"] += int(must_rej)
        cs["straddle"] += int(ref.decided(TOL) is None)
        if sol[i] == 1:
            ok, msg = VR.certificate(lam[i], ref, A[i], int(path[i]), TOL, Qd=Q[i], R=R[i], xd=xd[i], w=w[i], qd=qd[i])
            if not ok:
                fails.append(f"false accept, certificate fails ({msg}): {what}")
        if must_rej and sol[i] != 0:
            fails.append(f"false accept: {what}")
        if must_acc and sol[i] != 1:
            if ref.cond_eq <= COND_MAX and qn <= QNORM_MAX:
                fails.append(f"false reject: {what}")
            else:
                cs["false_reject"] += 1
    return fails


@pytest.mark.parametrize("cell", list(VC.CELLS))
def test_verify_route_against_reference(engine, cell, capsys):
    tally = {}
    fails = _check_batch(engine, cell, VC.cell_cases(cell), tally)
    with capsys.disabled():
        for r, cs in sorted(tally.items()):
            print(f"\n[verify {cell}] route {r}: {cs}")
    assert not fails, "\n".join(fails[:12]) + (f"\n... {len(fails)} in all" if len(fails) > 12 else "")
    # the route matrix: the cell's own route received cases on both sides of the band (and, where the fast factor has to hand over
    # to the pivoted one, dependent rows)
    mine = tally.get(cell if cell != "wide_c5" else "wide_fast")
    assert mine is not None and mine["accept"] > 0 and mine["reject"] > 0, f"{cell}: route not covered on both sides: {tally}"
    if cell in ("mid_slots", "wide_fast", "wide_c5", "wide_pivoted"):
        assert mine["dependent"] > 0, f"{cell}: no case with dependent active rows"
    if cell == "mid_overflow":
        assert mine["n"] > VC.MID_SLOTS, "the overflow cell needs more nodes than verify_wide_node has slots"
    total = sum(cs["n"] for cs in tally.values())
    assert sum(cs["straddle"] for cs in tally.values()) <= 0.05 * total


def test_verify_exact_thresholds(engine):
    """ax exactly at fl(l + 1e-2), fl(u - 1e-2), fl(l - 1e-3), fl(u + 1e-3) and one ulp off: flag and path equal the reference's
    on verify_node32, verify_node64 and verify_wide_node (the same rows, padded with inactive rows to each class's shape)."""
    cases = VC.exact_threshold_cases(np.random.default_rng(11))
    for n_pad, m_pad in ((0, 0), (32, 30), (80, 60)):
        padded = [dict(c, rec=VC.pad_node(c["rec"], n_pad, m_pad)) for c in cases]
        recs = VC.stack(padded)
        (sol, lam, path), (s2, l2, p2) = _run(engine, recs)
        assert np.array_equal(sol, s2) and np.array_equal(path, p2) and np.array_equal(lam, l2)
        seen = set()
        for i, c in enumerate(padded):
            ref = VR.verify_reference(*c["rec"], tol=TOL)
            assert ref.path is not None, c["tag"]
            assert path[i] == ref.path and sol[i] == (ref.path in (2, 3)), \
                f"{c['tag']} (+{n_pad}, +{m_pad}): kernel flag {sol[i]} path {path[i]}, reference path {ref.path}"
            seen.add(ref.path)
        assert {0, 2, 4} <= seen


def test_verify_nondefault_tol(engine):
    """tol = 1e-6: the sign and residual test of :119 takes tol, the fallback of :138 keeps 1e-4.  A planted residual of 1e-5
    fails :119 and passes :138 (path 3); none passes :119 (path 2)."""
    rng = np.random.default_rng(5)
    for n, m, k in ((12, 16, 6), (48, 48, 20), (96, 80, 60)):
        cases = [VC.make_case(rng, n, m, k, "generic", rperp=r) for r in (0.0, 3e-7, 1e-5, 1e-5, 3e-4)]
        (sol, lam, path), _ = _run(engine, VC.stack(cases), tol=1e-6)
        assert list(path) == [2, 2, 3, 3, 4] and list(sol) == [1, 1, 1, 1, 0], f"{n}x{m}: paths {path}, flags {sol}"
        for i, c in enumerate(cases):
            ref = VR.verify_reference(*c["rec"], tol=1e-6)
            if sol[i]:
                Q, R, qd, A, B, l, u, xd, w = c["rec"]
                ok, msg = VR.certificate(lam[i], ref, A, int(path[i]), 1e-6, Qd=Q, R=R, xd=xd, w=w, qd=qd)
                assert ok, f"{n}x{m} case {i}: {msg}"
