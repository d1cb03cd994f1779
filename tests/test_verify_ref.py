"""The verify reference (tests/verify_ref.py) and its case generators (tests/verify_cases.py) checked on the CPU:

* the interval [r_lo, r_hi] contains r* computed at 50 digits (mpmath) for k <= 32;
* on well-conditioned nodes the reference decides as the C oracle does wherever its interval does not straddle the threshold;
* every generated case lands where it is meant to: classification margins, cond(A_bar with unit columns), |q~|, and r* on the
  requested side of the band [0.5 tol, 2 tol].
"""
import itertools

import mpmath
import numpy as np
import pytest

import verify_cases as VC
import verify_ref as VR

TOL = 1e-4


def _mp_rstar(rec, ref, dps=50):
    """r* at `dps` digits: q~ from the records, then the bounded least squares by enumerating the free sets (k <= 10), or the
    reference's free set solved at that precision and confirmed optimal by its KKT conditions (larger k)."""
    Q, R, qd, A, B, l, u, x, w = rec
    with mpmath.workdps(dps):
        mf = lambda a: mpmath.matrix(np.asarray(a).tolist())
        qt = mf(Q) * mf(x.reshape(-1, 1)) + mf(R) * mf(w.reshape(-1, 1)) + mf(qd.reshape(-1, 1))
        cls = ref.cls[ref.cols]
        Ab = mf((A[ref.cols] * np.where(cls == 2, -1.0, 1.0)[:, None]).T) if ref.k else None
        con = cls != 3
        n, k = len(qd), ref.k

        def solve_on(S):
            if not S:
                return mpmath.matrix(k, 1), qt
            As = mpmath.matrix(n, len(S))
            for c, j in enumerate(S):
                for i in range(n):
                    As[i, c] = Ab[i, j]
            y = mpmath.lu_solve(As.T * As, As.T * qt)     # (50 digits: cond^2 <= 1e10 leaves 40 of them)
            lam = mpmath.matrix(k, 1)
            for c, j in enumerate(S):
                lam[j] = y[c]
            return lam, qt - Ab * lam

        def kkt(lam, r):
            """optimality of lam: A_bar' (q~ - A_bar lam) vanishes on free columns and positive multipliers, is <= 0 elsewhere"""
            g = Ab.T * r
            scale = mpmath.norm(qt) * mpmath.mpf(10) ** (-dps + 10)
            for j in range(k):
                if con[j] and (lam[j] < 0 or g[j] > scale):
                    return False
                if (not con[j] or lam[j] > 0) and abs(g[j]) > scale:
                    return False
            return True

        if k == 0:
            return mpmath.norm(qt)
        Af = A[ref.cols].T

        def independent(S):
            sel, basis = [], np.zeros((n, 0))
            for j in S:
                cand = np.column_stack([basis, Af[:, j]])
                if np.linalg.matrix_rank(cand, tol=1e-10) > basis.shape[1]:
                    basis, sel = cand, sel + [j]
            return sel

        free = independent([j for j in range(k) if not con[j]])    # (a duplicated free column adds nothing)
        cons = [j for j in range(k) if con[j]]
        if k <= 10:
            best = None
            for t in range(len(cons) + 1):
                for sub in itertools.combinations(cons, t):
                    S = sorted(free + list(sub))
                    if len(S) > n:
                        continue
                    try:
                        lam, r = solve_on(S)
                    except (ZeroDivisionError, ValueError):   # dependent columns: an independent subset spans the same
                        continue
                    if all(lam[j] >= 0 for j in sub):
                        nr = mpmath.norm(r)
                        best = nr if best is None or nr < best else best
            return best
        le = ref.lam[ref.cols] * np.where(cls == 2, -1.0, 1.0)
        S = sorted(set(free) | {j for j in cons if le[j] > 0})
        Ssel = independent(S)                 # (the same projection; the solve needs full column rank)
        lam, r = solve_on(Ssel)
        assert kkt(lam, r), "the reference's free set is not optimal at 50 digits"
        return mpmath.norm(r)


def _small_cases():
    rng = np.random.default_rng(3)
    out = []
    for n, m in ((8, 10), (20, 24), (32, 32)):
        for fam in ("generic", "scale", "dup", "signforce"):
            for r in VC.RPERP:
                out.append(VC.make_case(rng, n, m, int(rng.integers(4, 7 if n == 8 else 16)), fam, rperp=r))
        for theta in (1e-2, 1e-3, 1e-4):
            for pair in ("pp", "pn", "eq"):
                for qn in (1.0, 1e5):
                    out.append(VC.make_case(rng, n, m, int(rng.integers(4, 7 if n == 8 else 12)), "parallel",
                                            rperp=VC.RPERP[len(out) % 4], qnorm=qn, theta=theta, pair=pair))
    return out


def test_interval_contains_50_digit_rstar():
    cases = _small_cases()
    for c in cases:
        ref = VR.verify_reference(*c["rec"], tol=TOL)
        assert ref.feasible and ref.k <= 32
        rs = _mp_rstar(c["rec"], ref)
        assert mpmath.mpf(ref.r_lo) <= rs <= mpmath.mpf(ref.r_hi), \
            f"{c['tag']}: r* = {mpmath.nstr(rs, 17)} outside [{ref.r_lo!r}, {ref.r_hi!r}]"
        assert ref.r_lo > 0.9 * ref.r_hi or ref.r_hi < 1e-9, f"{c['tag']}: interval [{ref.r_lo}, {ref.r_hi}] is loose"


def test_exact_threshold_cases_reference():
    """The exact cases' ax is exact; the classes flip with one ulp, and the reference predicts every path."""
    cases = VC.exact_threshold_cases(np.random.default_rng(11))
    paths = {}
    for c in cases:
        ref = VR.verify_reference(*c["rec"], tol=TOL)
        Q, R, qd, A, B, l, u, x, w = c["rec"]
        assert np.array_equal(ref.ax, A @ x)                   # exact in any order
        assert ref.path is not None, c["tag"]
        paths[c["tag"]] = ref.path
    assert paths["exact l+act ulp=+0 r=0e+00"] == 4 and paths["exact l+act ulp=-1 r=0e+00"] == 2
    assert paths["exact u-act ulp=+0 r=0e+00"] == 4 and paths["exact u-act ulp=+1 r=0e+00"] == 2
    assert paths["exact l-feas ulp=+0 r=0e+00"] == 2 and paths["exact l-feas ulp=-1 r=0e+00"] == 0


def test_reference_decides_as_the_oracle(oracle):
    """Well-conditioned nodes (no near-parallel pairs, |q~| = 1): wherever the interval decides, the C oracle's flag agrees."""
    rng = np.random.default_rng(17)
    agree = 0
    for n, m in ((10, 12), (24, 20), (40, 48)):
        for fam in ("generic", "scale", "dup", "signforce"):
            for r in VC.RPERP:
                c = VC.make_case(rng, n, m, int(rng.integers(4, min(n, m) - 2)), fam, rperp=r)
                ref = VR.verify_reference(*c["rec"], tol=TOL)
                d = ref.decided(TOL)
                sol, lam, path = oracle.verify_solution(*c["rec"], tol=TOL)
                if d is not None:
                    assert sol == d, f"{c['tag']}: oracle {sol} (path {path}), reference r* in [{ref.r_lo}, {ref.r_hi}]"
                    agree += 1
                if sol:
                    Q, R, qd, A, B, l, u, x, w = c["rec"]
                    ok, msg = VR.certificate(lam, ref, A, path, TOL, Qd=Q, R=R, xd=x, w=w, qd=qd)
                    assert ok, f"{c['tag']}: {msg}"
    assert agree >= 40


@pytest.mark.parametrize("cell", list(VC.CELLS))
def test_generators_land_where_meant(cell):
    n, m, (k0, k1), _ = VC.CELLS[cell]
    cases = VC.cell_cases(cell)
    routes = set()
    for c in cases:
        ref = VR.verify_reference(*c["rec"], tol=TOL)
        assert ref.feasible, c["tag"]
        act = ref.cls != 0
        assert act.sum() == ref.k and k0 <= ref.k <= k1, f"{c['tag']}: k = {ref.k}"
        assert np.all(ref.margin >= 4e-4), f"{c['tag']}: a row within {ref.margin.min():.1e} of a threshold"
        qn = float(np.linalg.norm(ref.qt))
        tag = c["tag"]
        if "|q|=" in tag:
            want_q = float(tag.split("|q|=")[1].split()[0])
            if "signforce" not in tag:
                assert 0.5 * want_q <= qn <= 2 * want_q + 1e-2, f"{tag}: |q~| = {qn:.2e}"
        if "theta=" in tag:
            theta = float(tag.split("theta=")[1].split()[0])
            assert ref.cond_eq >= 0.3 / theta, f"{tag}: cond_eq {ref.cond_eq:.1e} does not reflect theta"
        elif tag.startswith(("generic", "dup")):
            assert ref.cond_eq <= 1e3, f"{tag}: cond_eq {ref.cond_eq:.1e}"
        if c["want"] == "accept":
            assert ref.r_hi <= 0.5 * TOL, f"{tag}: meant to be accepted, r* in [{ref.r_lo}, {ref.r_hi}]"
        else:
            assert ref.r_lo > 2 * TOL, f"{tag}: meant to be rejected, r* in [{ref.r_lo}, {ref.r_hi}]"
        routes.add(VC.route_of(n, m, ref.k, cell))
    assert routes == {cell if cell != "wide_c5" else "wide_fast"}


def test_certificate_rejects_what_it_should():
    rng = np.random.default_rng(23)
    c = VC.make_case(rng, 20, 24, 8, "generic")
    Q, R, qd, A, B, l, u, x, w = c["rec"]
    ref = VR.verify_reference(*c["rec"], tol=TOL)
    ok, _ = VR.certificate(ref.lam, ref, A, 2, TOL, Qd=Q, R=R, xd=x, w=w, qd=qd)
    assert ok
    bad = ref.lam.copy(); bad[np.flatnonzero(ref.cls == 0)[0]] = 1e-30
    assert not VR.certificate(bad, ref, A, 2, TOL)[0]                       # inactive row carries a multiplier
    j = np.flatnonzero(ref.cls == 1)[0]
    bad = ref.lam.copy(); bad[j] = -2 * TOL
    assert not VR.certificate(bad, ref, A, 3, TOL)[0]                       # wrong sign beyond tol
    d = 1.9 * TOL / np.linalg.norm(A[j])
    bad = ref.lam.copy(); bad[j] += d                                       # a residual of 1.9e-4: the old 2e-4 bound let it pass
    assert not VR.certificate(bad, ref, A, 2, TOL, Qd=Q, R=R, xd=x, w=w, qd=qd)[0]
